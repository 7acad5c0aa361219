// host_units.cpp — the host-only units of the product (no GPU call in any of them), compiled by tests/host_sanitize/Makefile with
// g++ -fsanitize=thread and -fsanitize=address,undefined and run by the CPU suite (tests/test_host_sanitize.py).
//
//   thread_pool.hpp    ThreadPool (per-stream control-plane pool) and AsyncLane (the decode's host lane), used the way the engine
//                      uses them: a lane task that calls parallel_for while the posting thread waits; several engines' worth at once
//   control_plane.hpp  FIG parse, lock rule, CIF ring, ETI headers over the FIBs of synthetic ensembles, streams in parallel
//   worklist.hpp       frame records, header rows, wave-groups and slices of the MSC decode (with plain std::allocator lists)
//   launch_limits.hpp  the cut of [0, n) into launches of at most `limit` that the launch loops share, and which limits are refused
//   segment_layout.hpp the frame list, TF slots and logical CIF rows of random segments (with and without the lock-in skip, mis-numbered
//                      ordinals under ASan) and the session carry over runs of segments, against a per-TF list kept here
//   decoder_form.hpp   the decoder-form rule at both sides of every documented crossover, each knob's 0 / 1 / N reading, every forced form
//   scan_plan.hpp      the K1 scan's schedule (split scan, look-ahead pass, its table and passes) at both sides of every crossover
//   fifo_view.hpp      the closed-form FIFO / stale-tail views under random timing corrections, against a byte-level replay of
//                      cbWrite / sdr_read_fifo's copying rule (sdr_fifo.c:26-61)
//   synth.cpp          the modulator's bit content and sample generation (bounds, UB)
//   session_windows.hpp a session's device windows replayed on byte arrays sized exactly as planned: every byte still needed where the plan says
//   placement.hpp      the dealing rule of a batch over slices (Deal) and its inverse
//   capi_host.cpp      the GPU-free entries as linked into the library: their buffer caps (the fifo case)
// The reference's own data race (rtlsdr_callback writing sdr->input_buffer while the demod thread reads it, dab2eti.c:117-130)
// has no counterpart here: segments are handed over by value of their pointers and never written while a decode runs.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <tuple>
#include <thread>
#include <vector>

#include "../../include/dabhip.h"
#include "../../dabtools_amd/csrc/control_plane.hpp"
#include "../../dabtools_amd/csrc/decoder_form.hpp"
#include "../../dabtools_amd/csrc/fifo_view.hpp"
#include "../../dabtools_amd/csrc/launch_limits.hpp"
#include "../../dabtools_amd/csrc/scan_plan.hpp"
#include "../../dabtools_amd/csrc/segment_layout.hpp"
#include "../../dabtools_amd/csrc/session_windows.hpp"
#include "../../dabtools_amd/csrc/thread_pool.hpp"
#include "../../dabtools_amd/csrc/worklist.hpp"

using namespace dabhip;

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

template <class T>
using StdAlloc = std::allocator<T>;

static void test_pool_and_lane()
{
  ThreadPool pool(5);
  for (int round = 0; round < 400; ++round) {
    const int n = 1 + (round * 37) % 301;
    std::vector<int> hits(static_cast<size_t>(n), 0);
    pool.parallel_for(n, [&](int i) { hits[static_cast<size_t>(i)] += 1; });      // every index exactly once, visible after the call
    for (int h : hits) CHECK(h == 1);
  }
  pool.parallel_for(0, [&](int) { CHECK(false); });
  // the engine's pattern: the decode thread posts the control-plane pass to the lane and waits; the pass fans out over the pool
  AsyncLane lane;
  long total = 0;
  for (int round = 0; round < 200; ++round) {
    std::vector<long> part(64, 0);
    lane.post([&]() {
      pool.parallel_for(64, [&](int i) { part[static_cast<size_t>(i)] = i + round; });
      for (long p : part) total += p;
    });
    lane.wait();
    CHECK(part[63] == 63 + round);
  }
  CHECK(total == 200L * (63 * 64 / 2) + 64L * (199 * 200 / 2));
  // several posts before one wait run in order
  std::vector<int> order;
  for (int i = 0; i < 50; ++i) lane.post([&order, i]() { order.push_back(i); });
  lane.wait();
  CHECK(order.size() == 50);
  for (int i = 0; i < 50; ++i) CHECK(order[static_cast<size_t>(i)] == i);
  // a pool without workers: the caller does everything
  ThreadPool solo(0);
  int sum = 0;
  solo.parallel_for(10, [&](int i) { sum += i; });
  CHECK(sum == 45);
  // host placement (placement.hpp): workers and lanes are bound to their CPU list before they run anything.  (The CPU this process may use: what
  // the container's cpuset leaves; bind to the first one of it.)
  cpu_set_t allowed;
  CHECK(sched_getaffinity(0, sizeof allowed, &allowed) == 0);
  int cpu0 = -1;
  for (int c = 0; c < CPU_SETSIZE && cpu0 < 0; ++c)
    if (CPU_ISSET(c, &allowed)) cpu0 = c;
  CHECK(cpu0 >= 0);
  {
    ThreadPool bound(3, std::vector<int>{cpu0});
    std::atomic<int> elsewhere{0}, by_workers{0};
    const std::thread::id me = std::this_thread::get_id();
    for (int round = 0; round < 20; ++round)
      bound.parallel_for(64, [&](int) {
        if (std::this_thread::get_id() == me) return;                  // the caller takes part and is not bound
        ++by_workers;
        if (sched_getcpu() != cpu0) ++elsewhere;
      });
    CHECK(elsewhere.load() == 0);
    AsyncLane on_cpu(std::vector<int>{cpu0});
    int where = -1;
    on_cpu.post([&]() { where = sched_getcpu(); });
    on_cpu.wait();
    CHECK(where == cpu0);
  }
  // a CPU list that reaches beyond what the process is allowed on (a launcher's taskset): bound to the part inside; a list wholly outside: left alone
  {
    const int outside = CPU_SETSIZE - 1;                               // (no box has 1024 hardware threads in its cpuset)
    CHECK(!CPU_ISSET(outside, &allowed));
    AsyncLane partly(std::vector<int>{outside, cpu0});
    int where = -1;
    partly.post([&]() { where = sched_getcpu(); });
    partly.wait();
    CHECK(where == cpu0);
    AsyncLane none(std::vector<int>{outside});
    cpu_set_t got;
    CPU_ZERO(&got);
    none.post([&]() { CHECK(sched_getaffinity(0, sizeof got, &got) == 0); });
    none.wait();
    CHECK(CPU_EQUAL(&got, &allowed));
    CHECK(intersect_cpus({5, 1, 9}, {1, 2, 5}) == (std::vector<int>{5, 1}));
  }
  // the quota rule: cgroup v2's cpu.max
  CHECK(parse_cpu_max("max 100000") == 0 && parse_cpu_max("1600000 100000") == 16 && parse_cpu_max("150000 100000") == 2 && parse_cpu_max("") == 0);
  CHECK(usable_cpus() >= 1 && usable_cpus() <= static_cast<int>(allowed_cpus().size()));
  // two callers of one pool (the engine's decode thread and its host lane never overlap, but nothing must break if they did)
  {
    ThreadPool shared(4);
    std::vector<int> a(500, 0), b(500, 0);
    std::thread other([&]() { for (int r = 0; r < 50; ++r) shared.parallel_for(500, [&](int i) { a[static_cast<size_t>(i)] += 1; }); });
    for (int r = 0; r < 50; ++r) shared.parallel_for(500, [&](int i) { b[static_cast<size_t>(i)] += 1; });
    other.join();
    for (int i = 0; i < 500; ++i) CHECK(a[static_cast<size_t>(i)] == 50 && b[static_cast<size_t>(i)] == 50);
  }
  // the plan itself: disjoint chunks of a node's CPUs
  {
    const std::vector<std::vector<int>> plan = plan_placement({0, 1, 0, -1, 0}, {parse_cpulist("0-3,8-11"), parse_cpulist("4-7")});
    CHECK(plan.size() == 5 && plan[3].empty() && plan[1] == (std::vector<int>{4, 5, 6, 7}));
    CHECK(plan[0] == (std::vector<int>{0, 1}) && plan[2] == (std::vector<int>{2, 3, 8}) && plan[4] == (std::vector<int>{9, 10, 11}));
  }
}

// the FIBs and CRC flags of `ntf` transmission frames of one synthetic ensemble, as the FIC decode hands them to the control plane
static void make_fibs(int preset, uint64_t seed, int cif0, int ntf, std::vector<uint8_t>& fibs, std::vector<uint8_t>& ok)
{
  dabhip_synth_cfg cfg;
  CHECK(dabhip_synth_preset(preset, &cfg) == 0);
  cfg.seed = seed;
  cfg.cif_count0 = cif0;
  fibs.assign(static_cast<size_t>(ntf) * 384, 0);
  ok.assign(static_cast<size_t>(ntf) * 12, 1);
  for (int c = 0; c < 4 * ntf; ++c) CHECK(dabhip_synth_fibs(&cfg, c, fibs.data() + static_cast<size_t>(c) * 96) == 96);
}

// one engine's host side for a batch: control plane over the pool, then the work lists -- checked for internal consistency
static void control_and_worklist(int nstreams, int ntf, int64_t max_rows, unsigned salt)
{
  ThreadPool pool(3);
  std::vector<std::vector<uint8_t>> fibs(static_cast<size_t>(nstreams)), ok(static_cast<size_t>(nstreams));
  for (int b = 0; b < nstreams; ++b) {
    make_fibs(b % 2, 100 + salt + static_cast<unsigned>(b), (977 * b + static_cast<int>(salt)) % 5000, ntf, fibs[static_cast<size_t>(b)], ok[static_cast<size_t>(b)]);
    if (b % 5 == 3)                       // a stream that loses lock four TFs before its end: one TF with a failed FIB CRC (dab.c:55-61)
      ok[static_cast<size_t>(b)][static_cast<size_t>(12 * (ntf - 4) + 4)] = 0;
  }
  std::vector<ControlPlane> planes(static_cast<size_t>(nstreams));
  std::vector<JobList> jobs(static_cast<size_t>(nstreams));
  pool.parallel_for(nstreams, [&](int b) {
    const size_t sb = static_cast<size_t>(b);
    planes[sb] = ControlPlane();
    if (b % 7 == 6) planes[sb].set_filter(0x6ull);                 // sub-channel filter: SubChIds 1 and 2 only
    for (int t = 0; t < ntf; ++t) {
      planes[sb].on_tf(t, fibs[sb].data() + static_cast<size_t>(t) * 384, ok[sb].data() + static_cast<size_t>(t) * 12, jobs[sb]);
      if (planes[sb].locked() && t >= 10) {                // the cached header against the straightforward builder, at this TF's CIF counter
        uint8_t fast[kEtiHeaderMax], slow[kEtiHeaderMax];
        const int n1 = planes[sb].frame_header(fast), n2 = build_eti_header(slow, planes[sb].ensemble(), planes[sb].filter());
        CHECK(n1 == n2 && std::memcmp(fast, slow, static_cast<size_t>(n1)) == 0);
      }
    }
    if (planes[sb].locked() && b % 7 == 5) {                     // a filter set while a header is cached (the engine sets it on a new plane only): the cache goes
      const uint64_t before = planes[sb].filter();
      for (const uint64_t keep : {uint64_t(0x4), uint64_t(0), before}) {
        uint8_t fast[kEtiHeaderMax], slow[kEtiHeaderMax];
        planes[sb].set_filter(keep);
        const int n1 = planes[sb].frame_header(fast), n2 = build_eti_header(slow, planes[sb].ensemble(), keep);
        CHECK(n1 == n2 && std::memcmp(fast, slow, static_cast<size_t>(n1)) == 0);
      }
    }
  });
  std::vector<const ControlPlane*> plane_ptrs;
  std::vector<const JobList*> job_ptrs;
  std::vector<int> row_base, fib_base;
  size_t nf = 0;
  for (int b = 0; b < nstreams; ++b) {
    const size_t sb = static_cast<size_t>(b);
    plane_ptrs.push_back(&planes[sb]);
    job_ptrs.push_back(&jobs[sb]);
    row_base.push_back(15 + b * (4 * ntf + 15));
    fib_base.push_back(4 * ntf * b);
    if (b % 5 != 3) CHECK(static_cast<int>(jobs[sb].size()) == 4 * (ntf - 13));      // 10 TFs to lock (dab.c:50-53), 16 CIFs in the ring before the first frame
    else CHECK(static_cast<int>(jobs[sb].size()) == 4 * (ntf - 4 - 13));
    nf += jobs[sb].size();
  }
  PlanTable plans;
  MscWorkT<StdAlloc> work;
  std::string error;
  CHECK(prepare_msc_work(plans, pool, job_ptrs, plane_ptrs, row_base, fib_base, max_rows, work, &error));
  CHECK(work.nframes == nf && work.jobs.size() == nf && work.meta.size() == nf);
  CHECK(work.header_stride % 16 == 0 && work.headers.size() == nf * static_cast<size_t>(work.header_stride));
  // frame records are stream-major and carry the stream's own jobs
  size_t f = 0;
  for (int b = 0; b < nstreams; ++b)
    for (const EtiJob& j : jobs[static_cast<size_t>(b)]) {
      CHECK(work.jobs[f].stream == b && work.jobs[f].cif == j.first_cif);
      CHECK(work.meta[f].header_len == j.header_len && work.meta[f].fib_block == fib_base[static_cast<size_t>(b)] + j.first_cif);
      CHECK(std::memcmp(work.headers.data() + f * static_cast<size_t>(work.header_stride), jobs[static_cast<size_t>(b)].header(j), static_cast<size_t>(j.header_len)) == 0);
      CHECK(12 + 96 + work.meta[f].mst_bytes + 8 <= 6144 + 12);
      ++f;
    }
  // wave-groups: longest first, lanes name valid frames, every (frame, sub-channel of its layout) exactly once
  const auto& batch = work.batch;
  CHECK(batch.job_ids.size() % 64 == 0 && !batch.groups.empty());
  std::vector<int> decoded_bytes(nf, 0);
  int prev_steps = 1 << 30;
  for (const WaveGroup& g : batch.groups) {
    CHECK(g.nsteps <= prev_steps);
    prev_steps = g.nsteps;
    CHECK(g.count >= 1 && g.count <= 64 && g.first >= 0 && static_cast<size_t>(g.first + g.count) <= batch.job_ids.size());
    const CodewordPlan& p = plans[g.plan];
    CHECK(p.nsteps == g.nsteps && p.out_bytes == (p.nsteps - 6) / 8);
    for (int l = 0; l < g.count; ++l) {
      const int id = batch.job_ids[static_cast<size_t>(g.first + l)];
      CHECK(id >= 0 && static_cast<size_t>(id) < nf);
      CHECK(p.out_offset >= work.meta[static_cast<size_t>(id)].header_len + 96);
      CHECK(p.out_offset + p.out_bytes <= work.meta[static_cast<size_t>(id)].header_len + 96 + work.meta[static_cast<size_t>(id)].mst_bytes);
      decoded_bytes[static_cast<size_t>(id)] += (p.out_bytes + 7) & 0xfff8;
    }
  }
  for (size_t i = 0; i < nf; ++i) CHECK(decoded_bytes[i] == work.meta[i].mst_bytes);   // the sub-channels tile the MST exactly (misc.c:259-260)
  // slices partition the groups; record rows fit the cap (a single group may exceed it on its own)
  CHECK(batch.slice_start.front() == 0 && batch.slice_start.back() == static_cast<int>(batch.groups.size()));
  for (size_t s = 0; s + 1 < batch.slice_start.size(); ++s) {
    CHECK(batch.slice_start[s] < batch.slice_start[s + 1]);
    int64_t rows = 0;
    for (int g = batch.slice_start[s]; g < batch.slice_start[s + 1]; ++g) {
      CHECK(batch.groups[static_cast<size_t>(g)].dec_base == rows);
      rows += (batch.groups[static_cast<size_t>(g)].nsteps + 7) / 8 * 8;
    }
    CHECK(rows <= batch.max_dec_rows);
    CHECK(rows <= max_rows || batch.slice_start[s + 1] - batch.slice_start[s] == 1);
  }
}

// Pieces: [0, n) in order, without gap or overlap, every piece but the last full, none empty -- at the sizes where a launch loop can go wrong
static void launch_pieces(int64_t limit)
{
  for (int64_t n : {int64_t(0), int64_t(1), limit - 1, limit, limit + 1, 2 * limit + 3}) {
    const Pieces cut{n, limit};
    CHECK(cut.count() == (n + limit - 1) / limit);
    int64_t at = 0;
    for (int64_t i = 0; i < cut.count(); ++i) {
      CHECK(cut.first(i) == at);
      CHECK(cut.size(i) >= 1 && cut.size(i) <= limit);
      CHECK(i + 1 == cut.count() || cut.size(i) == limit);
      at += cut.size(i);
    }
    CHECK(at == n);
  }
}
static void test_launch_limits()
{
  for (int64_t limit : {int64_t(1), int64_t(3), int64_t(8), int64_t(32768), int64_t(65535), kMaxDecisionRows}) launch_pieces(limit);
  CHECK((Pieces{-5, 8}.count() == 0));
  // the defaults are today's constants; 0 keeps a default; what no launch could be made with is refused and leaves *out alone
  const int64_t zeros[kLaunchLimitCount] = {0, 0, 0, 0, 0, 0};
  LaunchLimits l;
  CHECK(launch_limits_from(zeros, &l) == nullptr);
  CHECK(l.decision_rows == (int64_t(48) << 20) && l.regroup_tiles == 32768 && l.fic_group_tiles == 32768 && l.gather_descs == 65535 &&
        l.fetch_words == (int64_t(1) << 18) && l.fft_chunk_tfs == 4096);
  const int64_t low[kLaunchLimitCount] = {1, 8, 1, 3, 1, 5};
  CHECK(launch_limits_from(low, &l) == nullptr);
  CHECK(l.decision_rows == 1 && l.regroup_tiles == 8 && l.fic_group_tiles == 1 && l.gather_descs == 3 && l.fetch_words == 1 && l.fft_chunk_tfs == 5);
  const LaunchLimits before = l;
  const int64_t bad[][kLaunchLimitCount] = {{-1, 0, 0, 0, 0, 0}, {0, 12, 0, 0, 0, 0}, {0, 4, 0, 0, 0, 0}, {0, 32776, 0, 0, 0, 0}, {0, -8, 0, 0, 0, 0}, {0, 0, 65536, 0, 0, 0},
                                            {0, 0, 0, 65536, 0, 0}, {0, 0, 0, -3, 0, 0}, {0, 0, 0, 0, -1, 0}, {0, 0, 0, 0, 0, -5}, {0, 0, 0, 0, 0, (int64_t(1) << 20) + 1}};
  for (const auto& v : bad) {
    CHECK(launch_limits_from(v, &l) != nullptr);
    CHECK(std::memcmp(&l, &before, sizeof l) == 0);
  }
}

// the longest code word an ETI frame can hold (EEP 4-B at n = 57: 43,782 steps, 5,472 bytes per CIF) through the control plane and the work lists: its plan
// stays inside the decoders' descrambling table (kMaxCodewordBytes), its decision rows are sized by its length in both layouts; one unit more is refused
static void largest_codeword()
{
  dabhip_synth_cfg cfg;
  CHECK(dabhip_synth_preset(1, &cfg) == 0);
  cfg.nsub = 1;
  cfg.sub[0].id = 5; cfg.sub[0].start_cu = 9; cfg.sub[0].slform = 1; cfg.sub[0].uep_index = 0; cfg.sub[0].eep_protlev = 7; cfg.sub[0].size_cu = 15 * 57;
  const int ntf = 16;
  std::vector<uint8_t> fibs(static_cast<size_t>(ntf) * 384), ok(static_cast<size_t>(ntf) * 12, 1);
  for (int c = 0; c < 4 * ntf; ++c) CHECK(dabhip_synth_fibs(&cfg, c, fibs.data() + static_cast<size_t>(c) * 96) == 96);
  ControlPlane plane;
  JobList jobs;
  for (int t = 0; t < ntf; ++t) plane.on_tf(t, fibs.data() + static_cast<size_t>(t) * 384, ok.data() + static_cast<size_t>(t) * 12, jobs);
  CHECK(plane.fault() == 0 && jobs.size() == 12);
  ThreadPool pool(2);
  std::vector<const ControlPlane*> plane_ptrs = {&plane};
  std::vector<const JobList*> job_ptrs = {&jobs};
  std::vector<int> row_base = {15}, fib_base = {0};
  for (int64_t wave_max : {int64_t(0), int64_t(12288)}) {
    PlanTable plans;
    MscWorkT<StdAlloc> work;
    std::string error;
    CHECK(prepare_msc_work(plans, pool, job_ptrs, plane_ptrs, row_base, fib_base, int64_t(48) << 20, work, &error, nullptr, wave_max));
    CHECK(plans.plans().size() == 1 && work.batch.groups.size() == 1 && work.batch.wave_form == (wave_max > 0));
    const CodewordPlan& p = plans[0];
    CHECK(p.nsteps == 43782 && p.out_bytes == 5472 && p.out_bytes <= kMaxCodewordBytes && p.start_bit == 9 * 64);
    CHECK(p.out_offset + p.out_bytes + 8 <= kEtiBytes && work.meta[0].mst_bytes == 5472);
    CHECK(work.batch.max_dec_rows == (wave_max > 0 ? int64_t(64) * 730 : int64_t(43784)));
  }
  std::vector<SubChannel> active = plane.layouts().back();
  CHECK(active.size() == 1 && layout_fault(active, 16) == 0);
  active[0].size_cu = 15 * 58;                             // one unit more: past CU 863
  active[0].bitrate = 32 * 58;
  CHECK(layout_fault(active, 16) & kFaultOutsideCif);
  static_assert(kMaxCodewordWords * 4 == kMaxCodewordBytes && kMaxCodewordBytes >= kEtiBytes, "the table covers every code word of a frame");
}

static void test_control_and_worklist()
{
  test_launch_limits();
  largest_codeword();
  control_and_worklist(24, 30, int64_t(48) << 20, 0);
  control_and_worklist(9, 22, 20000, 1);                 // a small record cap: many slices
  // several engines' host sides at once in one process (dabhip_multi: one lane + one pool per slice)
  std::vector<std::unique_ptr<AsyncLane>> lanes;
  for (int i = 0; i < 4; ++i) lanes.emplace_back(new AsyncLane());
  for (int i = 0; i < 4; ++i) lanes[static_cast<size_t>(i)]->post([i]() { control_and_worklist(10 + i, 24, int64_t(1) << 20, 10u * static_cast<unsigned>(i)); });
  for (auto& l : lanes) l->wait();
}

// one random segment: the scan's records as K1 writes them ({status, ordinal}; a stream's demodulated TFs numbered densely from ord_done on)
struct RandomSegment {
  int nstreams, max_calls;
  std::vector<IntPair> info;
  std::vector<int> ncalls, nnew, defer;
  std::vector<StreamCarry> carry;
};
static RandomSegment random_segment(std::mt19937& rng)
{
  RandomSegment r;
  r.nstreams = 1 + static_cast<int>(rng() % 64);
  r.max_calls = 1 + static_cast<int>(rng() % 12);
  r.info.assign(static_cast<size_t>(r.nstreams) * r.max_calls, IntPair{0, -1});
  r.ncalls.resize(r.nstreams);
  r.nnew.assign(r.nstreams, 0);
  r.defer.resize(r.nstreams);
  r.carry.resize(r.nstreams);
  for (int b = 0; b < r.nstreams; ++b) {
    StreamCarry& c = r.carry[b];
    c.keep = static_cast<int>(rng() % 5);
    c.ord_done = static_cast<int>(rng() % 1000);
    r.ncalls[b] = static_cast<int>(rng() % (r.max_calls + 1));
    for (int k = 0; k < r.ncalls[b]; ++k) {
      const int status = static_cast<int>(rng() % 3);
      r.info[static_cast<size_t>(b) * r.max_calls + k] = IntPair{status, status == 2 ? c.ord_done + r.nnew[b]++ : -1};
    }
    r.defer[b] = static_cast<int>(rng() % (r.nnew[b] + 1));
  }
  return r;
}

static void test_layout()
{
  std::mt19937 rng(11);
  using Frame = std::tuple<int, int, int, int>;            // stream, call, slot, row
  for (int trial = 0; trial < 400; ++trial) {
    const RandomSegment r = random_segment(rng);
    const size_t nd = static_cast<size_t>(r.nstreams) * r.max_calls;
    const std::vector<int> no_defer(r.nstreams, 0);
    std::multiset<Frame> with_skip, without_skip;
    for (int pass = 0; pass < 2; ++pass) {                 // 0: the lock-in skip as drawn, 1: every deferred count 0
      SegmentLayout L;
      std::vector<IntPair> frames(nd, IntPair{-1, -1});    // exactly the engine's sizes: ASan sees a write beyond them
      std::vector<int> slot(nd, -1), row(nd, -1);
      std::string error;
      CHECK(layout_segment(r.info.data(), r.max_calls, r.ncalls.data(), r.carry, pass ? no_defer.data() : r.defer.data(), L, frames.data(), slot.data(), row.data(), &error));
      int ntf = 0, ndefer = 0;
      for (int b = 0; b < r.nstreams; ++b) {
        CHECK(L.nnew[b] == r.nnew[b] && L.ndefer_of[b] == (pass ? 0 : r.defer[b]));
        ntf += r.nnew[b];
        ndefer += L.ndefer_of[b];
        CHECK(L.tf_base[b + 1] == L.tf_base[b] + r.carry[b].keep + r.nnew[b] && L.fib_base[b] == 4 * L.tf_base[b]);
        if (b + 1 < r.nstreams) CHECK(L.row_base[b + 1] - L.row_base[b] == kRowLead + 4 * (r.carry[b].keep + r.nnew[b]));
      }
      CHECK(L.tf_base[0] == 0 && L.row_base[0] == kRowLead && L.ntf == ntf && L.nmsc == ntf - ndefer);
      CHECK(L.next_row == L.row_base[r.nstreams - 1] - kRowLead + kRowLead + 4 * (r.carry[r.nstreams - 1].keep + r.nnew[r.nstreams - 1]));
      // every list index in [0, ntf) written, nothing behind it, every demodulated call of every stream there once
      std::set<std::pair<int, int>> calls;
      std::vector<std::vector<std::pair<int, int>>> of_stream(r.nstreams);   // (call, list index)
      for (size_t i = 0; i < nd; ++i) {
        if (i >= static_cast<size_t>(ntf)) { CHECK(frames[i].x == -1 && slot[i] == -1 && row[i] == -1); continue; }
        const int b = frames[i].x, k = frames[i].y;
        CHECK(b >= 0 && b < r.nstreams && k >= 0 && k < r.ncalls[b] && r.info[static_cast<size_t>(b) * r.max_calls + k].x == 2);
        CHECK(calls.insert({b, k}).second);
        of_stream[b].push_back({k, static_cast<int>(i)});
        (pass ? without_skip : with_skip).insert(Frame{b, k, slot[i], row[i]});
      }
      CHECK(static_cast<int>(calls.size()) == ntf);
      for (int b = 0; b < r.nstreams; ++b) {
        std::sort(of_stream[b].begin(), of_stream[b].end());
        CHECK(static_cast<int>(of_stream[b].size()) == r.nnew[b]);
        for (int i = 0; i < r.nnew[b]; ++i) {
          const int at = of_stream[b][i].second, local = r.carry[b].keep + i;
          CHECK(slot[at] == L.tf_base[b] + local && row[at] == L.row_base[b] + 4 * local);      // contiguous from tf_base[b] + keep, in call order
          CHECK((at >= L.nmsc) == (i < L.ndefer_of[b]));                                        // the deferred ones: the stream's first new TFs, behind nmsc
        }
      }
    }
    CHECK(with_skip == without_skip);                      // the skip only re-orders the list
    // mis-numbered ordinals (one of them off by one, either way): refused with the error text, nothing written out of bounds
    std::vector<size_t> demodulated;
    for (size_t i = 0; i < nd; ++i)
      if (r.info[i].x == 2) demodulated.push_back(i);
    if (!demodulated.empty()) {
      std::vector<IntPair> bad = r.info;
      bad[demodulated[rng() % demodulated.size()]].y += (rng() & 1) ? 1 : -1;
      SegmentLayout L;
      std::vector<IntPair> frames(nd);
      std::vector<int> slot(nd), row(nd);
      std::string error;
      CHECK(!layout_segment(bad.data(), r.max_calls, r.ncalls.data(), r.carry, r.defer.data(), L, frames.data(), slot.data(), row.data(), &error));
      CHECK(error == "decode: the calls' ordinals do not number this segment's transmission frames");
    }
  }
}

// a session: StreamCarry::advance over a random run of segments against one flag per TF of the whole session, kept here
static void test_carry()
{
  std::mt19937 rng(13);
  for (int trial = 0; trial < 60; ++trial) {
    const int nstreams = 1 + static_cast<int>(rng() % 8), max_calls = 9;
    std::vector<StreamCarry> carry(nstreams);
    for (StreamCarry& c : carry) {
      c.keep = 3;                                          // (stale values: reset() is what a fresh decode starts from)
      c.msc_missing.assign(5, 1);
      c.reset();
      CHECK(c.keep == 0 && c.prev_used == 0 && c.calls_done == 0 && c.ord_done == 0 && c.last_keep == 0 && c.msc_missing.empty());
    }
    std::vector<std::vector<uint8_t>> missing(nstreams);   // per stream: TF i of the session had its MSC part deferred
    for (int segment = 0; segment < 40; ++segment) {
      std::vector<IntPair> info(static_cast<size_t>(nstreams) * max_calls, IntPair{0, -1});
      std::vector<int> ncalls(nstreams), defer(nstreams), nnew(nstreams, 0), keep_before(nstreams);
      for (int b = 0; b < nstreams; ++b) {
        ncalls[b] = static_cast<int>(rng() % (max_calls + 1));
        for (int k = 0; k < ncalls[b]; ++k)
          if (rng() % 3) info[static_cast<size_t>(b) * max_calls + k] = IntPair{2, static_cast<int>(missing[b].size()) + nnew[b]++};
        defer[b] = (rng() % 4 == 0) ? static_cast<int>(rng() % (nnew[b] + 1)) : 0;
        keep_before[b] = carry[b].keep;
      }
      SegmentLayout L;
      std::vector<IntPair> frames(info.size());
      std::vector<int> slot(info.size()), row(info.size());
      std::string error;
      CHECK(layout_segment(info.data(), max_calls, ncalls.data(), carry, defer.data(), L, frames.data(), slot.data(), row.data(), &error));
      for (int b = 0; b < nstreams; ++b) {
        carry[b].advance(L, b);
        for (int i = 0; i < nnew[b]; ++i) missing[b].push_back(i < defer[b] ? 1 : 0);
        const StreamCarry& c = carry[b];
        const int total = static_cast<int>(missing[b].size());
        CHECK(c.last_keep == keep_before[b] && c.prev_used == keep_before[b] + nnew[b] && c.keep == std::min(4, c.prev_used) && c.ord_done == total);
        CHECK(c.prev_tf_base == L.tf_base[b] && c.prev_row_base == L.row_base[b]);
        // the flags follow a TF from "deferred in this segment" to "carried slot of the next" to gone: slot j of the layout is TF total - prev_used + j
        CHECK(static_cast<int>(c.msc_missing.size()) == c.prev_used);
        for (int j = 0; j < c.prev_used; ++j) CHECK(c.msc_missing[j] == missing[b][static_cast<size_t>(total - c.prev_used + j)]);
      }
    }
  }
}

// The decoder-form rule: the expected forms are the rule as the engine spelled it out before it moved to decoder_form.hpp (launch_decode_batch,
// fic_decode_slots_async, msc_prepare), at the documented crossovers (include/dabhip.h)
static void test_forms()
{
  const int AUTO = DABHIP_FORM_AUTO, WAVE = DABHIP_FORM_WAVE, LANE = DABHIP_FORM_LANE, TWO = DABHIP_FORM_TWO, PLAIN = DABHIP_FORM_TWO_PLAIN, FOUR = DABHIP_FORM_FOUR;
  const FormKnobs def;
  CHECK(def.wave_max_codewords == 12288 && def.wave_max_fic_blocks == 3072 && def.two_lanes_max_groups == 1536 && def.four_lanes_max_groups == 800 &&
        !def.two_lanes_plain && def.fic_four_lanes_max_tiles == 128);
  // MSC, defaults: a batch in the wave form runs it whatever else holds; then four lanes up to 800 groups, two up to 1,536, one above
  struct { int forced; bool soft, wave_batch; int ngroups, want; } msc[] = {
      {AUTO, false, true, 10, WAVE},  {AUTO, true, true, 10, WAVE},    {FOUR, false, true, 10, WAVE},   {AUTO, false, false, 1, FOUR},
      {AUTO, false, false, 800, FOUR}, {AUTO, false, false, 801, TWO}, {AUTO, false, false, 1536, TWO}, {AUTO, false, false, 1537, LANE},
      {AUTO, false, false, 100000, LANE},
      // soft decisions: the lane form whatever the size and whatever is forced (the wave form apart: that is the batch's)
      {AUTO, true, false, 1, LANE},   {AUTO, true, false, 801, LANE},  {TWO, true, false, 5, LANE},     {PLAIN, true, false, 5, LANE},
      {FOUR, true, false, 5, LANE},   {LANE, true, false, 5, LANE},    {WAVE, true, false, 5, LANE},
      // forced forms, hard decisions, at sizes where the rule would say otherwise (WAVE forced on a batch that is not in the wave form: lanes)
      {LANE, false, false, 5, LANE},  {TWO, false, false, 5, TWO},     {TWO, false, false, 5000, TWO},  {PLAIN, false, false, 5, PLAIN},
      {PLAIN, false, false, 5000, PLAIN}, {FOUR, false, false, 5000, FOUR}, {WAVE, false, false, 5, LANE}};
  for (const auto& t : msc) CHECK(msc_form(def, t.forced, t.soft, t.wave_batch, t.ngroups) == t.want);
  // each knob's 0 / 1 / N reading
  struct { int two, four; bool plain; int ngroups, want; } knobs[] = {
      {0, 0, false, 1, LANE},     {0, 0, true, 1, LANE},      {1, 0, false, 100000, TWO}, {1, 0, true, 100000, PLAIN}, {0, 1, false, 100000, FOUR},
      {1, 1, false, 100000, FOUR}, {40, 0, false, 40, TWO},   {40, 0, false, 41, LANE},   {40, 20, false, 20, FOUR},   {40, 20, false, 21, TWO},
      {40, 20, true, 21, PLAIN},  {40, 20, true, 20, FOUR},   {20, 40, false, 30, FOUR},  {20, 40, false, 41, LANE},   {1536, 800, true, 801, PLAIN}};
  for (const auto& t : knobs) {
    FormKnobs k;
    k.two_lanes_max_groups = t.two;
    k.four_lanes_max_groups = t.four;
    k.two_lanes_plain = t.plain;
    CHECK(msc_form(k, AUTO, false, false, t.ngroups) == t.want);
    CHECK(msc_form(k, AUTO, true, false, t.ngroups) == LANE);
  }
  // the work-list build's bound: the knob, or all / nothing under a forced form
  CHECK(msc_wave_max(def, AUTO) == 12288 && msc_wave_max(def, WAVE) == INT64_MAX);
  for (int f : {LANE, TWO, PLAIN, FOUR}) CHECK(msc_wave_max(def, f) == 0);
  // FIC, defaults: the wave form up to 3,072 blocks (hard and soft), four lanes per block up to 128 tiles (hard only), one lane above
  struct { int forced; bool soft; int nblocks, ntiles, want; } fic[] = {
      {AUTO, false, 4, 1, WAVE},       {AUTO, false, 3072, 48, WAVE},   {AUTO, true, 3072, 48, WAVE},    {AUTO, false, 3073, 49, FOUR},
      {AUTO, false, 3076, 49, FOUR},   {AUTO, false, 8192, 128, FOUR},  {AUTO, false, 8196, 129, LANE},  {AUTO, true, 3076, 49, LANE},
      {AUTO, true, 8196, 129, LANE},   {WAVE, false, 100000, 1563, WAVE}, {WAVE, true, 100000, 1563, WAVE}, {LANE, false, 4, 1, LANE},
      {LANE, true, 4, 1, LANE},        {FOUR, false, 4, 1, FOUR},       {FOUR, false, 100000, 1563, FOUR}, {FOUR, true, 4, 1, LANE}};
  for (const auto& t : fic) CHECK(fic_form(def, t.forced, t.soft, t.nblocks, t.ntiles) == t.want);
  struct { int wave, four, nblocks, ntiles, want; } fknobs[] = {
      {0, 0, 4, 1, LANE},     {0, 1, 400000, 6250, FOUR}, {0, 10, 640, 10, FOUR}, {0, 10, 644, 11, LANE}, {640, 0, 640, 10, WAVE},
      {640, 0, 644, 11, LANE}, {640, 128, 644, 11, FOUR}, {3, 128, 4, 1, FOUR}};
  for (const auto& t : fknobs) {
    FormKnobs k;
    k.wave_max_fic_blocks = t.wave;
    k.fic_four_lanes_max_tiles = t.four;
    CHECK(fic_form(k, AUTO, false, t.nblocks, t.ntiles) == t.want);
  }
  // what set_decoder_forms admits
  for (int f = -3; f < 8; ++f) {
    CHECK(msc_form_valid(f) == (f >= -1 && f <= 4));
    CHECK(fic_form_valid(f) == (f == AUTO || f == WAVE || f == LANE || f == FOUR));
  }
}

// The scan's schedule: the expected values are the rule as Engine::scan_streams spelled it out before it moved to scan_plan.hpp (use_spec, nspec, passes,
// call_limit, the fetch's word count), at every crossover
static void test_scan()
{
  const ScanKnobs def;
  CHECK(def.hypotheses == 33 && def.spec_max_streams == 4);
  // nstreams streams of `calls` complete calls each, `done` of them scanned by an earlier segment
  auto plan = [](int nstreams, int calls, int done, bool afc, bool full_scan, bool cont, int mode, const ScanKnobs& k) {
    const std::vector<int> ncalls(static_cast<size_t>(nstreams), calls), calls_done(static_cast<size_t>(nstreams), done);
    return plan_scan(nstreams, ncalls.data(), calls_done.data(), afc, full_scan, cont, mode, k);
  };
  const size_t state_words = sizeof(StreamState) / 4;
  // default mode: the pass for at most 4 streams of at least 16 calls; forced: up to 512 streams, however few calls; off: never.  The split scan runs in all three
  struct { int nstreams, calls, mode; bool ahead; } rule[] = {
      {4, 16, -1, true},  {5, 16, -1, false},  {4, 15, -1, false}, {1, 16, -1, true},  {1, 15, -1, false}, {4, 1000, -1, true}, {5, 1000, -1, false},
      {512, 1, 1, true},  {513, 1, 1, false},  {513, 1000, 1, false}, {5, 15, 1, true}, {1, 1000, 0, false}, {4, 16, 0, false}};
  for (const auto& t : rule) {
    const ScanPlan p = plan(t.nstreams, t.calls, 0, false, false, false, t.mode, def);
    CHECK(p.split && p.ahead == t.ahead && p.max_calls == t.calls && p.ndesc == static_cast<size_t>(t.nstreams) * t.calls && p.nhyp == 33);
    CHECK(p.result_words == static_cast<size_t>(t.nstreams) + 1 + (t.ahead ? 1 : 0) + p.ndesc * 2 + t.nstreams * state_words);
  }
  // the software AFC and the full scan: the reference's order -- no split, no pass, whatever the mode; no violation marks in the fetch
  for (int mode : {-1, 0, 1})
    for (int which = 0; which < 2; ++which) {
      const ScanPlan p = plan(2, 64, 0, which == 0, which == 1, false, mode, def);
      CHECK(!p.split && !p.ahead && p.max_calls == 64 && p.ndesc == 128 && p.result_words == 128 * 2 + 2 * state_words);
    }
  // the table: nspec = min(max_calls, clamp(2^20 / nstreams, 64, 4096)) -- 2^20 / nstreams crosses 4096 at 256 streams and 64 at 16,384
  struct { int nstreams, calls, nspec; } table[] = {{1, 5000, 4096},   {255, 5000, 4096},  {256, 5000, 4096},  {257, 5000, 4080},   {512, 5000, 2048},
                                                    {16000, 100, 65},  {16384, 100, 64},   {16385, 100, 64},   {20000, 100, 64},    {4, 100, 100},
                                                    {4, 1, 1},         {20000, 10, 10}};
  for (const auto& t : table) CHECK(plan(t.nstreams, t.calls, 0, false, false, false, 1, def).nspec == t.nspec);
  // the passes: ceil(max_calls / nspec), at most 16; every pass but the last is followed by a chain of nspec calls, the last by one to the end
  struct { int nstreams, calls, nspec, passes; } passes[] = {{1, 4096, 4096, 1},   {1, 4097, 4096, 2},   {1, 65536, 4096, 16}, {1, 65537, 4096, 16}, {1, 200000, 4096, 16},
                                                            {512, 2048, 2048, 1}, {512, 2049, 2048, 2}, {512, 32768, 2048, 16}, {512, 32769, 2048, 16}, {4, 16, 16, 1}};
  for (const auto& t : passes) {
    const ScanPlan p = plan(t.nstreams, t.calls, 0, false, false, false, 1, def);
    CHECK(p.ahead && p.nspec == t.nspec && p.passes == t.passes);
    for (int r = 0; r < p.passes; ++r) CHECK(p.pass_limit(r) == (r + 1 < t.passes ? t.nspec : -1));
  }
  // the chain in front of the first pass: seven calls of a fresh decode, none of a session's further segment
  CHECK(plan(2, 64, 0, false, false, false, -1, def).first_limit == 7 && plan(2, 64, 0, false, false, true, -1, def).first_limit == 0);
  CHECK(plan(2, 64, 0, false, false, true, -1, def).ahead && plan(2, 64, 0, false, false, true, 0, def).first_limit == 0);
  // a session's segments: the calls that became complete since the last one, at least one descriptor per stream
  {
    const ScanPlan one = plan(3, 40, 39, false, false, true, -1, def), none = plan(3, 40, 40, false, false, true, -1, def);
    CHECK(one.max_calls == 1 && one.ndesc == 3 && !one.ahead && one.nspec == 1 && one.passes == 1);
    CHECK(none.max_calls == 1 && none.ndesc == 3 && !none.ahead);
    const int ncalls[3] = {40, 10, 57}, done[3] = {39, 10, 40};
    const ScanPlan mixed = plan_scan(3, ncalls, done, false, false, true, -1, def);
    CHECK(mixed.max_calls == 17 && mixed.ndesc == 51 && mixed.ahead && mixed.nspec == 17 && mixed.first_limit == 0);
    const int done16[3] = {39, 10, 42};
    CHECK(!plan_scan(3, ncalls, done16, false, false, true, -1, def).ahead);      // 15 calls left
  }
  // the knobs: the window is odd within 3 .. 63; the default mode's largest batch within 0 .. 512
  struct { int hyp, want; } windows[] = {{33, 33}, {32, 33}, {0, 3}, {1, 3}, {2, 3}, {3, 3}, {4, 5}, {62, 63}, {63, 63}, {64, 63}, {1000, 63}, {-5, 3}};
  for (const auto& t : windows) {
    ScanKnobs k;
    k.hypotheses = t.hyp;
    CHECK(plan(1, 16, 0, false, false, false, -1, k).nhyp == t.want);
  }
  struct { int knob, nstreams; bool ahead; } batches[] = {{0, 1, false}, {-3, 1, false}, {1, 1, true}, {1, 2, false}, {8, 8, true}, {8, 9, false}, {1000, 512, true}, {1000, 513, false}};
  for (const auto& t : batches) {
    ScanKnobs k;
    k.spec_max_streams = t.knob;
    CHECK(plan(t.nstreams, 16, 0, false, false, false, -1, k).ahead == t.ahead);
  }
}

// byte-level replay of what sdr_read_fifo does to the 393216-byte frame buffer (sdr_fifo.c:43-61), on a stream whose byte at
// offset x is the tag x itself (64-bit), so a view can be compared position by position
static void test_fifo_views()
{
  std::mt19937 rng(7);
  for (int trial = 0; trial < 30; ++trial) {
    StreamState st;
    std::memset(&st, 0, sizeof st);
    fifo_reset(st);
    std::vector<int64_t> buffer(kTfBytes, -1);            // stream offset held at each buffer position (-1: calloc'ed zero)
    std::vector<int64_t> tail(kTailBytes, -1);            // the last kTailBytes as K1 carries them (here: tags instead of bytes), updated by read_source
    int64_t rd = 0, fed = 0;
    int most_segments = 0;
    for (int call = 0; call < 160; ++call) {
      const int r = static_cast<int>(rng() % 10);
      st.coarse_timeshift = r == 0 ? static_cast<int>(rng() % 380000) : 0;               // a coarse resync now and then
      // trial >= 15: a receiver clock that runs fast -- ever larger negative shifts for a long stretch, then ever smaller ones: every read short,
      // each shorter (or longer) than the one before.  As views these nested once per read (more than kMaxSeg: the engine used to give up).
      if (trial >= 15) st.fine_timeshift = -2 * (call < 70 ? call + 1 : 161 - call) - (r < 2 ? 2 * static_cast<int>(rng() % 5) : 0);
      else st.fine_timeshift = r < 7 ? static_cast<int>(rng() % 61) - 30 : -2 * static_cast<int>(rng() % 768);      // >= (768 - 1536) * 2, sdr_sync.c:197-201
      const int chunk = trial % 3 == 2 ? 2 * static_cast<int>(rng() % (kChunkBytes / 2 + 1)) : kChunkBytes;   // input_buffer_len: any even length
      const int shift = st.coarse_timeshift + st.fine_timeshift;
      fed += chunk;
      int64_t count = fed - rd;
      bool read = false;
      if (count >= 3 * kTfSamples) {
        read = true;
        if (shift > 0) {
          for (int p = 0; p < shift && p < kTfBytes && p < count; ++p) buffer[static_cast<size_t>(p)] = rd + p;      // the skipped bytes pass through the buffer
          rd += shift;
          count -= shift;
          const int len = count < kTfBytes ? static_cast<int>(count) : kTfBytes;
          for (int p = 0; p < len; ++p) buffer[static_cast<size_t>(p)] = rd + p;
          rd += len;
        } else {
          const int len = kTfBytes + shift;
          for (int p = 0; p < len; ++p) buffer[static_cast<size_t>(p)] = rd + p;
          rd += len;
        }
      }
      const FifoCall c = fifo_call(st, chunk);
      CHECK(!st.overflow);
      CHECK((c.status != 0) == read);
      CHECK(c.fifo_count == static_cast<int>(fed - rd));
      CHECK(st.consumed == rd && st.fed == fed);
      if (!read) continue;
      CHECK(st.view.nseg >= 1 && st.view.nseg <= kMaxSeg && (c.fresh == 1 || c.fresh == 2));
      most_segments = std::max(most_segments, st.view.nseg);
      for (int p = kTailStart; p < kTfBytes; ++p) {                                       // the tail bytes by the kernel's rule ...
        const int64_t src = read_source(st.view, c.fresh, p);
        if (src >= 0) tail[static_cast<size_t>(p - kTailStart)] = src;
        CHECK(buffer[static_cast<size_t>(p)] == tail[static_cast<size_t>(p - kTailStart)]);
      }
      int lo = 0;                                                                          // ... the views everything below them
      for (int i = 0; i < st.view.nseg && lo < kTailStart; ++i) {
        CHECK(st.view.seg_end[i] > lo || (i == 0 && st.view.seg_end[0] >= 0));
        const int hi = std::min(st.view.seg_end[i], kTailStart);
        for (int p = lo; p < hi; p += 997)                                                // sampled positions plus both ends
          CHECK(buffer[static_cast<size_t>(p)] == (st.view.seg_src[i] < 0 ? -1 : st.view.seg_src[i] + p));
        if (hi > lo) {
          const int p = hi - 1;
          CHECK(buffer[static_cast<size_t>(p)] == (st.view.seg_src[i] < 0 ? -1 : st.view.seg_src[i] + p));
        }
        lo = st.view.seg_end[i];
      }
      CHECK(lo >= kTailStart);
      // whatever the views still refer to is recent: nothing pins the stream's past (Engine::stream_need_from)
      if (shift <= 0 && shift >= -kTailBytes)
        for (int i = 0; i < st.view.nseg; ++i) CHECK(st.view.seg_src[i] < 0 || i == 0);
    }
    CHECK(most_segments <= 6);
  }
}

// the GPU-free entries of the C ABI (capi_host.cpp) with buffers of exactly the size they are told: a write beyond the cap is an overrun under ASan
static void host_entries()
{
  dabhip_fifo* f = dabhip_host_fifo_new();
  CHECK(f);
  std::vector<uint8_t> stream(2 * kTfBytes);
  for (size_t i = 0; i < stream.size(); ++i) stream[i] = static_cast<uint8_t>(i * 7);
  std::vector<int32_t> seg_end(kMaxSeg);
  std::vector<int64_t> seg_src(kMaxSeg);
  std::vector<uint8_t> tail(kTailBytes);
  int32_t nseg = 0, count = 0;
  int status = 0;
  for (int call = 0; call < 4 && status == 0; ++call)      // until the FIFO holds a frame
    status = dabhip_host_fifo_call(f, 0, -100, kChunkBytes, stream.data(), &nseg, seg_end.data(), seg_src.data(), &count, tail.data());
  CHECK(status > 0 && nseg >= 1 && nseg <= kMaxSeg);
  CHECK(dabhip_host_fifo_call(f, 0, 0, kChunkBytes + 2, nullptr, &nseg, seg_end.data(), seg_src.data(), nullptr, nullptr) == -1);
  CHECK(std::strstr(dabhip_last_error(), "chunk_bytes") != nullptr);      // error.cpp's text, as the library keeps it
  dabhip_host_fifo_free(f);
  // the control-plane replay with room for fewer frames than it produces: the count of all of them, only cap_frames written
  const int ntf = 20, cap = 5;
  std::vector<uint8_t> fibs, ok;
  make_fibs(0, 3, 40, ntf, fibs, ok);
  std::vector<int32_t> first_cif(cap), header_len(cap);
  std::vector<uint8_t> headers(static_cast<size_t>(cap) * kEtiHeaderMax);
  CHECK(dabhip_host_control_replay(fibs.data(), ok.data(), ntf, first_cif.data(), headers.data(), header_len.data(), cap) == 4 * (ntf - 13));
  for (int i = 0; i < cap; ++i) CHECK(header_len[i] > 0 && header_len[i] <= kEtiHeaderMax && first_cif[i] == 4 * 13 - 16 + i);
  std::vector<char> log(8);
  CHECK(dabhip_host_control_replay_log(log.data(), static_cast<int64_t>(log.size())) >= 0 && std::strlen(log.data()) < log.size());
  // the placement plan with fewer CPU entries than the lists name: CPUs beyond ncpu are not recorded
  const int32_t slice_node[3] = {0, 1, 0};
  const char* lists[2] = {"0-3", "4-7"};
  std::vector<int32_t> cpu_slice(6);
  CHECK(dabhip_host_placement_plan(slice_node, 3, lists, 2, cpu_slice.data(), static_cast<int>(cpu_slice.size())) == 3);
  CHECK(cpu_slice == (std::vector<int32_t>{0, 0, 2, 2, 1, 1}));
}
static void test_fifo()
{
  test_fifo_views();
  host_entries();
}

// A session's windows (session_windows.hpp) on the host: three byte arrays per stream stand in for the device windows, sized exactly as the session sizes
// them; a known byte stream is fed in random even segments with a random non-decreasing need_from; every feed applies the plan's copies with memcpy and
// then finds byte x of the stream at window + virtual_base + x for every x the front end may still read.
static void session_on_host(size_t reserve, unsigned seed, bool reached[6])
{
  std::mt19937 rng(seed);
  std::vector<uint8_t> stream(40 * reserve + 4096);
  for (uint8_t& v : stream) v = static_cast<uint8_t>(rng());
  std::vector<uint8_t> win[3];           // window k % 3 holds segment k; like DeviceBuffer: grow-only, contents lost on growth
  auto reserve_window = [](std::vector<uint8_t>& w, size_t n) { if (n > w.size()) w = std::vector<uint8_t>(n, 0xEE); };
  WindowBook book;
  int64_t need_from = 0;
  bool first = true, grown_last = false;
  for (uint64_t k = 0; static_cast<size_t>(book.avail) < stream.size(); ++k) {
    std::vector<uint8_t>& to = win[k % 3];
    const std::vector<uint8_t>& from = win[(k + 2) % 3];
    const size_t left = stream.size() - static_cast<size_t>(book.avail);
    size_t nbytes = rng() % 4 == 0 ? 0 : 2 * (rng() % (reserve / 2 + 3));      // empty segments too; up to a little more than the reserve
    nbytes = std::min(nbytes, left);
    // the session's upload: the segment behind the reserve
    reserve_window(to, window_bytes(reserve, nbytes));
    std::memcpy(to.data() + reserve, stream.data() + book.avail, nbytes);
    // the front end's answer: never backwards, now and then beyond what was fed; every fourth feed steered to one of the edges of the grow rule
    const int64_t held = book.avail - need_from;
    const int64_t edge[3] = {0, static_cast<int64_t>(reserve), static_cast<int64_t>(reserve) + 2};
    const int64_t want = edge[rng() % 3];
    if (!first && k % 4 == 0 && held >= want) need_from = book.avail - want;
    else if (!first && rng() % 3 == 0) need_from += static_cast<int64_t>(rng() % (reserve / 2)) & ~int64_t(1);
    const WindowPlan p = plan_window(book, first, need_from, nbytes, reserve);
    CHECK(!p.refused && p.need == window_need_from(first, need_from, book.avail) && p.need >= book.base && p.kept == static_cast<size_t>(book.avail - p.need));
    CHECK(p.grow == (p.kept > reserve));
    if (p.grow) {                         // the segment moves to a window of its own size
      std::vector<uint8_t> big(p.grow_bytes, 0xEE);
      std::memcpy(big.data() + p.at, to.data() + reserve, nbytes);
      to = std::move(big);
    }
    if (p.kept) std::memcpy(to.data() + p.move_to, from.data() + p.move_from, p.kept);      // (the session queues no move of nothing either)
    CHECK(p.book.base == p.need && p.book.avail == book.avail + static_cast<int64_t>(nbytes));
    for (int64_t x = p.need; x < p.book.avail; ++x) CHECK(to[static_cast<size_t>(p.virtual_base + x)] == stream[static_cast<size_t>(x)]);
    reached[0] |= first;
    reached[1] |= !first && p.kept == 0;
    reached[2] |= p.kept == reserve;
    reached[3] |= p.kept == reserve + 2;
    reached[4] |= grown_last;
    reached[5] |= need_from > book.avail;
    grown_last = p.grow;
    book = p.book;
    first = false;
  }
}
static void test_windows()
{
  for (size_t reserve : {size_t(256), size_t(65536)}) {
    bool reached[6] = {false, false, false, false, false, false};      // first feed, kept == 0, == reserve, == reserve + 2 (grows), a feed after a grow, need_from beyond avail
    for (unsigned seed = 1; seed <= 3; ++seed) session_on_host(reserve, seed, reached);
    for (bool r : reached) CHECK(r);
  }
  // the refusals: a history the gather's 32-bit sizes cannot carry; segments the gather forms leave to the copy commands
  WindowBook far;
  far.avail = int64_t(1) << 32;
  CHECK(plan_window(far, false, 0, 16, 256).refused != nullptr && plan_window(far, false, 2, 16, 256).refused == nullptr);
  CHECK(gather_fits((size_t(1) << 32) - 1) && !gather_fits(size_t(1) << 32));
  CHECK(window_bytes(256, 0) == 272 && window_bytes(256, 16) == 272 && window_bytes(256, 18) == 274);
}

// The dealing rule (placement.hpp: Deal): contiguous slices that cover [0, B), sizes that differ by at most one with the larger ones first, and the
// inverse that dabhip_multi_plan answers with before any decode
static void test_deal()
{
  for (int n = 1; n <= 9; ++n)
    for (int B = 1; B <= 40; ++B) {
      const Deal d{B, n};
      int next = 0;
      for (int i = 0; i < n; ++i) {
        CHECK(d.first(i) == next && d.count(i) >= 0);
        CHECK(d.count(i) == B / n || d.count(i) == B / n + 1);
        if (i) CHECK(d.count(i) <= d.count(i - 1));
        for (int b = d.first(i); b < d.first(i) + d.count(i); ++b) CHECK(d.slice_of(b) == i);
        next += d.count(i);
      }
      CHECK(next == B);
    }
  const Deal node{2048, 8}, small{10, 4};       // the examples of multi.cpp's header
  for (int i = 0; i < 8; ++i) CHECK(node.count(i) == 256 && node.first(i) == 256 * i);
  for (int s = 0; s < 2048; ++s) CHECK(node.slice_of(s) == s / 256);
  const int want[4] = {3, 3, 2, 2};
  for (int i = 0; i < 4; ++i) CHECK(small.count(i) == want[i]);
  CHECK(small.slice_of(5) == 1 && small.slice_of(6) == 2 && small.slice_of(9) == 3);
}

static void test_synth()
{
  for (int preset = 0; preset < 2; ++preset) {
    dabhip_synth_cfg cfg;
    CHECK(dabhip_synth_preset(preset, &cfg) == 0);
    cfg.seed = 5 + static_cast<uint64_t>(preset);
    cfg.skip_samples = preset ? 4321 : 0;
    cfg.snr_db = preset ? 9.0 : 1000.0;
    cfg.cfo_hz = preset ? 123.0 : 0.0;
    const size_t n = dabhip_synth_bytes(&cfg, 2);
    std::vector<uint8_t> iq(n + 64, 0xAA);
    CHECK(dabhip_synth_generate(&cfg, 2, iq.data(), n) == static_cast<int64_t>(n));
    for (size_t i = n; i < n + 64; ++i) CHECK(iq[i] == 0xAA);
    CHECK(dabhip_synth_generate(&cfg, 2, iq.data(), n - 1) < 0);                           // too small a buffer is refused
    std::vector<uint8_t> pay(4096);
    for (int k = 0; k < cfg.nsub; ++k) CHECK(dabhip_synth_payload(&cfg, 3, k, pay.data(), static_cast<int>(pay.size())) > 0);
  }
}

int main(int argc, char** argv)
{
  const char* only = argc > 1 ? argv[1] : "";
  struct { const char* name; void (*fn)(); } tests[] = {
      {"pool", test_pool_and_lane}, {"worklist", test_control_and_worklist}, {"fifo", test_fifo}, {"synth", test_synth},
      {"layout", test_layout}, {"carry", test_carry}, {"forms", test_forms}, {"scan", test_scan}, {"windows", test_windows}, {"deal", test_deal}};
  for (const auto& t : tests) {
    if (*only && std::strcmp(only, t.name) != 0) continue;
    t.fn();
    std::printf("ok %s\n", t.name);
  }
  return 0;
}
