// engine.cpp — host side of the batch engine: construction, decode_impl, sessions, ETI reads, trace (see engine.hpp for the pipeline).
#include "engine_detail.hpp"

#include <cmath>

#include "dab_bits.hpp"
#include "dab_tables.hpp"
#include "placement.hpp"
#include "../../include/dabhip.h"

namespace dabhip {

// The single-TF seams and stage entries carry the reference's hard 0/1 bytes (dab.h:27-33): their row strides are those of
// one bit per value.  With soft decisions on, the rows hold four bits per value, so these entry points refuse to run.
bool Engine::hard_only(const char* what)
{
  if (soft_bits_ == 0) return true;
  set_error(std::string(what) + ": not available with soft decisions on (dabhip_engine_set_soft): this entry point carries hard bits");
  return false;
}

bool Engine::check(hipError_t e, const char* what)
{
  if (e == hipSuccess) return true;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return false;
}
// event records and queries on the decode path: a record that fails would silently corrupt a stage time or -- ev_part0_, ev_chain_ -- an ordering
bool Engine::record(hipEvent_t e, hipStream_t s) { return check(hipEventRecord(e, s), "hipEventRecord"); }
bool Engine::elapsed(float* ms, hipEvent_t a, hipEvent_t b) { return check(hipEventElapsedTime(ms, a, b), "hipEventElapsedTime"); }

Engine::Engine(int device, int host_threads, std::vector<int> cpus) : device_(device), host_cpus_(std::move(cpus))
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device: libdabhip has no CPU fallback"); return; }
  if (device < 0 || device >= ndev) { set_error("device index out of range"); return; }
  if (!check(hipSetDevice(device), "hipSetDevice")) return;
  // The side stream carries the FIC decode (1008 short waves beside the OFDM stage's 16 k workgroups) and the small copies the host waits for:
  // it gets the highest priority, so that the FIBs -- and with them the host control plane -- are not queued behind the bulk of the OFDM stage
  // (DABHIP_SIDE_PRIORITY=0: equal priorities, as before round 3).
  int prio_low = 0, prio_high = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
  static const bool side_prio = !(std::getenv("DABHIP_SIDE_PRIORITY") && std::atoi(std::getenv("DABHIP_SIDE_PRIORITY")) == 0);
  if (!check(hipStreamCreate(&stream_), "hipStreamCreate") ||
      !check(side_prio ? hipStreamCreateWithPriority(&copy_stream_, hipStreamDefault, prio_high) : hipStreamCreate(&copy_stream_), "hipStreamCreate"))
    return;
  for (Event* e : {&ev_[0], &ev_[1], &ev_[2], &ev_[3], &ev_upload_, &ev_fic_, &ev_fic_done_, &ev_chain_, &ev_info_, &ev_fibs_, &ev_part0_, &ev_msc_[0], &ev_msc_[1],
                   &ev_msc_[2], &ev_msc_[3], &ev_h2d_[0], &ev_h2d_[1]})
    if (!check(e->create(), "hipEventCreate")) return;
  for (Event& e : stage_ev_)
    if (!check(e.create(false), "hipEventCreate")) return;
  if (!check(hipStreamCreateWithFlags(&d2h_stream_, hipStreamNonBlocking), "hipStreamCreate") || !check(ev_eti_fetch_[0].create(false), "hipEventCreate") ||
      !check(ev_eti_fetch_[1].create(false), "hipEventCreate"))
    return;

  std::vector<double2> tw2048(2048), tw1536(1536);
  std::vector<float2> twf(2048);
  for (int k = 0; k < 2048; ++k) {
    const double a = 2 * M_PI * k / 2048;
    tw2048[k] = make_double2(std::cos(a), std::sin(a));
    // the quarter points exactly (libm's cos(pi / 2) is 6.1e-17): bins 512 and 1536 of an int8 symbol are Gaussian integers, their differential products can
    // be EXACTLY zero (at low signal levels they are, every few thousand frames), and the fp64 re-decision of such a product must come out as the exact
    // integer arithmetic does -- as the sample-by-sample form happened to, and as any transform with trivial quarter turns (FFTW's codelets) does
    if (k % 512 == 0) tw2048[k] = make_double2(k == 0 ? 1.0 : k == 1024 ? -1.0 : 0.0, k == 512 ? 1.0 : k == 1536 ? -1.0 : 0.0);
    twf[k] = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(-std::sin(a)));   // forward kernel
  }
  for (int k = 0; k < 1536; ++k) tw1536[k] = make_double2(std::cos(2 * M_PI * k / 1536), std::sin(2 * M_PI * k / 1536));
  std::vector<uint8_t> prs(prs_quarter_turns().begin(), prs_quarter_turns().end());
  std::vector<uint16_t> qpsk(carrier_to_qpsk().begin(), carrier_to_qpsk().end());
  std::vector<uint16_t> crc(256);
  for (int v = 0; v < 256; ++v) {
    const uint8_t b = static_cast<uint8_t>(v);
    crc[v] = crc16_ccitt(&b, 1, 0);
  }
  // CRC shift operators: column b of operator i = CRC register after feeding 2^i zero bytes starting from 1 << b
  std::vector<uint16_t> crc_shift(14 * 16);
  for (int i = 0; i < 14; ++i)
    for (int bit = 0; bit < 16; ++bit) {
      if (i == 0) {
        const uint8_t zero = 0;
        crc_shift[bit] = crc16_ccitt(&zero, 1, static_cast<uint16_t>(1u << bit));
      } else {                               // square the previous operator
        uint16_t v = crc_shift[(i - 1) * 16 + bit], y = 0;
        for (int b = 0; b < 16; ++b)
          if ((v >> b) & 1) y ^= crc_shift[(i - 1) * 16 + b];
        crc_shift[i * 16 + bit] = y;
      }
    }
  // the descrambling words of the longest code word an ETI frame can hold (dab_tables.hpp: kMaxCodewordBytes; EEP 4-B at n = 57 is 5472 bytes per CIF),
  // and as many zero words for the S1 entry, which descrambles nothing
  std::vector<uint32_t> prbs(kMaxCodewordWords), zeros(kMaxCodewordWords, 0u);
  {
    Prbs g;
    for (auto& w : prbs) {
      uint32_t x = 0;
      for (int b = 0; b < 4; ++b) x |= static_cast<uint32_t>(g.next_byte()) << (8 * b);
      w = x;
    }
  }
  if (!d_tw2048_.upload(tw2048, stream_) || !d_tw1536_.upload(tw1536, stream_) || !d_twf_.upload(twf, stream_) ||
      !d_prs_.upload(prs, stream_) || !d_qpsk_.upload(qpsk, stream_) || !d_crc_tab_.upload(crc, stream_) || !d_crc_shift_.upload(crc_shift, stream_) ||
      !d_prbs_.upload(prbs, stream_) || !d_zero_words_.upload(zeros, stream_))
    return;
  if (!check(hipStreamSynchronize(stream_), "table upload")) return;
  // host threads for the per-stream control plane: half the CPUs this process may use (its affinity mask capped by the cgroup's CFS quota:
  // placement.hpp usable_cpus(); the machine's thread count says nothing in a container), at most 24, at least 2; DABHIP_HOST_THREADS overrides it
  // (bench.py gives each of N ranks on a node its share, so that 8 ranks do not start 8 full pools)
  const int hw = usable_cpus();
  int nthreads = host_threads > 0 ? std::min(host_threads, 64) : std::max(2, std::min(hw / 2, 24));
  if (const char* env = std::getenv("DABHIP_HOST_THREADS")) nthreads = std::max(1, std::min(64, std::atoi(env)));
  // host placement (placement.hpp): the device's NUMA node; without an explicit CPU list the host threads go to that node's CPUs when the machine
  // has more than one node with CPUs (on a single-socket box there is nothing to choose)
  {
    char bdf[32] = {0};
    if (numa_enabled() && hipDeviceGetPCIBusId(bdf, sizeof bdf, device) == hipSuccess) numa_node_ = numa_node_of_pci(bdf);
    else (void)hipGetLastError();
    if (host_cpus_.empty() && numa_enabled() && numa_node_ >= 0) {
      const std::vector<std::vector<int>> nodes = allowed_node_cpus();       // (a process pinned to one socket sees one populated node: nothing to choose)
      int populated = 0;
      for (const auto& n : nodes) populated += n.empty() ? 0 : 1;
      if (populated > 1 && numa_node_ < static_cast<int>(nodes.size())) host_cpus_ = nodes[static_cast<size_t>(numa_node_)];
    }
  }
  knobs_.from_env();
  pool_.reset(new ThreadPool(std::max(0, nthreads - 1), host_cpus_));
  host_lane_.reset(new AsyncLane(host_cpus_));
  ok_ = true;
}

bool Engine::set_decoder_forms(int msc_form, int fic_form)
{
  if (!msc_form_valid(msc_form) || !fic_form_valid(fic_form)) {
    set_error("set_decoder_forms: no such form (MSC " + std::to_string(msc_form) + ", FIC " + std::to_string(fic_form) +
              "; the FIC decoder has AUTO, WAVE, LANE and FOUR)");
    return false;
  }
  msc_form_ = msc_form;
  fic_form_ = fic_form;
  return true;
}

bool Engine::set_launch_limits(const int64_t* v)
{
  LaunchLimits l;
  const char* const wrong = v ? launch_limits_from(v, &l) : "null argument";
  if (wrong) {
    set_error(std::string("set_launch_limits: ") + wrong);
    return false;
  }
  limits_ = l;
  return true;
}

Engine::~Engine()
{
  if (d2h_stream_) { (void)hipStreamSynchronize(d2h_stream_); (void)hipStreamDestroy(d2h_stream_); }
  if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

bool Engine::read_eti(int64_t first, int64_t n, uint8_t* dst)
{
  if (n <= 0) return true;
  if (!check(hipSetDevice(device_), "hipSetDevice")) return false;   // callers may sit on another device's thread (dabhip_multi)
  // on the download stream and ended by a stream synchronise (hip_util.hpp: blocking_copy): callers read after every decode or segment, for ever
  return check(hipMemcpyAsync(dst, d_eti_.get() + first * kEtiBytes, static_cast<size_t>(n) * kEtiBytes, hipMemcpyDeviceToHost, d2h_stream_), "eti download") &&
         check(hipStreamSynchronize(d2h_stream_), "eti download");
}

// ---------------------------------------------------------------------------------------------
// Session carry-over: the FIC blocks, FIBs and CRC flags of each stream's last StreamCarry::keep TF slots and its logical CIF rows
// from 15 before the oldest kept CIF move from the previous segment's layout to the front of the stream's part of the new
// one (through a dense temporary: the buffers may be re-allocated in between).
bool Engine::carry_and_reserve(const SegmentLayout& seg)
{
  const int nslots = seg.tf_base.back(), nrows = seg.next_row + 1;
  const size_t bits = soft_bits_ ? 4 : 1;
  const size_t unit[4] = {kFicWords * 4 * bits, 384, 12, kCifWords * 4 * bits};
  HostList<CopyDesc>&out = carry_out_descs_, &in = carry_in_descs_;   // (the previous segment's lists were consumed before its feed returned)
  out.clear();
  in.clear();
  size_t tmp_bytes = 0;
  const int n = static_cast<int>(carry_.size());
  uint8_t* base[4] = {reinterpret_cast<uint8_t*>(d_fic_bits_.get()), d_fibs_.get(), d_fib_ok_.get(), reinterpret_cast<uint8_t*>(d_msc_bits_.get())};
  struct Piece { int which; size_t src, dst, bytes, tmp; };
  std::vector<Piece> pieces;
  for (int b = 0; b < n; ++b) {
    const StreamCarry& c = carry_[b];
    const int keep = c.keep;
    if (keep == 0) continue;
    const size_t src_slot = static_cast<size_t>(c.prev_tf_base) + c.prev_used - keep, dst_slot = seg.tf_base[b];
    for (int w = 0; w < 3; ++w) {
      pieces.push_back(Piece{w, src_slot * unit[w], dst_slot * unit[w], keep * unit[w], tmp_bytes});
      tmp_bytes += (keep * unit[w] + 15) & ~size_t(15);
    }
    const size_t src_row = static_cast<size_t>(c.prev_row_base) - kRowLead + 4 * (c.prev_used - keep), dst_row = static_cast<size_t>(seg.row_base[b]) - kRowLead;
    const size_t rows = 4 * static_cast<size_t>(keep) + kRowLead;
    pieces.push_back(Piece{3, src_row * unit[3], dst_row * unit[3], rows * unit[3], tmp_bytes});
    tmp_bytes += rows * unit[3];
  }
  if (!pieces.empty()) {
    if (!d_carry_.reserve(tmp_bytes)) return false;
    for (const Piece& p : pieces) out.push_back(CopyDesc{base[p.which] + p.src, d_carry_.get() + p.tmp, static_cast<uint32_t>(p.bytes)});
    // (the copy out must be over before a growing buffer is given back; when nothing grows -- every segment of a session but the first few --
    // stream order alone keeps the two copies apart, and the host does not wait)
    const bool grows = nslots > tf_slots_ || nrows > msc_rows_;
    if (!d_copy_descs_.upload(out, stream_) || !check(launch_batched_copy(d_copy_descs_.get(), static_cast<int>(out.size()), stream_), "carry out") ||
        (grows && !check(hipStreamSynchronize(stream_), "carry out")))
      return false;
  }
  if (!reserve_tf_slots(nslots, nrows)) return false;
  if (!pieces.empty()) {
    uint8_t* nbase[4] = {reinterpret_cast<uint8_t*>(d_fic_bits_.get()), d_fibs_.get(), d_fib_ok_.get(), reinterpret_cast<uint8_t*>(d_msc_bits_.get())};
    for (const Piece& p : pieces) in.push_back(CopyDesc{d_carry_.get() + p.tmp, nbase[p.which] + p.dst, static_cast<uint32_t>(p.bytes)});
    if (!d_copy_descs_.upload(in, stream_) || !check(launch_batched_copy(d_copy_descs_.get(), static_cast<int>(in.size()), stream_), "carry in"))
      return false;
  }
  return true;
}

int64_t Engine::decode(const uint8_t* const* iq, const size_t* nbytes, int nstreams, bool on_device)
{
  clear_forms_ran();
  return decode_impl(iq, nbytes, nstreams, on_device, false);
}

// Streaming continuation: iq[b] are DEVICE pointers positioned so that iq[b][x] is byte x of stream b counted from the
// start of the session (only the bytes stream_need_from(b) .. avail[b] have to be backed by memory); avail[b] = bytes
// of the stream received so far.  Decodes the calls that became complete since the previous segment; state carried:
// the front-end state (K1), the lock / CIF-ring state of the control plane, the FIC blocks and FIBs of the last 4 TFs
// and the partly filled logical CIF rows.  The ETI frames of all segments concatenated equal those of one decode().
int64_t Engine::feed(const uint8_t* const* iq, const size_t* avail, int nstreams, bool first_segment)
{
  return decode_impl(iq, avail, nstreams, true, !first_segment);
}

int64_t Engine::stream_need_from(int b) const
{
  if (b < 0 || b >= static_cast<int>(h_states_.size())) return 0;
  const StreamState& st = h_states_[b];
  int64_t need = st.consumed;
  for (int i = 0; i < st.view.nseg; ++i)
    if (st.view.seg_src[i] >= 0) need = std::min(need, st.view.seg_src[i] + (i ? st.view.seg_end[i - 1] : 0));
  return std::max<int64_t>(need, 0) & ~int64_t(1);
}

// session bookkeeping at the start of a decode (fresh) or of a further segment (cont)
bool Engine::begin_decode(int nstreams, bool cont)
{
  if (cont && (nstreams != nstreams_ || static_cast<int>(planes_.size()) != nstreams)) { set_error("feed: the number of streams changed within a session"); return false; }
  nstreams_ = nstreams;
  eti_base_.assign(nstreams, 0);
  eti_count_.assign(nstreams, 0);
  if (!cont || static_cast<int>(stream_status_.size()) != nstreams) stream_status_.assign(nstreams, 0);
  total_eti_ = 0;
  if (!cont) {
    planes_.resize(nstreams);                  // re-initialised by the control-plane pass itself (planes_fresh_): 0.2 ms that would otherwise delay K1
    planes_fresh_ = true;
    carry_.resize(nstreams);
    for (StreamCarry& c : carry_) c.reset();
  }
  return true;
}

void Engine::DecodeRun::mark(const char* what) const { host_mark("[host] %-18s %8.3f ms\n", what, wall0); }

// Stage A: everything between the layout and the FIC decode -- buffers for the layout, then the FIC symbols (0..3) of every TF
// through the OFDM stage.  K3 comes first so that the FIC is decoded, and the host control plane can run, while the bulk of the
// OFDM stage still occupies the GPU: a launch of 4 / 76 of the work, so that the FIBs reach the host 2 ms before the MSC
// symbols are through (with the first 19 symbols in this launch the host finished 0.4 ms AFTER the OFDM stage).  Two-kernel stage
// (set_fused(0)): a pre-pass over the same four symbols.
// A fresh decode runs stage A from the layout callback, i.e. queued right behind K1 while the host still waits for K1's last
// downloads (0.19 ms of idle GPU otherwise); if a stream is scanned again afterwards (rare), the layout and stage A simply run
// again for the new frame list.  A session's further segments run it after the scan: their carry-over copies must happen once.
bool Engine::stage_a(DecodeRun& run)
{
  const SegmentLayout& seg = seg_;
  const int ntf = seg.ntf, nslots = seg.tf_base[run.nstreams];
  if (ntf == 0) return true;
  if (!carry_and_reserve(seg)) return false;
  const bool guard = guard_active(), soft = soft_bits_ != 0;
  const bool energies = guard || soft;                    // the per-symbol sample energies: the guard's error bounds, the soft scale
  const int chunk = run.chunk = fused_ ? std::max(ntf, 1) : std::min(ntf, limits_.fft_chunk_tfs);   // only the spectra buffer of the two-kernel stage calls for chunks
  if (!fused_ && !d_spectra_.reserve(static_cast<size_t>(chunk) * kSymbolsPerTf * 2048)) return false;
  if (!h_fibs_.resize(static_cast<size_t>(nslots) * 384) || !h_fib_ok_.resize(static_cast<size_t>(nslots) * 12)) return false;
  if (!record(ev_[3], stream_)) return false;
  if (energies && !d_delta_.reserve(static_cast<size_t>(ntf) * kSymbolsPerTf)) return false;
  if (guard && guard_launches_ == 0 && !guard_counters_clear_ && !guard_reserve_counters(ntf)) return false;
  if (fused_) {
    for (int first = 0; first < ntf; first += chunk)
      if (!fused_parts(first, std::min(chunk, ntf - first), 1, 4, 1)) return false;      // the three FIC symbols (and symbol 0, their reference)
  } else {
    const Pieces cut{ntf, int64_t(chunk) * 19};                   // 4 of 76 symbols: 19 x as many TFs fit the spectra buffer
    for (int64_t p = 0; p < cut.count(); ++p) {
      const int first = static_cast<int>(cut.first(p)), n = static_cast<int>(cut.size(p));
      ++report_.fic_prepass;
      GuardArgs ga = soft ? soft_guard_args() : GuardArgs{};   // (hard decisions: a non-null delta switches the guard's listing on)
      if (guard && !guard_begin(n, &ga)) return false;
      if (energies && !check(launch_symbol_delta(frame_list(), first, n, 4, d_delta_.get(), kSymbolsPerTf, soft ? kSoftNormC : guard_c_of(guard_rule_level()), stream_), "symbol delta launch"))
        return false;
      if (!check(launch_fic_prepass(soft_bits_, frame_list(), first, n, d_spectra_.get(), ga, stream_), "fic pre-pass launch")) return false;
      if (guard && !guard_finish(true, first, n, 1, 4, false)) return false;
    }
  }
  return record(ev_part0_, stream_);
}

// The control plane of every stream over the segment's new FIBs (h_fibs_, h_fib_ok_), then the MSC decode's work lists, built and queued for upload on the
// side stream while the OFDM stage still runs on the main one.  Runs on the host lane; its outcome in run.host_ok / host_error.
void Engine::control_pass(DecodeRun& run)
{
  (void)hipSetDevice(device_);               // the current device is per thread
  const SegmentLayout& seg = seg_;
  const int nstreams = run.nstreams;
  const uint8_t *const fibs = h_fibs_.data(), *const ok = h_fib_ok_.data();
  const auto t0 = std::chrono::steady_clock::now();
  const bool fresh = planes_fresh_;
  pool_->parallel_for(nstreams, [&](int b) {
    if (fresh) {
      planes_[b] = ControlPlane();
      planes_[b].set_filter(subch_keep_);
    }
    stream_jobs_[b].reserve(static_cast<size_t>(4) * seg.nnew[b]);
    planes_[b].rebase(4 * (carry_[b].prev_used - carry_[b].keep));   // CIF numbering of this segment's layout
    for (int s = seg.tf_base[b] + carry_[b].keep; s < seg.tf_base[b + 1]; ++s)
      planes_[b].on_tf(s - seg.tf_base[b], fibs + static_cast<size_t>(s) * 384, ok + static_cast<size_t>(s) * 12, stream_jobs_[b]);
  });
  std::vector<const ControlPlane*> plane_ptrs(nstreams);
  std::vector<const JobList*> job_ptrs(nstreams);
  total_eti_ = 0;
  for (int b = 0; b < nstreams; ++b) {
    plane_ptrs[b] = &planes_[b];
    job_ptrs[b] = &stream_jobs_[b];
    eti_base_[b] = total_eti_;
    eti_count_[b] = static_cast<int64_t>(stream_jobs_[b].size());
    stream_status_[b] = planes_[b].fault();
    total_eti_ += eti_count_[b];
  }
  planes_fresh_ = false;
  times_.control = ms_since(t0);
  run.mark("control plane done");
  const auto t1 = std::chrono::steady_clock::now();
  run.host_ok = msc_prepare(job_ptrs, plane_ptrs, seg.row_base, seg.fib_base, work_);
  run.mark("work lists built");
  run.host_ok = run.host_ok && msc_upload(work_, copy_stream_) && check(hipEventRecord(ev_upload_, copy_stream_), "work list upload");
  run.mark("work lists queued");
  if (!run.host_ok) run.host_error = dabhip_last_error();
  times_.worklist = ms_since(t1);
}

// one decode / segment: K1 with the layout and stage A inside it, K3 beside the MSC symbols' OFDM launches, the control plane on the host lane behind
// the FIBs, K4 + K5 -- the pipeline of engine.hpp, awaited once
int64_t Engine::decode_impl(const uint8_t* const* iq, const size_t* nbytes, int nstreams, bool on_device, bool cont, bool full_scan)
{
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (nstreams <= 0) { set_error("decode: no streams"); return -1; }
  if (!check(hipSetDevice(device_), "hipSetDevice")) return -1;
  DecodeRun run{nbytes, nstreams, cont, std::chrono::steady_clock::now()};
  times_ = StageTimes{};
  fft_launches_ = fft_tfs_ = 0;
  fft_ms_ = 0;
  guard_new_count();
  guard_decisions_ = 0;
  guard_overflows_ = 0;
  report_ = LaunchReport{};
  last_.pending = false;                     // the scan overwrites the descriptors the deferred frames of the last decode would be completed from
  last_.deferred = 0;
  layout_ms_ = 0;
  if (!begin_decode(nstreams, cont)) return -1;
  tii_ms_ = 0;
  tii_ran_ = false;
  if (tii_ && !tii_begin(nstreams, cont)) return -1;
  const SegmentLayout& seg = seg_;          // filled by layout_frames, from inside the scan
  struct SideStreamGuard {                   // whatever was queued on the side stream is awaited before returning
    hipStream_t s;
    ~SideStreamGuard() { (void)hipStreamSynchronize(s); }
  } side_guard{copy_stream_};
  run.mark("begin_decode done");
  if (!scan_streams(iq, on_device, full_scan, run)) return -1;      // (a fresh decode: with the layout and stage A)
  run.mark("scan done");
  times_.setup = scan_setup_ms_;
  for (int b = 0; b < nstreams; ++b) carry_[b].calls_done = std::max(carry_[b].calls_done, static_cast<int>(nbytes[b] / kChunkBytes));
  if (cont && !stage_a(run)) return -1;
  const int ntf = seg.ntf, nslots = seg.tf_base[nstreams], chunk = run.chunk;
  if (ntf == 0) return 0;                   // nothing demodulated: the carried data stay as they are
  times_.frames = layout_ms_;
  const bool guard = guard_active();
  if (guard) guard_decisions_ += static_cast<int64_t>(ntf) * (kFicBits + kMscBits);
  // FIC decode kernels and the FIB download on the side stream: the rest of the OFDM stage is queued on the main stream right
  // away and shares the GPU with them, waiting neither for the download nor for the host
  if (!fic_decode_slots_async(0, nslots, h_fibs_.data(), h_fib_ok_.data(), copy_stream_)) return -1;      // carried slots are decoded again: their FIBs are read by K5

  // K2 + K2b over the MSC symbols of the frames that can be locked: [0, nmsc) of the list (ofdm_msc_part); the deferred ones stay as they are
  bool gpu_ok = true;
  const int nmsc = seg.nmsc, nchunks = (nmsc + chunk - 1) / chunk;
  while (gpu_ok && static_cast<int>(chunk_ev_.size()) < 3 * nchunks) {
    chunk_ev_.emplace_back();
    gpu_ok = check(chunk_ev_.back().create(), "hipEventCreate");
  }
  gpu_ok = gpu_ok && ofdm_msc_part(0, nmsc, chunk, 0);
  if (tii_) gpu_ok = gpu_ok && tii_launch();      // behind the OFDM stage's launches: it delays none of them
  run.mark("ofdm queued");
  if (!check(hipEventSynchronize(ev_fibs_), "fic decode")) return -1;
  run.mark("fibs on host");
  {
    float part0_ms = 0, fic_ms = 0;
    // (the FIC decode runs beside the OFDM stage since round 2: no longer a term of the step.  A failed query: the decode fails below, after the drain)
    if (!elapsed(&part0_ms, ev_[3], ev_part0_) || !elapsed(&fic_ms, ev_part0_, ev_fic_done_)) gpu_ok = false;
    times_.fic = fic_ms + (fused_ ? 0.0f : part0_ms);   // the pre-pass of the two-kernel stage is FIC work; the FIC symbols' launch of the fused kernel is OFDM work
    if (fused_) times_.fft += part0_ms;
  }

  // control plane + work lists on a host thread, hidden behind the MSC symbols' part of the OFDM stage
  // host work lists live in the engine: ~35 MB per step at the benchmark size, reused instead of re-allocated
  stream_jobs_.resize(nstreams);
  for (auto& v : stream_jobs_) v.clear();
  // (on the engine's persistent lane since round 3; a std::thread created and joined per decode measured the same on an idle host:
  // 4.41 M against 4.40 M ETI frames/s)
  host_lane_->post([&]() { control_pass(run); });

  // the host thread is done before the OFDM stage (at 4.5 of 5.8 ms into the step with 24 threads): K4 + K5 are queued right
  // behind it, and the whole pipeline is awaited ONCE
  host_lane_->wait();
  if (gpu_ok && run.host_ok)
    // (the upload is normally through long before this point: then no wait is queued at all -- a wait on an event that has already fired still costs the
    // main stream a barrier packet, 10 .. 15 us of idle GPU before K4)
    gpu_ok = (hipEventQuery(ev_upload_) == hipSuccess || check(hipStreamWaitEvent(stream_, ev_upload_, 0), "work list wait")) && msc_launch_async(work_);
  if (guard && gpu_ok) gpu_ok = guard_download();        // the entry counts of all guarded launches, behind everything else
  run.mark("all queued");
  const bool drained = check(hipStreamSynchronize(stream_), "decode");      // also on the error paths: nothing may stay in flight
  run.mark("stream drained");
  if (!gpu_ok || !drained) return -1;
  if (!run.host_ok) { set_error(run.host_error); return -1; }
  for (int c = 0; c < nchunks; ++c) {
    float a = 0, d = 0;
    if (!elapsed(&a, chunk_ev_[3 * c], chunk_ev_[3 * c + 1]) || !elapsed(&d, chunk_ev_[3 * c + 1], chunk_ev_[3 * c + 2])) return -1;
    times_.fft += a;
    times_.demap += d;
    fft_ms_ += a;
    fft_launches_ += 1;
    fft_tfs_ += std::min(chunk, nmsc - c * chunk);
  }
  msc_collect();
  if (tii_ran_ && !elapsed(&tii_ms_, ev_tii_[0], ev_tii_[1])) return -1;
  if (!on_device && times_.h2d_bytes > 0 && !elapsed(&times_.h2d, ev_h2d_[0], ev_h2d_[1])) return -1;
  if (guard && !guard_check()) return -1;
  // what the next segment of a session starts from
  for (int b = 0; b < nstreams; ++b) carry_[b].advance(seg, b);
  last_.chunk = chunk;
  last_.deferred = ntf - nmsc;
  last_.pending = last_.deferred > 0;
  times_.wall = ms_since(run.wall0);
  run.mark("return");
  return total_eti_;
}

int64_t Engine::eti_count(int stream) const { return (stream >= 0 && stream < nstreams_) ? eti_count_[stream] : -1; }
uint32_t Engine::stream_status(int stream) const { return (stream >= 0 && stream < static_cast<int>(stream_status_.size())) ? stream_status_[stream] : 0xffffffffu; }

int64_t Engine::eti_read(int stream, uint8_t* dst, int64_t cap_frames)
{
  if (stream < 0 || stream >= nstreams_) { set_error("eti_read: bad stream"); return -1; }
  const int64_t n = std::min(cap_frames, eti_count_[stream]);
  return read_eti(eti_base_[stream], n, dst) ? n : -1;
}

// Up to TWO fetches may be outstanding (the CLI's pipeline: its writer thread still waits for fetch k while the decode thread, through with decode
// k + 1, issues fetch k + 1 into the other output buffer): each has its own event, eti_fetch_wait() waits for the OLDEST one not yet waited for.  A
// third fetch without a wait is refused -- its destination would be a buffer somebody is still reading.  The copies run in order on one stream.
int64_t Engine::eti_fetch_async(uint8_t* dst, int64_t cap_frames)
{
  if (!dst) { set_error("eti_fetch: null destination"); return -1; }
  if (!check(hipSetDevice(device_), "hipSetDevice")) return -1;
  const uint64_t issued = eti_fetch_issued_.load(), waited = eti_fetch_waited_.load();
  if (issued - waited >= 2) { set_error("eti_fetch: two fetches are outstanding -- eti_fetch_wait first"); return -1; }
  const int64_t n = std::min(cap_frames, total_eti_);
  // (decode() has returned: the frames are complete; the copy is ordered before the next decode's K4 by the newest fetch event)
  if (n > 0 && !check(hipMemcpyAsync(dst, d_eti_.get(), static_cast<size_t>(n) * kEtiBytes, hipMemcpyDeviceToHost, d2h_stream_), "eti fetch")) return -1;
  if (!check(hipEventRecord(ev_eti_fetch_[issued & 1], d2h_stream_), "eti fetch event")) return -1;
  eti_fetch_issued_.store(issued + 1);
  return n;
}

bool Engine::eti_fetch_wait()
{
  const uint64_t waited = eti_fetch_waited_.load();
  if (waited == eti_fetch_issued_.load()) return true;
  bool ok = check(hipSetDevice(device_), "hipSetDevice") && check(hipEventSynchronize(ev_eti_fetch_[waited & 1]), "eti fetch");
  // the download stream is only ever waited for through these events: let the runtime drop its records of the finished fetches (engine.hpp:
  // blocking_copy) whenever that costs nothing -- no newer fetch queued -- and on every 32nd fetch of a pipeline that always has one in flight
  if (ok && reap_enabled() && (waited + 1 == eti_fetch_issued_.load() || waited % kReapEvery == kReapEvery - 1)) ok = check(hipStreamSynchronize(d2h_stream_), "eti fetch");
  eti_fetch_waited_.store(waited + 1);
  return ok;
}

const uint8_t* Engine::eti_device(int64_t* nframes) const
{
  if (nframes) *nframes = total_eti_;
  return d_eti_.get();
}

int Engine::trace(int stream, int32_t* ints6, double* ffs, int cap_calls) const
{
  if (stream < 0 || stream >= nstreams_ || h_descs_.size() < static_cast<size_t>(nstreams_) * scan_.max_calls) return -1;   // (a decode that failed before its scan)
  int n = 0;
  for (int k = 0; k < scan_.max_calls && n < cap_calls; ++k, ++n) {
    const CallDesc& d = h_descs_[static_cast<size_t>(stream) * scan_.max_calls + k];
    int32_t* o = ints6 + 6 * k;
    o[0] = d.status == 2; o[1] = d.status >= 1; o[2] = d.coarse_timeshift; o[3] = d.fine_timeshift;
    o[4] = d.coarse_freq_shift; o[5] = d.fifo_count;
    if (ffs) ffs[k] = d.fine_freq_shift;
  }
  return n;
}

int Engine::trace_nco(int stream, int32_t* nco_hz, int cap_calls) const
{
  if (stream < 0 || stream >= nstreams_ || !nco_hz || h_descs_.size() < static_cast<size_t>(nstreams_) * scan_.max_calls) return -1;
  int n = 0;
  for (int k = 0; k < scan_.max_calls && n < cap_calls; ++k, ++n) nco_hz[k] = h_descs_[static_cast<size_t>(stream) * scan_.max_calls + k].nco_hz;
  return n;
}

}  // namespace dabhip
