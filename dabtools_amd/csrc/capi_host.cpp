// capi_host.cpp — the entries of the C ABI (include/dabhip.h) that need no GPU: the host-side control plane, the constant tables, the parity guard's
// constants, K1's FIFO bookkeeping, the ingest stage's tap table and bookkeeping, the CPU budget and the placement plan -- what the CPU test-suite compares with the reference.  No HIP runtime call
// in here: tests/host_sanitize links this file as it is.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "capi_detail.hpp"
#include "control_plane.hpp"
#include "dab_tables.hpp"
#include "device_types.hpp"
#include "fifo_view.hpp"
#include "ingest_plan.hpp"
#include "placement.hpp"
#include "scan_blocks.hpp"

using namespace dabhip;

extern "C" {

// ---- what the host side may use, and where it would run (placement.hpp) -------------------------------
int dabhip_host_cpu_budget(int* affinity_cpus, int* cfs_quota_cpus)
{
  if (affinity_cpus) *affinity_cpus = static_cast<int>(dabhip::allowed_cpus().size());
  if (cfs_quota_cpus) *cfs_quota_cpus = dabhip::cfs_quota_cpus();
  return dabhip::usable_cpus();
}
int dabhip_host_placement_plan(const int32_t* slice_node, int nslices, const char* const* node_cpulist, int nnodes, int32_t* cpu_slice, int ncpu)
{
  if (!slice_node || !node_cpulist || !cpu_slice || nslices <= 0 || nnodes <= 0 || ncpu <= 0) { set_error("placement_plan: bad argument"); return -1; }
  std::vector<int> nodes(slice_node, slice_node + nslices);
  std::vector<std::vector<int>> node_cpus;
  for (int n = 0; n < nnodes; ++n) node_cpus.push_back(dabhip::parse_cpulist(node_cpulist[n] ? node_cpulist[n] : ""));
  const std::vector<std::vector<int>> plan = dabhip::plan_placement(nodes, node_cpus);
  for (int c = 0; c < ncpu; ++c) cpu_slice[c] = -1;
  int bound = 0;
  for (int i = 0; i < nslices; ++i) {
    bound += plan[static_cast<size_t>(i)].empty() ? 0 : 1;
    for (int c : plan[static_cast<size_t>(i)])
      if (c >= 0 && c < ncpu) cpu_slice[c] = i;       // (fewer CPUs than slices on a node: the later slice is the one recorded)
  }
  return bound;
}

// ---- the parity guard's constants and K1's per-stream state (device_types.hpp) ------------------------
int dabhip_parity_guard_default_level(void) { return dabhip::kDefaultGuardLevel; }
double dabhip_parity_guard_bin_scale(int raw_bin) { return (raw_bin >= 0 && raw_bin < 2048) ? static_cast<double>(dabhip::guard_bin_scale(raw_bin)) : -1.0; }
int dabhip_parity_guard_constants(int level, double* bin_c, double* prod_c)
{
  if (level < 1 || level > 2) return -1;
  if (bin_c) *bin_c = dabhip::guard_c_of(level);
  if (prod_c) *prod_c = dabhip::guard_prod_of(level);
  return 0;
}
int dabhip_host_stream_state_bytes(void) { return static_cast<int>(sizeof(StreamState)); }

}  // extern "C"

// ---- host-side control plane without a GPU -----------------------------------------------------------
namespace {
void sub_to_row(const SubChannel& s, int32_t* o)
{
  o[0] = s.id; o[1] = s.slform; o[2] = s.uep_index; o[3] = s.start_cu;
  o[4] = s.size_cu; o[5] = s.bitrate; o[6] = s.protlev; o[7] = s.ascty;
}
}  // namespace

extern "C" {

int dabhip_host_parse_fibs(const uint8_t* fibs, const uint8_t* crc_ok, int32_t* hdr3, int32_t* sub)
{
  if (!fibs || !crc_ok || !hdr3 || !sub) { set_error("host_parse_fibs: null argument"); return -1; }
  EnsembleInfo info;
  decode_fibs(info, fibs, crc_ok);
  hdr3[0] = info.eid; hdr3[1] = info.cif_hi; hdr3[2] = info.cif_lo;
  for (int i = 0; i < 64; ++i) sub_to_row(info.sub[i], sub + 8 * i);
  return 0;
}

int dabhip_host_lockin_deferred(int locked, int okcount, int ntf) { return lockin_deferred(locked != 0, okcount, ntf); }
int dabhip_host_eti_header(const int32_t* hdr3, const int32_t* sub, uint8_t* out, int cap)
{
  if (!hdr3 || !sub || !out || cap < kEtiHeaderMax) { set_error("host_eti_header: bad argument"); return -1; }
  EnsembleInfo info;
  info.eid = static_cast<uint16_t>(hdr3[0]);
  info.cif_hi = static_cast<uint8_t>(hdr3[1]);
  info.cif_lo = static_cast<uint8_t>(hdr3[2]);
  for (int i = 0; i < 64; ++i) {
    const int32_t* r = sub + 8 * i;
    SubChannel& s = info.sub[i];
    s.id = r[0]; s.slform = r[1]; s.uep_index = r[2]; s.start_cu = r[3];
    s.size_cu = r[4]; s.bitrate = r[5]; s.protlev = r[6]; s.ascty = r[7];
  }
  info.rescan();
  return build_eti_header(out, info);
}

// the operator messages (ControlPlane::take_log) of the calling thread's last dabhip_host_control_replay
static thread_local std::string g_replay_log;
int64_t dabhip_host_control_replay_log(char* buf, int64_t cap) { return hand_over_text(g_replay_log, buf, cap); }
int dabhip_host_control_replay(const uint8_t* fibs, const uint8_t* crc_ok, int ntf, int32_t* first_cif, uint8_t* headers,
                               int32_t* header_len, int cap_frames)
{
  if (!fibs || !crc_ok || !first_cif || !headers || !header_len) { set_error("host_control_replay: null argument"); return -1; }
  ControlPlane plane;
  JobList jobs;
  for (int t = 0; t < ntf; ++t) plane.on_tf(t, fibs + static_cast<size_t>(t) * 384, crc_ok + static_cast<size_t>(t) * 12, jobs);
  g_replay_log = plane.take_log();
  const int n = static_cast<int>(jobs.size());
  for (int i = 0; i < n && i < cap_frames; ++i) {
    first_cif[i] = jobs[i].first_cif;
    header_len[i] = jobs[i].header_len;
    std::memset(headers + static_cast<size_t>(i) * kEtiHeaderMax, 0, kEtiHeaderMax);
    std::memcpy(headers + static_cast<size_t>(i) * kEtiHeaderMax, jobs.header(jobs[i]), static_cast<size_t>(jobs[i].header_len));
  }
  return n;
}

}  // extern "C"

// ---- the product's constant tables (dab_tables.hpp), for the CPU test-suite to compare with the reference's arrays ----
extern "C" int dabhip_host_table(int which, int32_t* out, int cap)
{
  if (!out) { set_error("host_table: null argument"); return -1; }
  int n = 0;
  auto put = [&](int v) { if (n < cap) out[n] = v; ++n; };
  switch (which) {
    case 0:                                  // 64 rows {bitrate, size_cu, protlevel, L1..L4, PI1..PI4} (PI as in ETSI: 1..24, 0 = unused)
      for (int i = 0; i < 64; ++i) {
        const UepProfile& u = uep_table()[i];
        put(u.bitrate); put(u.size_cu); put(u.protlevel);
        for (int k = 0; k < 4; ++k) put(u.l[k]);
        for (int k = 0; k < 4; ++k) put(u.pi[k]);
      }
      break;
    case 1:                                  // puncturing vectors PI = 1..24 as 32 flags each
      for (int pi = 1; pi <= 24; ++pi)
        for (int b = 0; b < 32; ++b) put(static_cast<int>((puncture_mask(pi) >> b) & 1u));
      break;
    case 2:                                  // frequency de-interleaver: carrier -> QPSK symbol index
      for (uint16_t v : carrier_to_qpsk()) put(v);
      break;
    case 3:                                  // phase reference symbol, quarter turns per carrier
      for (uint8_t v : prs_quarter_turns()) put(v);
      break;
    default:
      set_error("host_table: unknown table");
      return -1;
  }
  if (n > cap) { set_error("host_table: buffer too small"); return -1; }
  return n;
}

// ---- FIFO / frame-buffer bookkeeping of K1 on the host (fifo_view.hpp), callable without a GPU ---------
struct dabhip_fifo {
  StreamState st;
  uint8_t tail[kTailBytes];          // the last kTailBytes of sdr->buffer, kept as bytes (device_types.hpp)
};
extern "C" dabhip_fifo* dabhip_host_fifo_new(void)
{
  dabhip_fifo* f = new (std::nothrow) dabhip_fifo;
  if (!f) return nullptr;
  std::memset(&f->st, 0, sizeof f->st);
  std::memset(f->tail, 0, sizeof f->tail);
  fifo_reset(f->st);
  return f;
}
extern "C" void dabhip_host_fifo_free(dabhip_fifo* f) { delete f; }
extern "C" int dabhip_host_fifo_call(dabhip_fifo* f, int32_t coarse_timeshift, int32_t fine_timeshift, int32_t chunk_bytes, const uint8_t* stream,
                                     int32_t* nseg, int32_t* seg_end, int64_t* seg_src, int32_t* fifo_count, uint8_t* tail)
{
  if (!f || !nseg || !seg_end || !seg_src) { set_error("host_fifo_call: null argument"); return -1; }
  if (chunk_bytes < 0 || chunk_bytes > kChunkBytes || (chunk_bytes & 1)) { set_error("host_fifo_call: chunk_bytes must be even, 0 .. 262144"); return -1; }
  f->st.coarse_timeshift = coarse_timeshift;
  f->st.fine_timeshift = fine_timeshift;
  const FifoCall c = fifo_call(f->st, chunk_bytes);
  if (f->st.overflow) { set_error("host_fifo_call: more than kMaxSeg nested short reads"); return -1; }
  if (c.status && stream)                                  // the rule K1 applies to its registers (sync_scan_kernel), byte by byte
    for (int p = kTailStart; p < kTfBytes; ++p) {
      const int64_t src = read_source(f->st.view, c.fresh, p);
      if (src >= 0) f->tail[p - kTailStart] = stream[src];
    }
  *nseg = f->st.view.nseg;
  for (int i = 0; i < kMaxSeg; ++i) { seg_end[i] = f->st.view.seg_end[i]; seg_src[i] = f->st.view.seg_src[i]; }
  if (fifo_count) *fifo_count = c.fifo_count;
  if (tail) std::memcpy(tail, f->tail, kTailBytes);
  return c.status ? (c.do_sync ? 2 : 1) : 0;
}

extern "C" int dabhip_host_fifo_skip_unshifted(dabhip_fifo* f, int32_t ncalls, int64_t* fed, int64_t* consumed)
{
  if (!f || ncalls < 0) { set_error("host_fifo_skip_unshifted: bad argument"); return -1; }
  if (f->st.coarse_timeshift + f->st.fine_timeshift != 0 || f->st.startup_delay <= 0) { set_error("host_fifo_skip_unshifted: a shift is pending or the first frame is still to be dropped"); return -1; }
  fifo_skip_unshifted(f->st.fed, f->st.consumed, ncalls);
  if (fed) *fed = f->st.fed;
  if (consumed) *consumed = f->st.consumed;
  return 0;
}

// ---- the ingest stage's host rule (ingest_plan.hpp): the tap table of a rate and the bookkeeping of a sequence of pushes ----
extern "C" int dabhip_ingest_taps(int format, int64_t rate_hz, int16_t* taps, int cap, int* L, int* M, int* T)
{
  if (format < 0 || format >= kIngestFormats) { set_error("ingest_taps: unknown format " + std::to_string(format) + " (0 = cu8, 1 = cs8, 2 = cs16, 3 = cf32)"); return -1; }
  IngestRatio r;
  const std::string why = ingest_ratio(rate_hz, &r);
  if (!why.empty()) { set_error("ingest_taps: " + why); return -1; }
  if (L) *L = r.L;
  if (M) *M = r.M;
  if (T) *T = r.T;
  const int n = r.L * r.T;
  if (r.bypass()) return 0;
  const std::vector<int16_t> t = ingest_design_taps(r, rate_hz);
  const std::string bad = ingest_check_taps(r, t.data());
  if (!bad.empty()) { set_error("ingest_taps: " + bad); return -1; }
  if (taps) {
    if (cap < n) { set_error("ingest_taps: buffer too small"); return -1; }
    std::memcpy(taps, t.data(), static_cast<size_t>(n) * sizeof(int16_t));
  }
  return n;
}

extern "C" int dabhip_ingest_plan(int64_t rate_hz, int auto_gain, const int64_t* push_samples, int npush, int64_t* nout, int64_t* carried)
{
  if (!push_samples || npush < 0 || !nout || !carried) { set_error("ingest_plan: bad argument"); return -1; }
  IngestRatio r;
  const std::string why = ingest_ratio(rate_hz, &r);
  if (!why.empty()) { set_error("ingest_plan: " + why); return -1; }
  IngestStreamState s;
  s.window_open = auto_gain != 0;
  for (int i = 0; i < npush; ++i) {
    if (push_samples[i] < 0) { set_error("ingest_plan: negative push"); return -1; }
    const IngestPush p = ingest_plan_push(r, s, push_samples[i]);
    nout[i] = p.nout;
    carried[i] = p.keep;
  }
  return 0;
}

extern "C" uint32_t dabhip_ingest_auto_gain(uint64_t energy) { return ingest_auto_gain(energy); }

// ---- the tuned mode's host rule: its table, the NCO table, the step of an offset and the bookkeeping ----
extern "C" int dabhip_ingest_tune_taps(int format, int64_t rate_hz, int16_t* taps, int cap, int* L, int* M, int* T)
{
  if (format < 0 || format >= kIngestFormats) { set_error("ingest_tune_taps: unknown format " + std::to_string(format) + " (0 = cu8, 1 = cs8, 2 = cs16, 3 = cf32)"); return -1; }
  IngestRatio r;
  const std::string why = ingest_tune_ratio(rate_hz, &r);
  if (!why.empty()) { set_error("ingest_tune_taps: " + why); return -1; }
  if (L) *L = r.L;
  if (M) *M = r.M;
  if (T) *T = r.T;
  const int n = r.L * r.T;
  if (n == 0) return 0;
  const std::vector<int16_t> t = ingest_tune_design_taps(r, rate_hz);
  const std::string bad = ingest_check_taps(r, t.data());
  if (!bad.empty()) { set_error("ingest_tune_taps: " + bad); return -1; }
  if (taps) {
    if (cap < n) { set_error("ingest_tune_taps: buffer too small"); return -1; }
    std::memcpy(taps, t.data(), static_cast<size_t>(n) * sizeof(int16_t));
  }
  return n;
}

extern "C" int dabhip_ingest_tune_nco(int16_t* cs, int cap)
{
  if (!cs || cap < kTuneNcoSize) { set_error("ingest_tune_nco: room for 4096 pairs is wanted"); return -1; }
  const std::vector<int16_t> t = ingest_tune_nco();
  std::memcpy(cs, t.data(), t.size() * sizeof(int16_t));
  return kTuneNcoSize;
}

extern "C" int dabhip_ingest_tune_step(int64_t rate_hz, int64_t offset_hz, uint32_t* step)
{
  if (!step) { set_error("ingest_tune_step: null argument"); return -1; }
  IngestRatio r;
  std::string why = ingest_tune_ratio(rate_hz, &r);
  if (why.empty()) why = ingest_tune_offset(rate_hz, offset_hz);
  if (!why.empty()) { set_error("ingest_tune_step: " + why); return -1; }
  *step = ingest_tune_step(rate_hz, offset_hz);
  return 0;
}

extern "C" int dabhip_ingest_tune_plan(int64_t rate_hz, int auto_gain, const int64_t* push_samples, int npush, int64_t* nout, int64_t* carried)
{
  if (!push_samples || npush < 0 || !nout || !carried) { set_error("ingest_tune_plan: bad argument"); return -1; }
  IngestRatio r;
  const std::string why = ingest_tune_ratio(rate_hz, &r);
  if (!why.empty()) { set_error("ingest_tune_plan: " + why); return -1; }
  IngestStreamState s;
  s.window_open = auto_gain != 0;
  for (int i = 0; i < npush; ++i) {
    if (push_samples[i] < 0) { set_error("ingest_tune_plan: negative push"); return -1; }
    const IngestPush p = ingest_tune_plan_push(r, s, push_samples[i]);
    nout[i] = p.nout;
    carried[i] = p.keep;
  }
  return 0;
}

// ---- the block scan's host rule (scan_blocks.hpp): from a spectrum to the blocks, and the bookkeeping of a sequence of pushes ----
extern "C" int dabhip_scan_detect(const uint64_t* P, int64_t rate_hz, int64_t center_hz, dabhip_scan_block* out, int cap)
{
  if (!P || (!out && cap > 0) || cap < 0) { set_error("scan_detect: bad argument"); return -1; }
  std::string why;
  const int n = scan_detect(P, rate_hz, center_hz, out, cap, &why);
  if (n < 0) set_error("scan_detect: " + why);
  return n;
}

extern "C" int dabhip_scan_plan(int nsegments, const int64_t* push_samples, int npush, int64_t* nseg, int64_t* carried)
{
  if (!push_samples || npush < 0 || !nseg || !carried) { set_error("scan_plan: bad argument"); return -1; }
  if (nsegments < 1 || nsegments > kScanMaxSegments) { set_error("scan_plan: nsegments must be 1 .. 65536"); return -1; }
  ScanStreamState s;
  for (int i = 0; i < npush; ++i) {
    if (push_samples[i] < 0) { set_error("scan_plan: negative push"); return -1; }
    const ScanPush p = scan_plan_push(nsegments, s, push_samples[i]);
    nseg[i] = p.nseg;
    carried[i] = p.keep;
  }
  return 0;
}
