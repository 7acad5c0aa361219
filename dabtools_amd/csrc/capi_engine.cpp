// capi_engine.cpp — the batch handle of the C ABI (include/dabhip.h: dabhip_engine_*), the stage entries and the decoder seam S1 (viterbi), all
// thin shims over Engine.  The other seams: capi_seams.cpp; sessions: session.cpp; several devices: multi.cpp.
#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "capi_detail.hpp"
#include "engine.hpp"

using namespace dabhip;

// One Engine, and what the handle itself answers for: which stream indices the last decode made valid (from the moment it started, also when it
// failed -- Engine's own bounds move with the stage entries too), its frames and its wall time.
struct dabhip_engine {
  Engine eng;
  int nstreams = 0;
  int64_t frames = 0;
  float wall_ms = 0;
  explicit dabhip_engine(int dev, int host_threads = 0, std::vector<int> cpus = {}) : eng(dev, host_threads, std::move(cpus)) {}
  bool has(int stream) const { return stream >= 0 && stream < nstreams; }
};

namespace {

Engine* default_engine()
{
  static std::mutex mu;
  static std::unique_ptr<Engine> eng;
  std::lock_guard<std::mutex> lock(mu);
  if (!eng) {
    std::unique_ptr<Engine> e(new Engine(0));
    if (!e->ok()) return nullptr;
    eng = std::move(e);
  }
  return eng.get();
}

dabhip_engine* checked(dabhip_engine* e)
{
  if (e && !e->eng.ok()) { delete e; return nullptr; }
  return e;
}

}  // namespace

extern "C" {

// ---- batch engine -----------------------------------------------------------------------------
dabhip_engine* dabhip_engine_create(int device) { return checked(new (std::nothrow) dabhip_engine(device)); }
dabhip_engine* dabhip_engine_create_ex(int device, int host_threads) { return checked(new (std::nothrow) dabhip_engine(device, host_threads)); }
dabhip_engine* dabhip_engine_create_on_cpus(int device, int host_threads, const int32_t* cpus, int ncpus)
{
  std::vector<int> list;
  for (int i = 0; cpus && i < ncpus; ++i) list.push_back(cpus[i]);
  return checked(new (std::nothrow) dabhip_engine(device, host_threads, list));
}
int dabhip_engine_host_cpus(const dabhip_engine* e, int32_t* cpus, int cap, int* numa_node)
{
  if (!e) return -1;
  const std::vector<int>& c = e->eng.host_cpus();
  if (numa_node) *numa_node = e->eng.numa_node();
  for (int i = 0; cpus && i < cap && i < static_cast<int>(c.size()); ++i) cpus[i] = c[static_cast<size_t>(i)];
  return static_cast<int>(c.size());
}
void dabhip_engine_destroy(dabhip_engine* e) { delete e; }

int64_t dabhip_engine_decode(dabhip_engine* e, const uint8_t* const* iq, const size_t* nbytes, int nstreams, int on_device)
{
  if (!e || !iq || !nbytes) { set_error("engine_decode: null argument"); return -1; }
  if (nstreams <= 0) { set_error("engine_decode: no streams"); return -1; }
  const auto t0 = std::chrono::steady_clock::now();
  e->eng.clear_forms_ran();
  e->nstreams = nstreams;
  e->frames = 0;
  const int64_t total = e->eng.decode(iq, nbytes, nstreams, on_device != 0);
  if (total < 0) return -1;
  e->frames = total;
  e->wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return total;
}
int64_t dabhip_engine_eti_count(const dabhip_engine* e, int stream) { return e && e->has(stream) ? e->eng.eti_count(stream) : -1; }
uint32_t dabhip_engine_stream_status(const dabhip_engine* e, int stream) { return e && e->has(stream) ? e->eng.stream_status(stream) : 0xffffffffu; }
int64_t dabhip_engine_eti_read(dabhip_engine* e, int stream, uint8_t* dst, int64_t cap_frames)
{
  if (!e || !dst) { set_error("eti_read: null argument"); return -1; }
  if (!e->has(stream)) { set_error("eti_read: bad stream"); return -1; }
  return e->eng.eti_read(stream, dst, cap_frames);
}
int64_t dabhip_engine_stream_log(dabhip_engine* e, int stream, char* buf, int64_t cap)
{
  if (!e || !e->has(stream)) return -1;
  return hand_over_text(e->eng.take_stream_log(stream), buf, cap);
}
int64_t dabhip_engine_eti_fetch(dabhip_engine* e, uint8_t* dst, int64_t cap_frames)
{
  if (!e || !dst) { set_error("eti_fetch: null argument"); return -1; }
  return e->eng.eti_fetch_async(dst, cap_frames);
}
int dabhip_engine_eti_fetch_wait(dabhip_engine* e)
{
  if (!e) { set_error("eti_fetch_wait: null handle"); return -1; }
  return e->eng.eti_fetch_wait() ? 0 : -1;
}
int64_t dabhip_engine_eti_drain(dabhip_engine* e, dabhip_eti_sink sink, void* user)
{
  if (!e || !sink) { set_error("eti_drain: null argument"); return -1; }
  return drain_eti(e->nstreams, sink, user, true, [e](int b) { return dabhip_engine_eti_count(e, b); },
                   [e](int b, uint8_t* dst, int64_t n) { return dabhip_engine_eti_read(e, b, dst, n); });
}
const void* dabhip_engine_eti_device_ptr(const dabhip_engine* e, int64_t* nframes)
{
  if (!e) return nullptr;
  if (nframes) *nframes = e->frames;
  return e->eng.eti_buffer();
}
int dabhip_engine_demapped_tf(dabhip_engine* e, int stream, int tf, int8_t* fic, int8_t* msc)
{
  if (!e || !fic || !msc) { set_error("demapped_tf: null argument"); return -1; }
  if (!e->has(stream)) { set_error("demapped_tf: bad stream"); return -1; }
  return e->eng.read_demapped_tf(stream, tf, fic, msc) ? 0 : -1;
}
int dabhip_engine_trace(const dabhip_engine* e, int stream, int32_t* ints6, double* ffs, int cap_calls)
{
  if (!e || !ints6 || !e->has(stream)) return -1;
  return e->eng.trace(stream, ints6, ffs, cap_calls);
}
int dabhip_engine_trace_nco(const dabhip_engine* e, int stream, int32_t* nco_hz, int cap_calls)
{
  if (!e || !e->has(stream)) return -1;
  return e->eng.trace_nco(stream, nco_hz, cap_calls);
}
int dabhip_engine_stage_ms(const dabhip_engine* e, const char** names, float* ms, int cap)
{
  if (!e) return -1;
  constexpr int kN = 17;
  static const char* kNames[kN] = {"sync", "fft", "demap", "fic", "control", "gather", "viterbi", "eti", "host_setup", "host_frames", "host_worklist", "wall",
                                   "h2d", "h2d_mbytes", "h2d_pinned_mbytes", "sync_fp64_calls", "sync_spec_calls"};
  const StageTimes& t = e->eng.stage_times();
  const float v[kN] = {t.sync, t.fft, t.demap, t.fic, t.control, t.gather, t.viterbi, t.eti, t.setup, t.frames, t.worklist, e->wall_ms,      // "wall": the handle's
                       t.h2d, static_cast<float>(t.h2d_bytes * 1e-6), static_cast<float>(t.h2d_pinned_bytes * 1e-6), t.sync_fp64_calls, t.sync_spec_calls};
  int n = 0;
  for (; n < kN && n < cap; ++n) {
    if (names) names[n] = kNames[n];
    if (ms) ms[n] = v[n];
  }
  return n;
}
int dabhip_engine_set_afc(dabhip_engine* e, int enable) { if (!e) return -1; e->eng.set_afc(enable != 0); return 0; }
int dabhip_engine_set_soft(dabhip_engine* e, int enable) { if (!e) return -1; e->eng.set_soft(enable != 0); return 0; }
int dabhip_engine_set_decoder_forms(dabhip_engine* e, int msc_form, int fic_form)
{
  if (!e) { set_error("set_decoder_forms: null handle"); return -1; }
  return e->eng.set_decoder_forms(msc_form, fic_form) ? 0 : -1;
}
int dabhip_engine_set_soft_lanes(dabhip_engine* e, int enable)
{
  if (!e) { set_error("set_soft_lanes: null handle"); return -1; }
  e->eng.set_soft_lanes(enable != 0);
  return 0;
}
int dabhip_engine_decoder_forms(const dabhip_engine* e, uint32_t* msc_mask, uint32_t* fic_mask)
{
  if (!e) { set_error("decoder_forms: null handle"); return -1; }
  if (msc_mask) *msc_mask = e->eng.msc_forms_ran();
  if (fic_mask) *fic_mask = e->eng.fic_forms_ran();
  return 0;
}
int dabhip_engine_set_subchannels(dabhip_engine* e, const int32_t* ids, int n) { if (!e) return -1; e->eng.set_subchannel_filter(subchannel_mask(ids, n)); return 0; }
int dabhip_engine_set_parity_guard(dabhip_engine* e, int level) { if (!e) return -1; e->eng.set_parity_guard(level); return 0; }
int dabhip_engine_parity_guard_level(const dabhip_engine* e) { return e ? e->eng.parity_guard_level() : -1; }
int dabhip_engine_guard_stats(const dabhip_engine* e, int64_t* flagged, int64_t* decisions)
{
  if (!e) return -1;
  e->eng.guard_stats(flagged, decisions);
  return 0;
}
int dabhip_engine_guard_overflows(const dabhip_engine* e) { return e ? e->eng.guard_overflows() : -1; }
int dabhip_engine_set_guard_list_cap(dabhip_engine* e, uint32_t cap) { if (!e) return -1; e->eng.set_guard_list_cap(cap); return 0; }
int dabhip_engine_set_launch_limits(dabhip_engine* e, const int64_t* limits, int n)
{
  if (!e || !limits || n != kLaunchLimitCount) { set_error("set_launch_limits: bad argument"); return -1; }
  return e->eng.set_launch_limits(limits) ? 0 : -1;
}
int dabhip_engine_launch_report(const dabhip_engine* e, int64_t* out, int cap)
{
  if (!e || !out || cap < 0) { set_error("launch_report: bad argument"); return -1; }
  return report_to_words(e->eng.launch_report(), out, cap);
}
int dabhip_engine_msc_plan(const dabhip_engine* e, int32_t* nsteps, int cap, int64_t* ntiles)
{
  if (!e || cap < 0) { set_error("msc_plan: bad argument"); return -1; }
  return e->eng.msc_plan(nsteps, cap, ntiles);
}
int dabhip_engine_set_fused(dabhip_engine* e, int enable) { if (!e) return -1; e->eng.set_fused(enable != 0); return 0; }
int dabhip_engine_set_demod_all(dabhip_engine* e, int on) { if (!e) return -1; e->eng.set_demod_all(on != 0); return 0; }
int dabhip_engine_msc_deferred(const dabhip_engine* e) { return e ? e->eng.msc_deferred() : -1; }
int dabhip_engine_set_sync_speculation(dabhip_engine* e, int mode) { if (!e) return -1; e->eng.set_sync_speculation(mode); return 0; }
int dabhip_engine_fft_stats(const dabhip_engine* e, int64_t* launches, int64_t* tfs, double* ms)
{
  if (!e) return -1;
  e->eng.fft_stats(launches, tfs, ms);
  return 0;
}
int dabhip_engine_fft_roofline(dabhip_engine* e, int reps, int64_t* launches, int64_t* tfs, double* ms)
{
  if (!e) { set_error("fft_roofline: null handle"); return -1; }
  return e->eng.fft_roofline(reps, launches, tfs, ms) != 0 ? -1 : 0;
}

// ---- transmitter identification (tii.cpp) ---------------------------------------------------------
int dabhip_engine_set_tii(dabhip_engine* e, int enable) { if (!e) return -1; e->eng.set_tii(enable != 0); return 0; }
int dabhip_engine_tii_sums(dabhip_engine* e, int stream, uint64_t* T, int* frames)
{
  if (!e || !e->has(stream)) { set_error("tii_sums: bad argument"); return -1; }
  return e->eng.tii_sums(stream, T, frames) ? 0 : -1;
}
int dabhip_engine_tii(dabhip_engine* e, int stream, dabhip_tii_id* out, int cap)
{
  uint64_t T[DABHIP_TII_SUMS];
  if (cap < 0 || (!out && cap > 0)) { set_error("tii: bad argument"); return -1; }
  if (dabhip_engine_tii_sums(e, stream, T, nullptr) != 0) return -1;
  return dabhip_tii_detect(T, out, cap);
}
int dabhip_engine_tii_ms(const dabhip_engine* e, float* ms)
{
  if (!e || !ms) { set_error("tii_ms: null argument"); return -1; }
  *ms = e->eng.tii_ms();
  return 0;
}

// ---- stage entries ----------------------------------------------------------------------------
int dabhip_stage_tii(dabhip_engine* e, const uint8_t* frames, int nframes, const int32_t* w0, const uint32_t* step, int on_device, uint64_t* T)
{
  if (!e || !frames || !w0 || !step || !T) { set_error("stage_tii: null argument"); return -1; }
  return e->eng.stage_tii(frames, nframes, w0, step, on_device != 0, T);
}
int dabhip_stage_ofdm_fft(dabhip_engine* e, const uint8_t* frames, int nframes, float* spectra, int on_device, int reps, float* kernel_ms)
{
  if (!e || !frames) { set_error("stage_ofdm_fft: null argument"); return -1; }
  return e->eng.stage_ofdm_fft(frames, nframes, spectra, on_device != 0, reps, kernel_ms);
}
int dabhip_stage_demap(dabhip_engine* e, const float* spectra, int nframes, uint8_t* fic, uint8_t* msc)
{
  if (!e || !spectra || !fic || !msc) { set_error("stage_demap: null argument"); return -1; }
  return e->eng.stage_demap(spectra, nframes, fic, msc);
}
int dabhip_stage_decision_audit(dabhip_engine* e, const uint8_t* frames, int nframes, int on_device, int guard_on, double* out8)
{
  if (!e || !frames || !out8) { set_error("stage_decision_audit: null argument"); return -1; }
  return e->eng.stage_decision_audit(frames, nframes, on_device != 0, guard_on != 0, out8);
}
int dabhip_stage_decision_audit_fused(dabhip_engine* e, const uint8_t* frames, int nframes, int on_device, int guard_on, double* out10)
{
  if (!e || !frames || !out10) { set_error("stage_decision_audit_fused: null argument"); return -1; }
  return e->eng.stage_decision_audit(frames, nframes, on_device != 0, guard_on != 0, out10, true, out10 + 8);
}
int dabhip_stage_fic_decode(dabhip_engine* e, const uint8_t* fic, int nframes, uint8_t* fibs, uint8_t* crc_ok)
{
  if (!e || !fic || !fibs || !crc_ok) { set_error("stage_fic_decode: null argument"); return -1; }
  e->eng.clear_forms_ran();
  return e->eng.stage_fic_decode(fic, nframes, fibs, crc_ok);
}

// ---- S1: decoder seam ---------------------------------------------------------------------------
void* dabhip_create_viterbi(int /*len*/) { return default_engine(); }
int dabhip_init_viterbi(void) { return default_engine() ? 0 : -1; }

int dabhip_viterbi_batch(void* p, const unsigned char* symbols, unsigned char* data, int framebits, int n)
{
  Engine* eng = p ? static_cast<Engine*>(p) : default_engine();
  if (!eng) return -1;
  if (!symbols || !data) { set_error("viterbi: null argument"); return -1; }
  return eng->viterbi_batch(symbols, data, framebits, n);
}
void dabhip_viterbi(void* p, unsigned char* symbols, unsigned char* data, int framebits)
{
  (void)dabhip_viterbi_batch(p, symbols, data, framebits, 1);   // like the reference: no error return
}

}  // extern "C"
