// engine_stage.cpp — stage entries, audits and the single-call seams (see engine.hpp for the pipeline).
#include "engine_detail.hpp"

namespace dabhip {

namespace {
// n transmission frames that lie back to back in one stream, from its frame `first` on, as calls 0 .. n - 1 (Engine::set_frame_list)
std::vector<CallDesc> contiguous_descs(int first, int n)
{
  std::vector<CallDesc> descs(static_cast<size_t>(n));
  for (int j = 0; j < n; ++j) {
    std::memset(&descs[j], 0, sizeof(CallDesc));
    descs[j].status = 2;
    descs[j].ordinal = j;
    descs[j].view = initial_state().view;
    descs[j].view.seg_src[0] = static_cast<int64_t>(first + j) * kTfBytes;
  }
  return descs;
}
// decision_audit_kernel's result (k_parity.hip) -> out8 of the stage entries; listed: entries the demappers listed
struct AuditOut { unsigned long long decisions, disagree, outside, flagged; unsigned bin_bits, dec_bits, prod_bits, pad; };
bool read_audit(const uint8_t* d_out, uint64_t listed, double* out8)
{
  AuditOut h;
  if (blocking_copy(&h, d_out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return false;
  auto f = [](unsigned bits) { float v; std::memcpy(&v, &bits, 4); return static_cast<double>(v); };
  out8[0] = static_cast<double>(h.decisions); out8[1] = static_cast<double>(h.disagree); out8[2] = static_cast<double>(h.outside);
  out8[3] = static_cast<double>(h.flagged); out8[4] = f(h.bin_bits); out8[5] = f(h.dec_bits); out8[6] = f(h.prod_bits); out8[7] = static_cast<double>(listed);
  return true;
}
void pack_bits(const uint8_t* bytes, int nbits, uint32_t* words)
{
  std::memset(words, 0, static_cast<size_t>(nbits / 32) * 4);
  for (int i = 0; i < nbits; ++i) words[i >> 5] |= static_cast<uint32_t>(bytes[i] & 1u) << (i & 31);
}
}  // namespace

// K2 (ofdm_fft_kernel) alone over the frames of the last decode: the same IQ, the same frame list and the same launch
// shape (chunks of LaunchLimits::fft_chunk_tfs) as the two-kernel OFDM stage, whatever stage the decode itself used.  This is the
// HBM-roofline measurement of SURVEY.md 8(d): 311,296 B read + 1,245,184 B written per TF.
int Engine::fft_roofline(int reps, int64_t* launches, int64_t* tfs, double* ms)
{
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (seg_.ntf <= 0) { set_error("fft_roofline: no decode to measure on"); return -1; }
  if (!check(hipSetDevice(device_), "hipSetDevice")) return -1;
  const int ntf = seg_.ntf, chunk = std::min(ntf, limits_.fft_chunk_tfs);      // (the launch report stays that of the decode: this entry returns its own count)
  if (!d_spectra_.reserve(static_cast<size_t>(chunk) * kSymbolsPerTf * 2048)) return -1;
  reps = std::max(reps, 1);
  int64_t nl = 0, nt = 0;
  double total = 0;
  for (int r = -1; r < reps; ++r) {                      // r = -1: untimed
    const Pieces cut{ntf, chunk};
    for (int64_t p = 0; p < cut.count(); ++p) {
      const int first = static_cast<int>(cut.first(p)), n = static_cast<int>(cut.size(p));
      if (!record(ev_[0], stream_)) return -1;
      if (!check(launch_ofdm_fft(frame_list(), first, n, d_spectra_.get(), stream_), "fft launch")) return -1;
      if (!record(ev_[1], stream_)) return -1;
      if (!check(hipEventSynchronize(ev_[1]), "fft")) return -1;
      float t = 0;
      if (!elapsed(&t, ev_[0], ev_[1])) return -1;
      if (r >= 0) { total += t; ++nl; nt += n; }
    }
  }
  if (launches) *launches = nl;
  if (tfs) *tfs = nt;
  if (ms) *ms = total;
  return 0;
}

void Engine::fft_stats(int64_t* launches, int64_t* tfs, double* ms) const
{
  if (launches) *launches = fft_launches_;
  if (tfs) *tfs = fft_tfs_;
  if (ms) *ms = fft_ms_;
}

// ---------------------------------------------------------------------------------------------
int Engine::stage_ofdm_fft(const uint8_t* frames, int nframes, float* spectra, bool on_device, int reps, float* kernel_ms)
{
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (nframes <= 0) return 0;
  const uint8_t* const d_in = frames_on_device(frames, nframes, on_device);
  const std::vector<CallDesc> descs = contiguous_descs(0, nframes);
  const size_t nspec = static_cast<size_t>(nframes) * kSymbolsPerTf * 2048;
  if (!d_in || !set_frame_list(d_in, descs.data(), nframes, 0, false) || !d_spectra_.reserve(nspec)) return -1;
  reps = std::max(reps, 1);
  const FrameListArgs fl = frame_list();
  // one untimed launch first when timing
  if (reps > 1 && !check(launch_ofdm_fft(fl, 0, nframes, d_spectra_.get(), stream_), "fft launch")) return -1;
  if (!record(ev_[0], stream_)) return -1;
  for (int r = 0; r < reps; ++r)
    if (!check(launch_ofdm_fft(fl, 0, nframes, d_spectra_.get(), stream_), "fft launch")) return -1;
  if (!record(ev_[1], stream_)) return -1;
  if (!check(hipEventSynchronize(ev_[1]), "fft")) return -1;
  float ms = 0;
  if (!elapsed(&ms, ev_[0], ev_[1])) return -1;
  if (kernel_ms) *kernel_ms = ms / reps;
  if (spectra && !check(blocking_copy(spectra, d_spectra_.get(), nspec * sizeof(float2), hipMemcpyDeviceToHost), "spectra download")) return -1;
  return nframes;
}

int Engine::stage_demap(const float* spectra, int nframes, uint8_t* fic, uint8_t* msc)
{
  if (!hard_only("stage_demap")) return -1;
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (nframes <= 0) return 0;
  const size_t nspec = static_cast<size_t>(nframes) * kSymbolsPerTf * 2048;
  if (!set_frame_list(nullptr, nullptr, nframes, 0, true) || !d_spectra_.reserve(nspec)) return -1;
  if (!check(hipMemcpyAsync(d_spectra_.get(), spectra, nspec * sizeof(float2), hipMemcpyHostToDevice, stream_), "spectra upload")) return -1;
  // spectra only: no samples to re-decide from, so this stage entry returns the raw fp32 decisions (no parity guard)
  if (!check(launch_demap(false, 0, d_spectra_.get(), 0, nframes, d_frame_slot_.get(), d_frame_cif_row_.get(), d_qpsk_.get(), d_fic_bits_.get(), d_msc_bits_.get(), GuardArgs{}, stream_), "demap launch") ||
      !check(hipStreamSynchronize(stream_), "demap"))
    return -1;
  for (int j = 0; j < nframes; ++j)
    if (!unpack_tf_slot(j, fic + static_cast<size_t>(j) * kFicBits, msc + static_cast<size_t>(j) * kMscBits)) return -1;
  return nframes;
}

int Engine::stage_fic_decode(const uint8_t* fic, int nframes, uint8_t* fibs, uint8_t* crc_ok)
{
  clear_forms_ran();
  report_ = LaunchReport{};
  if (!hard_only("stage_fic_decode")) return -1;
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (nframes <= 0) return 0;
  if (!reserve_tf_slots(nframes)) return -1;
  std::vector<uint32_t> words(static_cast<size_t>(nframes) * kFicWords);
  for (int j = 0; j < nframes; ++j) pack_bits(fic + static_cast<size_t>(j) * kFicBits, kFicBits, words.data() + static_cast<size_t>(j) * kFicWords);
  if (!check(blocking_copy(d_fic_bits_.get(), words.data(), words.size() * 4, hipMemcpyHostToDevice), "fic upload")) return -1;
  return fic_decode_slots(0, nframes, fibs, crc_ok) ? nframes : -1;
}

// Decision audit (calibration / test tool of the parity guard): nframes contiguous cu8 frames through K2 + K2b (natural
// layout), optionally with the guard, then decision_audit_kernel's fp64 transforms against the result.
// out8 = {decisions, disagreements with fp64, disagreements on carriers the guard rule does NOT flag, decisions the rule flags,
//         max |X32 - X64| / sqrt(symbol energy), max product error / (|cur|_1 s(l-1) + |prev|_1 s(l)), max residual product
//         error / (|cur|_1 |prev|_1), entries the demapper listed (guard on)}
// fused = true (round 5): the same audit of the kernel the DEFAULT decode runs -- ofdm_demap_kernel's guarded build, through its audit build (the same source
// lines plus stores of its bins and products; k_fused.hip) -- with the frames laid out as a decode lays them out (FIC slot j, logical CIF rows from kRowLead +
// 4 j).  out8[7] = entries that kernel listed.  out_extra (2 values, may be null): {1 when the SHIPPING build (launch_ofdm_demap_fused_guarded) run on the
// same frames leaves exactly the bits the audit build left, before any re-decision; 1 when it lists the same number of decisions}.
int Engine::stage_decision_audit(const uint8_t* frames, int nframes, bool on_device, bool guard_on, double* out8, bool fused, double* out_extra)
{
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (!hard_only("stage_decision_audit")) return -1;
  if (nframes <= 0 || !out8) return 0;
  if (fused) return stage_decision_audit_fused(frames, nframes, on_device, guard_on, out8, out_extra);
  DeviceBuffer<uint8_t> d_out;
  if (!d_out.reserve(sizeof(AuditOut)) || !check(hipMemsetAsync(d_out.get(), 0, sizeof(AuditOut), stream_), "audit memset")) return -1;
  const int chunk = std::min(256, limits_.fft_chunk_tfs);      // (its own spectra buffer: never more than the decode's chunk)
  uint64_t listed = 0;
  const uint8_t* const d_in = frames_on_device(frames, nframes, on_device);
  if (!d_in) return -1;
  report_ = LaunchReport{};
  const Pieces cut{nframes, chunk};
  for (int64_t p = 0; p < cut.count(); ++p) {
    const int first = static_cast<int>(cut.first(p)), n = static_cast<int>(cut.size(p));
    ++report_.ofdm_chunks;
    const std::vector<CallDesc> descs = contiguous_descs(first, n);
    if (!set_frame_list(d_in, descs.data(), n, 0, true) || !d_spectra_.reserve(static_cast<size_t>(n) * kSymbolsPerTf * 2048)) return -1;
    GuardArgs ga{};
    guard_new_count();
    if (guard_on && (!d_delta_.reserve(static_cast<size_t>(n) * kSymbolsPerTf) || !guard_begin(n, &ga) ||
                     !check(launch_symbol_delta(frame_list(), 0, n, kSymbolsPerTf, d_delta_.get(), kSymbolsPerTf, guard_c_of(guard_rule_level()), stream_), "symbol delta launch")))
      return -1;
    if (!check(launch_ofdm_fft(frame_list(), 0, n, d_spectra_.get(), stream_), "fft launch") ||
        !check(launch_demap(false, 0, d_spectra_.get(), 0, n, d_frame_slot_.get(), d_frame_cif_row_.get(), d_qpsk_.get(), d_fic_bits_.get(), d_msc_bits_.get(), ga, stream_), "demap launch") ||
        (guard_on && !guard_finish(false, 0, n, 1, kSymbolsPerTf, false)) ||
        !check(launch_decision_audit(d_in + static_cast<size_t>(first) * kTfBytes, n, d_spectra_.get(), d_fic_bits_.get(), d_msc_bits_.get(), d_tw2048_.get(), d_qpsk_.get(), d_out.get(), stream_, nullptr, 0, guard_rule_level()), "audit launch") ||
        (guard_on && !guard_download()) || !check(hipStreamSynchronize(stream_), "audit") || (guard_on && !guard_check()))
      return -1;
    listed += static_cast<uint64_t>(guard_flagged_);
  }
  if (!read_audit(d_out.get(), listed, out8)) { set_error("audit download failed"); return -1; }
  return nframes;
}

int Engine::stage_decision_audit_fused(const uint8_t* frames, int nframes, bool on_device, bool guard_on, double* out8, double* out_extra)
{
  DeviceBuffer<uint8_t> d_out;
  DeviceBuffer<float2> d_bins, d_prod;
  if (!d_out.reserve(sizeof(AuditOut)) || !check(hipMemsetAsync(d_out.get(), 0, sizeof(AuditOut), stream_), "audit memset")) return -1;
  const int chunk = 128;
  uint64_t listed = 0;
  bool bits_equal = true, list_equal = true;
  const uint8_t* const d_in = frames_on_device(frames, nframes, on_device);
  if (!d_in) return -1;
  const size_t per_frame = static_cast<size_t>(kSymbolsPerTf) * 2048;
  if (!d_bins.reserve(per_frame * chunk) || !d_prod.reserve(per_frame * chunk)) return -1;
  std::vector<uint32_t> bits_a, bits_b;
  for (int first = 0; first < nframes; first += chunk) {
    const int n = std::min(chunk, nframes - first);
    const std::vector<CallDesc> descs = contiguous_descs(first, n);
    // (rows from kRowLead: where a decode puts the frame's first CIF -- the scatter reaches kRowLead rows back)
    if (!set_frame_list(d_in, descs.data(), n, kRowLead, true) || !d_delta_.reserve(static_cast<size_t>(n) * kSymbolsPerTf)) return -1;
    const size_t fic_words = static_cast<size_t>(n) * kFicWords, msc_words = static_cast<size_t>(4 * n + kRowLead + 1) * kCifWords;
    // two passes: the shipping build first (its raw bits and its list count kept), then the audit build, whose output the audit kernel reads
    uint32_t counts[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
      GuardArgs ga{};
      guard_new_count();
      if (!check(hipMemsetAsync(d_msc_bits_.get(), 0, msc_words * 4, stream_), "row clear")) return -1;     // (the rows before the first frame's are never written)
      for (int part = 0; part < 2; ++part) {              // the decode's own two launches: FIC symbols, then MSC symbols, one workgroup per frame each
        const int sym_a = part ? 4 : 1, sym_b = part ? kSymbolsPerTf : 4;
        if (!guard_begin(n, &ga)) return -1;
        const hipError_t e = pass == 0
            ? launch_ofdm_demap_fused_guarded(frame_list(), 0, n, ga, stream_, sym_a, sym_b, 1)
            : launch_ofdm_demap_fused_audit(frame_list(), 0, n, ga, stream_, sym_a, sym_b, 1, d_bins.get(), d_prod.get());
        if (!check(e, "fused audit launch")) return -1;
        if (pass == 1 && guard_on) {
          if (!guard_finish(true, 0, n, sym_a, sym_b, false)) return -1;
        } else {
          ++guard_launches_;                              // (guard_finish counts the launch; without it the list is only counted, never acted on)
        }
      }
      std::vector<uint32_t>& keep = pass == 0 ? bits_a : bits_b;
      keep.resize(fic_words + msc_words);
      const bool raw = !(pass == 1 && guard_on);          // bits as the kernel left them
      if (raw && (!check(hipMemcpyAsync(keep.data(), d_fic_bits_.get(), fic_words * 4, hipMemcpyDeviceToHost, stream_), "bits download") ||
                  !check(hipMemcpyAsync(keep.data() + fic_words, d_msc_bits_.get(), msc_words * 4, hipMemcpyDeviceToHost, stream_), "bits download")))
        return -1;
      if (pass == 1 &&
          !check(launch_decision_audit(d_in + static_cast<size_t>(first) * kTfBytes, n, d_bins.get(), d_fic_bits_.get(), d_msc_bits_.get(), d_tw2048_.get(), d_qpsk_.get(),
                                       d_out.get(), stream_, d_prod.get(), kRowLead, guard_rule_level()),
                 "audit launch"))
        return -1;
      if (!guard_download() || !check(hipStreamSynchronize(stream_), "audit") || !guard_check()) return -1;
      counts[pass] = static_cast<uint32_t>(guard_flagged_);
    }
    listed += counts[1];
    list_equal = list_equal && counts[0] == counts[1];
    if (!guard_on) bits_equal = bits_equal && bits_a == bits_b;
  }
  if (!read_audit(d_out.get(), listed, out8)) { set_error("audit download failed"); return -1; }
  if (out_extra) {
    out_extra[0] = guard_on ? -1.0 : (bits_equal ? 1.0 : 0.0);      // (compared on the raw bits only: with the guard on the audit pass's bits are the re-decided ones)
    out_extra[1] = list_equal ? 1.0 : 0.0;
  }
  return nframes;
}

// S1: n code words of `framebits` data bits, symbols 127/129 hard, 128 erased (depuncture.c:36-43)
int Engine::viterbi_batch(const uint8_t* symbols, uint8_t* data, int framebits, int n)
{
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (n <= 0) return 0;
  if (framebits <= 0 || framebits % 32 != 0) { set_error("viterbi: framebits must be a positive multiple of 32"); return -1; }
  // (the chain-back reads a zero word per output word: engine.cpp; refused before the plan enters the table the kernels read)
  if (framebits / 32 > kMaxCodewordWords) { set_error("viterbi: code word too long (at most " + std::to_string(32 * kMaxCodewordWords) + " bits)"); return -1; }
  const int nsteps = framebits + 6, n16 = (nsteps + 15) / 16;
  const int ngroups = (n + 63) / 64;
  CodewordPlan plan;
  std::memset(&plan, 0, sizeof plan);
  plan.nsteps = nsteps;
  plan.out_bytes = framebits / 8;
  const int pid = plan_table_.id(plan);
  std::vector<WaveGroup> groups;
  const int64_t dr = (nsteps + 7) / 8 * 8;
  std::vector<uint4> steps(static_cast<size_t>(ngroups) * n16 * 64, make_uint4(0, 0, 0, 0));
  for (int g = 0; g < ngroups; ++g) {
    groups.push_back(WaveGroup{pid, 64 * g, std::min(64, n - 64 * g), nsteps, static_cast<int64_t>(g) * n16, g * dr});
    for (int l = 0; l < 64; ++l) {
      const int cw = g * 64 + l;
      if (cw >= n) continue;
      const uint8_t* sym = symbols + static_cast<size_t>(cw) * 4 * nsteps;
      for (int t = 0; t < nsteps; ++t) {
        unsigned byte = 0;
        for (int j = 0; j < 4; ++j) {
          const uint8_t sv = sym[4 * t + j];
          if (sv != 128) byte |= (1u << (4 + j)) | ((sv > 128 ? 1u : 0u) << j);
        }
        uint4& u = steps[(static_cast<size_t>(g) * n16 + t / 16) * 64 + l];
        uint32_t* w = &u.x;
        w[(t % 16) / 4] |= byte << (8 * (t % 4));
      }
    }
  }
  // no gather: upload the step rows directly, then run the decoder with an all-zero scrambler
  const size_t out_bytes = static_cast<size_t>(n) * (framebits / 8);
  if (framebits / 32 > kMaxCodewordWords) { set_error("viterbi: code word too long"); return -1; }      // (the zero words the chain-back reads: engine.cpp)
  if (!d_plans_.upload(plan_table_.plans(), stream_) || !d_groups_.upload(groups, stream_) || !d_steps_.upload(steps, stream_) ||
      !d_decisions_.reserve(static_cast<size_t>(ngroups) * dr * 64) || !d_bytes_.reserve(out_bytes))
    return -1;
  if (!check(launch_viterbi(d_groups_.get(), ngroups, nullptr, d_plans_.get(), d_steps_.get(), d_decisions_.get(), d_zero_words_.get(),
                            d_bytes_.get(), framebits / 8, stream_),
             "viterbi launch") ||
      !check(hipMemcpyAsync(data, d_bytes_.get(), out_bytes, hipMemcpyDeviceToHost, stream_), "decoded download") ||
      !check(hipStreamSynchronize(stream_), "viterbi"))
    return -1;
  return n;
}

// ---------------------------------------------------------------------------------------------
// S2 building blocks: one sdr_demod call on an explicit stream
bool Engine::scan_one_call(const uint8_t* iq_virtual_base, StreamState* d_state, uint8_t* d_tail, int call, int chunk, CallDesc* out)
{
  std::vector<const uint8_t*> ptrs = {iq_virtual_base};
  std::vector<int64_t> nb = {static_cast<int64_t>(call + 1) * kChunkBytes};     // (only bounds the kernel's call loop: this is call number `call`, whatever its length)
  if (!d_iq_ptrs_.upload(ptrs, stream_) || !d_nbytes_.upload(nb, stream_) || !d_descs_.reserve(1) || !d_tail_images_.reserve(kTailBytes)) return false;
  // the kernel indexes descs[stream * max_calls + call]; with max_calls = 0 and the pointer moved back by `call` it hits slot 0 (the tail copy likewise)
  SyncArgs a = sync_args(1, 0);
  a.states = d_state;
  a.descs -= call;
  a.info = nullptr;
  SyncScanOpts o;
  o.call_begin = call;
  o.call_end = call + 1;
  o.tails = SyncTails{d_tail, d_tail, d_tail_images_.get() - static_cast<ptrdiff_t>(call) * kTailBytes, chunk};
  if (!check(launch_sync_scan(a, o, stream_), "sync scan launch")) return false;
  return check(hipMemcpyAsync(out, d_descs_.get(), sizeof(CallDesc), hipMemcpyDeviceToHost, stream_), "desc download") &&
         check(hipStreamSynchronize(stream_), "sync scan");
}

bool Engine::demod_one_frame(const uint8_t* iq_virtual_base, const CallDesc& desc, uint8_t* fic_bytes, uint8_t* msc_bytes)
{
  if (!set_frame_list(iq_virtual_base, &desc, 1, 0, true) || !d_spectra_.reserve(static_cast<size_t>(kSymbolsPerTf) * 2048)) return false;   // the frame is {0, 0}
  const bool guard = guard_active();
  GuardArgs ga{};
  guard_new_run();
  if (guard && (!d_delta_.reserve(kSymbolsPerTf) || !guard_begin(1, &ga) ||
                !check(launch_symbol_delta(frame_list(), 0, 1, kSymbolsPerTf, d_delta_.get(), kSymbolsPerTf, guard_c_of(guard_rule_level()), stream_), "symbol delta launch")))
    return false;
  if (!check(launch_ofdm_fft(frame_list(), 0, 1, d_spectra_.get(), stream_), "fft launch") ||
      !check(launch_demap(false, 0, d_spectra_.get(), 0, 1, d_frame_slot_.get(), d_frame_cif_row_.get(), d_qpsk_.get(), d_fic_bits_.get(), d_msc_bits_.get(), ga, stream_), "demap launch") ||
      (guard && !guard_finish(false, 0, 1, 1, kSymbolsPerTf, false)) || (guard && !guard_download()) ||
      !check(hipStreamSynchronize(stream_), "demod") || (guard && !guard_check()))
    return false;
  return unpack_tf_slot(0, fic_bytes, msc_bytes);
}

}  // namespace dabhip
