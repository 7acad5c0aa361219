// engine_ofdm.cpp — the OFDM stage of a decode: frame list, launches, parity guard plumbing (see engine.hpp for the pipeline).
#include "engine_detail.hpp"

namespace dabhip {

static_assert(sizeof(IntPair) == sizeof(int2) && alignof(IntPair) <= alignof(int2), "layout_segment reads h_info_ and writes h_frames_ as {int, int} records");

// ---------------------------------------------------------------------------------------------
// Parity guard around one demapping launch: guard_begin() hands the kernel its list and its counter (all counters of a decode are cleared
// before the first launch); guard_finish() queues the fp64 re-decision of what was listed; guard_download() (once, behind the last launch)
// copies the entry counts to the host; guard_check() (after the stream has been awaited) adds them up and counts the launches whose
// list overflowed (those were decided again in full).
constexpr int kGuardMinLaunches = 64;
constexpr int kGuardSlotWords = 4;                       // a launch's counter and three spare words
bool Engine::guard_begin(int ntf_in_launch, GuardArgs* out)
{
  // the list: flag rates measured on noisy input are a few decisions per TF (7e-6 of 230,400 at 5 dB); 64 entries per TF, at least
  // 256 K, and a launch that overflows it is decided again in full (exact_decide_all_kernel) instead of failing
  // (the proven level's band is 13 x as wide: 16 x the entries)
  const int level = guard_rule_level();
  uint32_t cap = static_cast<uint32_t>(std::min<int64_t>(int64_t(1) << 30, std::max<int64_t>(int64_t(1) << (level >= 2 ? 20 : 18), static_cast<int64_t>(ntf_in_launch) * (level >= 2 ? 512 : 64))));
  if (guard_cap_override_) cap = guard_cap_override_;
  if (guard_launches_ == 0 && h_guard_counts_.size() < static_cast<size_t>(kGuardMinLaunches) * kGuardSlotWords && !h_guard_counts_.resize(static_cast<size_t>(kGuardMinLaunches) * kGuardSlotWords)) return false;
  if (static_cast<size_t>(guard_launches_ + 1) * kGuardSlotWords > h_guard_counts_.size()) { set_error("parity guard: more guarded launches than planned for in one decode"); return false; }
  if (!d_guard_list_.reserve(cap) || !d_guard_counter_.reserve(h_guard_counts_.size())) return false;
  guard_cap_ = guard_cap_override_ ? guard_cap_override_ : static_cast<uint32_t>(std::min<size_t>(d_guard_list_.capacity(), 0xffffffffu));
  // every launch of a decode has its own counter: ONE clear before the first and ONE download behind the last (guard_download) instead of a
  // clear and a download per launch (small copy-engine operations cost 20 .. 35 us of idle GPU each between two kernels); a decode's layout
  // kernel has normally cleared them already (guard_counters_clear_)
  if (guard_launches_ == 0 && !guard_counters_clear_ &&
      !check(hipMemsetAsync(d_guard_counter_.get(), 0, h_guard_counts_.size() * sizeof(uint32_t), stream_), "guard counters"))
    return false;
  guard_counters_clear_ = false;
  // the capacity THIS launch was given (a later launch of the same decode may find the list re-reserved and larger): guard_check compares with it
  if (guard_caps_.size() <= static_cast<size_t>(guard_launches_)) guard_caps_.resize(static_cast<size_t>(guard_launches_) + 1);
  guard_caps_[static_cast<size_t>(guard_launches_)] = guard_cap_;
  *out = GuardArgs{d_delta_.get(), kSymbolsPerTf, guard_c_of(level), guard_prod_of(level), level >= 2 ? 1 : 0, guard_cap_, d_guard_list_.get(),
                   d_guard_counter_.get() + static_cast<size_t>(guard_launches_) * kGuardSlotWords};
  return true;
}
// the counters' host and device arrays for a decode of ntf frames (the layout kernel clears the device side)
bool Engine::guard_reserve_counters(int ntf)
{
  const size_t words = (static_cast<size_t>(kGuardMinLaunches) + 2 * static_cast<size_t>(ntf / limits_.fft_chunk_tfs + 1)) * kGuardSlotWords;
  return (h_guard_counts_.size() >= words || h_guard_counts_.resize(words)) && d_guard_counter_.reserve(h_guard_counts_.size());
}
bool Engine::guard_finish(bool planar, int first, int n, int sym_a, int sym_b, bool skip_fic)
{
  uint32_t* const counter = d_guard_counter_.get() + static_cast<size_t>(guard_launches_) * kGuardSlotWords;    // guard_begin's
  ++guard_launches_;
  const FrameListArgs fl = frame_list();
  return check(launch_exact_decide(d_guard_list_.get(), counter, guard_cap_, fl, d_tw2048_.get(), planar, stream_), "exact decide launch") &&
         check(launch_exact_decide_all(counter, guard_cap_, fl, first, n, sym_a, sym_b, d_tw2048_.get(), planar, skip_fic, stream_), "exact decide (overflow) launch");
}
// behind the last guarded launch of a decode, before the stream is awaited
bool Engine::guard_download()
{
  return guard_launches_ == 0 ||
         check(hipMemcpyAsync(h_guard_counts_.data(), d_guard_counter_.get(), static_cast<size_t>(guard_launches_) * kGuardSlotWords * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_),
               "guard count download");
}
bool Engine::guard_check()
{
  for (int i = 0; i < guard_launches_; ++i) {
    const uint32_t count = h_guard_counts_[static_cast<size_t>(i) * kGuardSlotWords];
    if (count > guard_caps_[static_cast<size_t>(i)]) ++guard_overflows_;       // that launch was decided again in full: still exact, only slow
    guard_flagged_ += count;
  }
  guard_launches_ = 0;
  return true;
}

// the argument block of every launch over the frame list: THE one place that names these buffers (taken afresh before a launch: a reserve may move them)
FrameListArgs Engine::frame_list() const
{
  return FrameListArgs{d_iq_ptrs_.get(), d_descs_.get(), list_max_calls_, d_frames_.get(), d_twf_.get(), d_frame_slot_.get(), d_frame_cif_row_.get(), d_qpsk_.get(),
                       d_fic_bits_.get(), d_msc_bits_.get()};
}
bool Engine::set_frame_list(const uint8_t* d_iq, const CallDesc* descs, int n, int row_lead, bool bit_rows)
{
  if (!h_ptrs_.resize(1) || !h_frames_.resize(n) || !h_frame_slot_.resize(n) || !h_frame_cif_row_.resize(n)) return false;      // (page-locked: they outlive this call)
  h_ptrs_[0] = d_iq;
  for (int j = 0; j < n; ++j) {
    h_frames_[j] = make_int2(0, j);
    h_frame_slot_[j] = j;
    h_frame_cif_row_[j] = row_lead + 4 * j;
  }
  last_.pending = false;             // the last decode's frame list and descriptors are gone: its deferred TFs can no longer be completed
  if (!(!bit_rows || reserve_tf_slots(n)) || !d_frame_slot_.upload(h_frame_slot_.data(), n, stream_) || !d_frame_cif_row_.upload(h_frame_cif_row_.data(), n, stream_)) return false;
  if (!descs) return true;           // (stage_demap: spectra, no samples -- its launch reads the slots and rows only)
  list_max_calls_ = n;               // (one stream: its descriptors are descs[call])
  return d_iq_ptrs_.upload(h_ptrs_.data(), 1, stream_) && d_descs_.upload(descs, n, stream_) && d_frames_.upload(h_frames_.data(), n, stream_);
}
const uint8_t* Engine::frames_on_device(const uint8_t* frames, int nframes, bool on_device)
{
  if (on_device) return frames;
  const size_t bytes = static_cast<size_t>(nframes) * kTfBytes;
  if (!d_iq_own_.reserve(bytes) || !check(blocking_copy(d_iq_own_.get(), frames, bytes, hipMemcpyHostToDevice), "frame upload")) return nullptr;
  return d_iq_own_.get();
}
GuardArgs Engine::soft_guard_args() const { return GuardArgs{d_delta_.get(), kSymbolsPerTf, kSoftNormC, 0.0f, 0, 0u, nullptr, nullptr}; }

// The one-kernel OFDM stage over frames [first, first + n) of the frame list, data symbols [sym_a, sym_b), nparts workgroups per frame
bool Engine::fused_parts(int first, int n, int sym_a, int sym_b, int nparts)
{
  const FrameListArgs fl = frame_list();
  if (soft_bits_ != 0) return check(launch_ofdm_demap_fused_soft(afc_, fl, first, n, stream_, sym_a, sym_b, nparts), "fused fft/demap launch");
  const bool guard = guard_active();
  GuardArgs ga{};
  if (guard && !guard_begin(n, &ga)) return false;
  const bool launched = check(guard ? launch_ofdm_demap_fused_guarded(fl, first, n, ga, stream_, sym_a, sym_b, nparts)
                                    : launch_ofdm_demap_fused_plain(afc_, fl, first, n, stream_, sym_a, sym_b, nparts),
                              "fused fft/demap launch");
  return launched && (!guard || guard_finish(true, first, n, sym_a, sym_b, false));
}

// K2 + K2b over the 72 MSC symbols of frames [first, first + n) in chunks (the two-kernel stage's chunks share one spectra buffer; stream order keeps
// them apart), timed with per-chunk events.  The FIC symbols of those frames ran before (stage A of decode_impl).
bool Engine::ofdm_msc_part(int first, int n, int chunk, int ev_base)
{
  const bool guard = guard_active(), soft = soft_bits_ != 0, energies = guard || soft;
  bool gpu_ok = true;
  const Pieces cut{n, chunk};
  for (int c = 0; c < cut.count() && gpu_ok; ++c) {
    const int f0 = first + static_cast<int>(cut.first(c)), nf = static_cast<int>(cut.size(c));
    ++report_.ofdm_chunks;
    Event* const ev = ev_base >= 0 ? &chunk_ev_[static_cast<size_t>(3) * (ev_base + c)] : nullptr;
    gpu_ok = !ev || record(ev[0], stream_);
    if (fused_) {
      // the 72 MSC symbols (the FIC symbols ran before the FIC decode was queued); workgroups per frame: measurement knob
      static const int msc_wgs = std::getenv("DABHIP_FUSED_MSC_WGS") ? std::max(1, std::min(8, std::atoi(std::getenv("DABHIP_FUSED_MSC_WGS")))) : 1;
      gpu_ok = gpu_ok && fused_parts(f0, nf, 4, 76, msc_wgs);
      gpu_ok = gpu_ok && (!ev || record(ev[1], stream_));
    } else {
      GuardArgs ga = soft ? soft_guard_args() : GuardArgs{};   // (hard decisions: a non-null delta switches the guard's listing on)
      if (guard && !guard_begin(nf, &ga)) return false;
      // with the guard on (or soft decisions), K2 also leaves the per-symbol sample energies K2b decides with
      gpu_ok = gpu_ok && check(launch_ofdm_fft(frame_list(), f0, nf, d_spectra_.get(), stream_, energies ? d_delta_.get() : nullptr,
                                               soft ? kSoftNormC : guard_c_of(guard_rule_level())),
                               "fft launch");
      gpu_ok = gpu_ok && (!ev || record(ev[1], stream_));
      gpu_ok = gpu_ok && check(launch_demap(true, soft_bits_, d_spectra_.get(), f0, nf, d_frame_slot_.get(), d_frame_cif_row_.get(), d_qpsk_.get(), d_fic_bits_.get(), d_msc_bits_.get(), ga, stream_), "demap launch");
      if (guard) gpu_ok = gpu_ok && guard_finish(true, f0, nf, 1, kSymbolsPerTf, true);     // timed with the demapper; the FIC symbols belong to the pre-pass
    }
    gpu_ok = gpu_ok && (!ev || record(ev[2], stream_));
  }
  return gpu_ok;
}

// read_demapped_tf asked for a TF whose MSC part the last decode deferred: that part now, over all deferred frames of that decode -- its frame list, call
// descriptors and IQ pointers are still on the device (the engine's own upload buffer outlives the decode; device-resident input must still be where it was).
bool Engine::complete_deferred()
{
  const int first = seg_.nmsc, n = seg_.ntf - seg_.nmsc;
  if (!last_.pending || n <= 0) return true;
  if (!fused_ && !d_spectra_.reserve(static_cast<size_t>(last_.chunk) * kSymbolsPerTf * 2048)) return false;
  const bool guard = guard_active();
  guard_new_run();
  bool gpu_ok = ofdm_msc_part(first, n, last_.chunk, -1);
  if (guard && gpu_ok) gpu_ok = guard_download();
  const bool drained = check(hipStreamSynchronize(stream_), "deferred MSC symbols");      // also on the error path: nothing may stay in flight
  if (!gpu_ok || !drained) return false;
  if (guard && !guard_check()) return false;
  last_.pending = false;
  for (StreamCarry& c : carry_)
    std::fill(c.msc_missing.begin() + std::min<size_t>(static_cast<size_t>(c.last_keep), c.msc_missing.size()), c.msc_missing.end(), uint8_t(0));
  return true;
}

// The frame list of this decode / segment (segment_layout.hpp) into seg_ and, in one launch, onto the device: called by the scan as soon as the calls'
// {status, ordinal} are on the host (h_info_), i.e. while K1's verification kernel still runs, and again after a re-scan.
bool Engine::layout_frames(const size_t* nbytes, int nstreams)
{
  const auto tfr = std::chrono::steady_clock::now();
  SegmentLayout& seg = seg_;
  const int max_calls = list_max_calls_ = scan_.max_calls;
  const size_t nd = scan_.ndesc;
  if (!h_frames_.resize(nd) || !h_frame_slot_.resize(nd) || !h_frame_cif_row_.resize(nd)) return false;   // page-locked: uploaded asynchronously
  // Lock-in skip: the leading TFs of a stream that cannot be locked (a fresh decode's planes are reset later, inside the control-plane pass: their
  // content here is stale) go to the END of the list: the FIC launches run over the whole list, the MSC launches over [0, nmsc)
  seg_ncalls_.resize(nstreams);
  seg_defer_max_.resize(nstreams);
  for (int b = 0; b < nstreams; ++b) {
    seg_ncalls_[b] = static_cast<int>(nbytes[b] / kChunkBytes) - carry_[b].calls_done;
    seg_defer_max_[b] = demod_all_ ? 0 : (planes_fresh_ ? lockin_deferred(false, 0, max_calls) : lockin_deferred(planes_[b].locked(), planes_[b].okcount(), max_calls));
  }
  std::string error;
  if (!layout_segment(reinterpret_cast<const IntPair*>(h_info_.data()), max_calls, seg_ncalls_.data(), carry_, seg_defer_max_.data(), seg,
                      reinterpret_cast<IntPair*>(h_frames_.data()), h_frame_slot_.data(), h_frame_cif_row_.data(), &error)) {
    set_error(error);
    return false;
  }
  // the three lists go up in ONE launch that reads the page-locked arrays itself (three copy-engine copies cost 45 us of idle GPU before the first
  // OFDM launch); with the guard on it also clears the guard's counters, which guard_begin() then leaves alone
  bool up = true;
  if (seg.ntf > 0) {
    up = d_frames_.reserve(seg.ntf) && d_frame_slot_.reserve(seg.ntf) && d_frame_cif_row_.reserve(seg.ntf);
    HostWordsArgs hw{};
    hw.set(0, h_frames_.data(), d_frames_.get(), 2 * static_cast<size_t>(seg.ntf));
    hw.set(1, h_frame_slot_.data(), d_frame_slot_.get(), static_cast<size_t>(seg.ntf));
    hw.set(2, h_frame_cif_row_.data(), d_frame_cif_row_.get(), static_cast<size_t>(seg.ntf));
    if (up && guard_active() && guard_launches_ == 0 && guard_reserve_counters(seg.ntf)) {
      hw.zero = d_guard_counter_.get();
      hw.nzero = static_cast<uint32_t>(h_guard_counts_.size());
      guard_counters_clear_ = true;
    }
    up = up && check(launch_host_words(hw, stream_), "frame list upload");
  }
  layout_ms_ += ms_since(tfr);
  return up;
}

}  // namespace dabhip
