// engine.hpp — batch engine: B independent cu8 IQ streams resident in HBM -> ETI frames.
//
// Pipeline of one decode() (kernel files in brackets):
//   K1  sync scan            [k_sync.hip]   one workgroup per stream, sequential over its TFs
//   K2  OFDM FFT             [k_fft.hip]    all demodulated TFs, chunked to bound the spectra buffer
//   K2b DQPSK/demap          [k_fft.hip]    -> bit-packed FIC / MSC rows, kept for the whole batch
//   K3  FIC decode           [k_decode.hip] gather + Viterbi + CRC -> 12 FIBs per TF  (D2H: 396 B/TF)
//   --  control plane        [control_plane.hpp, host] lock FSM, CIF ring, ETI headers, work lists
//   K4  MSC decode           [k_decode.hip] gather (time de-interleave + de-puncture) + Viterbi
//   K5  ETI finish           [k_decode.hip] header, FIBs, EOF CRC, trailer
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "control_plane.hpp"
#include "decoder_form.hpp"
#include "device_types.hpp"
#include "hip_util.hpp"
#include "launch_limits.hpp"
#include "scan_plan.hpp"
#include "segment_layout.hpp"
#include "thread_pool.hpp"
#include "worklist.hpp"

namespace dabhip {

struct FrameListArgs;     // kernels.hpp
struct SyncArgs;

// std::allocator over page-locked host memory: vectors that are uploaded every decode (the work lists) go to the device
// as plain asynchronous DMA instead of staged copies that block the issuing thread
template <class T>
struct PinnedAllocator {
  using value_type = T;
  PinnedAllocator() = default;
  template <class U>
  PinnedAllocator(const PinnedAllocator<U>&) {}
  T* allocate(size_t n)
  {
    void* p = nullptr;
    if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) throw std::bad_alloc();
    return static_cast<T*>(p);
  }
  void deallocate(T* p, size_t) { (void)hipHostFree(p); }
  template <class U>
  bool operator==(const PinnedAllocator<U>&) const { return true; }
  template <class U>
  bool operator!=(const PinnedAllocator<U>&) const { return false; }
};
template <class T>
using HostList = std::vector<T, PinnedAllocator<T>>;

// grow-only page-locked host allocation (device copies to and from it run at full PCIe rate and truly asynchronously)
template <class T>
class PinnedBuffer {
 public:
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  ~PinnedBuffer() { if (p_) (void)hipHostFree(p_); }
  bool resize(size_t n)
  {
    size_ = n;
    if (n <= cap_) return true;
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    cap_ = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), hipHostMallocDefault) != hipSuccess) {
      p_ = nullptr;
      size_ = 0;
      set_error("hipHostMalloc of " + std::to_string(n * sizeof(T)) + " bytes failed");
      return false;
    }
    cap_ = n;
    return true;
  }
  T* data() const { return p_; }
  size_t size() const { return size_; }
  T& operator[](size_t i) const { return p_[i]; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0, size_ = 0;
};

struct StageTimes {
  float sync = 0, fft = 0, demap = 0, fic = 0, control = 0, gather = 0, viterbi = 0, eti = 0;
  float setup = 0, frames = 0, worklist = 0, wall = 0;   // host-side phases (wall clock)
  float sync_fp64_calls = 0;                             // K1 verification: calls whose fp32 arg-max was not clear-cut (decided in fp64)
  float sync_spec_calls = 0;                             // K1 chain: calls whose estimators came out of the look-ahead pass's table (0: the plain chain ran)
  float h2d = 0;                                         // host-fed decode: upload of the IQ (HIP events; 0 when the IQ was resident)
  double h2d_bytes = 0, h2d_pinned_bytes = 0;            // bytes uploaded, and how many of them came from page-locked memory
};

// the MSC decode's work lists (worklist.hpp) in page-locked memory: they go to the device as plain asynchronous DMA
using DecodeBatch = DecodeBatchT<PinnedAllocator>;
using MscWork = MscWorkT<PinnedAllocator>;

class Engine {
 public:
  // host_threads: threads of the per-stream control-plane pool (0 = half the cores, at most 24; DABHIP_HOST_THREADS overrides)
  // cpus: the CPUs this engine's host threads (control-plane pool, host lane) are bound to; empty = those of the device's NUMA node on a machine
  // with more than one (placement.hpp), or none
  explicit Engine(int device, int host_threads = 0, std::vector<int> cpus = {});
  const std::vector<int>& host_cpus() const { return host_cpus_; }
  int numa_node() const { return numa_node_; }
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  bool ok() const { return ok_; }
  const uint8_t* eti_buffer() const { return d_eti_.get(); }
  // software AFC: an NCO per stream steered by the reference's tuner rule; off = parity mode
  void set_afc(bool on) { afc_ = on; }
  // soft-decision decoding (not in the reference): 4-bit soft values from the demapper through
  // de-interleaving and de-puncturing into the Viterbi branch metrics.  Batch path only; off = parity mode.
  // K2 + K2b as one kernel that never writes the spectra (k_fused.hip; hard decisions only; the default) or as the two
  // kernels K2 (the HBM-roofline stage of SURVEY.md 8(d), always measurable on its own: fft_roofline) and K2b.  The output
  // bits are identical either way.
  void set_fused(bool on) { fused_ = on; }
  // Lock-in skip (default on): the 72 MSC symbols of the TFs that cannot be locked whatever their FIBs say (control_plane.hpp: lockin_deferred --
  // the first 9 - okcount TFs of a stream that is not locked when the decode starts) are not demodulated: no ETI frame ever reads them.
  // read_demapped_tf completes them on demand.  on = true (DABHIP_DEMOD_ALL=1): every TF is demodulated in full, as before.
  void set_demod_all(bool on) { demod_all_ = on; }
  int msc_deferred() const { return last_.deferred; }    // TFs of the last decode / segment whose MSC part was deferred (completed on demand or not)
  // K1's chain: 0 = call after call, 1 = with the look-ahead pass, -1 = the pass for small batches (include/dabhip.h: dabhip_engine_set_sync_speculation)
  void set_sync_speculation(int mode) { spec_mode_ = mode < 0 ? -1 : (mode > 0 ? 1 : 0); }
  // sub-channel filter (TODO.md:28-31): bit i = SubChId i is decoded and carried in the ETI frames; takes effect with the next
  // decode() / first segment of a session.  All ones (default) = the reference's frames.
  void set_subchannel_filter(uint64_t keep) { subch_keep_ = keep; }
  void set_soft(bool on) { soft_bits_ = on ? 4 : 0; tf_slots_ = 0; msc_rows_ = 0; }
  // Viterbi decoder forms (include/dabhip.h: DABHIP_FORM_*; test plumbing): -1 = the rule of the knobs and defaults below, else that form for
  // every MSC / FIC launch.  False for a form the decoder does not have (TWO, TWO_PLAIN for the FIC).  forms_ran: bit f = form f ran in a
  // launch since clear_forms_ran() (a multi-lane form asked of a soft engine runs, and reports, the lane form -- with set_soft_lanes on only TWO does:
  // FOUR, and TWO_PLAIN for the MSC, then run as asked).
  bool set_decoder_forms(int msc_form, int fic_form);
  // soft decisions through the four-lane and table-free two-lane forms (decoder_form.hpp: FormKnobs::soft_lanes); any time, like set_decoder_forms
  void set_soft_lanes(bool on) { knobs_.soft_lanes = on; }
  void clear_forms_ran() { msc_ran_ = 0; fic_ran_ = 0; }
  uint32_t msc_forms_ran() const { return msc_ran_.load(); }
  uint32_t fic_forms_ran() const { return fic_ran_.load(); }
  // parity guard (k_parity.hip; default on): hard decisions whose fp32 margin lies inside the error band of the fp32 OFDM
  // transform are re-decided in fp64 from the int8 samples, so the demapped bits are those of exact arithmetic (what the
  // reference's fp64 FFTW path yields).  Inactive with soft decisions and with the software AFC (no reference semantics there).
  // level: 0 = off (raw fp32 decisions), 1 = the measured constants, 2 = the proven ones (device_types.hpp: kGuardC.. / kGuardCProven..)
  void set_parity_guard(int level) { guard_level_ = level < 0 ? kDefaultGuardLevel : (level > 2 ? 2 : level); }   // < 0: the default level
  int parity_guard_level() const { return guard_level_; }
  // decisions flagged and re-decided by the guard in the last decode (FIC pre-pass + OFDM stage), and decisions taken
  // the reference's operator messages of one stream (ControlPlane::take_log): text pending since the last call, cleared by it
  std::string take_stream_log(int stream) { return (stream >= 0 && stream < static_cast<int>(planes_.size())) ? planes_[static_cast<size_t>(stream)].take_log() : std::string(); }
  void guard_stats(int64_t* flagged, int64_t* decisions) const { if (flagged) *flagged = guard_flagged_; if (decisions) *decisions = guard_decisions_; }
  int guard_overflows() const { return guard_overflows_; }
  void set_guard_list_cap(uint32_t cap) { guard_cap_override_ = cap; }   // test knob: a tiny list makes the overflow path run
  // test knob (launch_limits.hpp): v[0 .. kLaunchLimitCount), 0 = the default.  False, with the limits as they were, for a value no launch could be made with
  bool set_launch_limits(const int64_t* v);
  const LaunchLimits& launch_limits() const { return limits_; }
  // the launches of the last decode / segment / stage entry, loop by loop (the session's device gathers: dabhip_stream_launch_report adds them)
  const LaunchReport& launch_report() const { return report_; }
  void clear_launch_report() { report_ = LaunchReport{}; }
  // the MSC batch of the last decode as the host planned it: trellis steps of every wave-group in launch order (at most cap), tiles of 64 records; returns the groups
  int msc_plan(int32_t* nsteps, int cap, int64_t* ntiles) const
  {
    const DecodeBatch& b = work_.batch;
    if (ntiles) *ntiles = work_.nframes ? static_cast<int64_t>(b.job_ids.size() / 64) : 0;
    if (work_.nframes == 0) return 0;
    for (size_t g = 0; nsteps && g < b.groups.size() && static_cast<int>(g) < cap; ++g) nsteps[g] = b.groups[g].nsteps;
    return static_cast<int>(b.groups.size());
  }

  // -- batch path ---------------------------------------------------------------------------
  int64_t decode(const uint8_t* const* iq, const size_t* nbytes, int nstreams, bool on_device);
  // -- streaming sessions: decode() of an unbounded stream, one segment at a time ------------
  int64_t feed(const uint8_t* const* iq_virtual, const size_t* avail, int nstreams, bool first_segment);
  int64_t stream_need_from(int stream) const;   // oldest stream byte the next segment may still read
  int64_t eti_count(int stream) const;
  // StreamFault bits (control_plane.hpp) of the stream's multiplex in the last decode / so far in the session: such a stream emits no frames while
  // its signalled multiplex is one the reference could not assemble inside its own arrays; every other stream of the batch is unaffected
  uint32_t stream_status(int stream) const;
  int64_t eti_read(int stream, uint8_t* dst, int64_t cap_frames);
  // All frames of the last decode / segment (stream-major, emission order) to host memory on a stream of their own, without waiting: the copy
  // runs beside the NEXT decode's scan and OFDM stage (only its K4, which rewrites the ETI buffer, waits for it).  dst should be page-locked.
  // eti_fetch_wait() returns when the bytes are there.  The output side of the CLI contract (dab2eti.c:132-135) at the link's rate.
  int64_t eti_fetch_async(uint8_t* dst, int64_t cap_frames);
  bool eti_fetch_wait();
  const uint8_t* eti_device(int64_t* nframes) const;
  int trace(int stream, int32_t* ints6, double* ffs, int cap_calls) const;
  int trace_nco(int stream, int32_t* nco_hz, int cap_calls) const;      // software AFC: the frequency each call's samples were de-rotated by
  const StageTimes& stage_times() const { return times_; }
  void fft_stats(int64_t* launches, int64_t* tfs, double* ms) const;
  int fft_roofline(int reps, int64_t* launches, int64_t* tfs, double* ms);   // K2 alone over the last decode's frames

  // -- stage entries --------------------------------------------------------------------------
  int stage_ofdm_fft(const uint8_t* frames, int nframes, float* spectra, bool on_device, int reps, float* kernel_ms);
  int stage_demap(const float* spectra, int nframes, uint8_t* fic, uint8_t* msc);
  int stage_fic_decode(const uint8_t* fic, int nframes, uint8_t* fibs, uint8_t* crc_ok);
  int stage_decision_audit(const uint8_t* frames, int nframes, bool on_device, bool guard_on, double* out8, bool fused = false, double* out_extra = nullptr);
  int stage_decision_audit_fused(const uint8_t* frames, int nframes, bool on_device, bool guard_on, double* out8, double* out_extra);
  int viterbi_batch(const uint8_t* symbols, uint8_t* data, int framebits, int n);

  // -- building blocks shared with the streaming seams (capi_seams.cpp) ------------------------------
  // FIC rows / FIB records for nslots TFs and msc_rows logical CIF rows (default 4 per slot + 15 lead-in + 1)
  bool reserve_tf_slots(int nslots, int msc_rows = -1);
  // host 0/1 bytes of one demapped TF -> bit rows of TF slot `slot`
  bool store_tf_bytes(int slot, const uint8_t* fic_bytes, const uint8_t* msc_bytes);
  // S3 recycling: keep the newest `keep_slots` TF slots (and the logical CIF rows still being filled) at the front
  bool recycle_tf_slots(int used_slots, int keep_slots);
  // FIC-decode TF slots [first, first+n): FIBs and CRC flags to host
  bool fic_decode_slots(int first, int n, uint8_t* fibs_host, uint8_t* ok_host);
  bool fic_decode_slots_async(int first, int n, uint8_t* fibs_host, uint8_t* ok_host, hipStream_t copy);   // completion: ev_fibs_
  // decode the ETI frames described by the per-stream job lists into the ETI buffer (stream-major order)
  // stream_row_base[b]: logical CIF row of stream b's CIF 0; stream_fib_base[b]: FIB block (4 per TF slot) of its CIF 0
  bool msc_decode(const std::vector<const JobList*>& stream_jobs, const std::vector<const ControlPlane*>& planes,
                  const std::vector<int>& stream_row_base, const std::vector<int>& stream_fib_base)
  {
    return msc_prepare(stream_jobs, planes, stream_row_base, stream_fib_base, work_s3_) && msc_run(work_s3_);   // reused: its lists are page-locked
  }
  // host half (work lists, headers, plans) and GPU half (regroup, Viterbi, ETI finish) of msc_decode
  bool msc_prepare(const std::vector<const JobList*>& stream_jobs, const std::vector<const ControlPlane*>& planes,
                   const std::vector<int>& stream_row_base, const std::vector<int>& stream_fib_base, MscWork& out);
  bool msc_run(MscWork& w);
  bool msc_upload(const MscWork& w, hipStream_t s);
  bool msc_launch(const MscWork& w);
  bool read_eti(int64_t first, int64_t n, uint8_t* dst);
  // the demapped values (hard: 0 / 1, soft: -7 .. 7) of one TF of the last decode, in the reference's hand-off order (dab.h:27-33)
  bool read_demapped_tf(int stream, int tf, int8_t* fic_out, int8_t* msc_out);
  // front end on an explicit single stream (S2 seam): calls [call, call+1)
  // d_tail: the seam's kTailBytes tail bytes (device, zero at sdr_init); chunk: bytes this call appended (input_buffer_len)
  bool scan_one_call(const uint8_t* iq_virtual_base, StreamState* d_state, uint8_t* d_tail, int call, int chunk, CallDesc* out);
  bool demod_one_frame(const uint8_t* iq_virtual_base, const CallDesc& desc, uint8_t* fic_bytes, uint8_t* msc_bytes);
  hipStream_t stream() const { return stream_; }
  int device() const { return device_; }

  // -- transmitter identification (tii.cpp; include/dabhip.h: "TII") -------------------------------------
  // on: every later decode / segment also folds the null symbols of its counted frames onto the streams' sums (k_tii.hip), one launch behind the OFDM
  // stage's.  A decode() starts from zero sums; a session's further segments add to them until tii_reset().
  void set_tii(bool on) { tii_ = on; }
  bool tii_sums(int stream, uint64_t* T, int* frames);      // a stream's 192 sums and the frames counted
  bool tii_reset();
  float tii_ms() const { return tii_ms_; }
  int stage_tii(const uint8_t* frames, int nframes, const int32_t* w0, const uint32_t* step, bool on_device, uint64_t* T);

 private:
  bool check(hipError_t e, const char* what);
  bool record(hipEvent_t e, hipStream_t s);
  bool elapsed(float* ms, hipEvent_t a, hipEvent_t b);
  bool hard_only(const char* what);
  // one decode_impl call: what its stages share
  struct DecodeRun {
    const size_t* nbytes;
    int nstreams;
    bool cont;                               // a session's further segment
    std::chrono::steady_clock::time_point wall0;
    int chunk = 1;                           // frames per launch of the OFDM stage
    bool host_ok = true;                     // the control-plane pass's outcome
    std::string host_error;
    void mark(const char* what) const;       // DABHIP_TRACE_HOST: a line with the time since wall0
  };
  int64_t decode_impl(const uint8_t* const* iq, const size_t* nbytes, int nstreams, bool on_device, bool cont, bool full_scan = false);
  bool begin_decode(int nstreams, bool cont);
  bool stage_a(DecodeRun& run);              // layout's buffers, then the FIC symbols of every TF through the OFDM stage
  void control_pass(DecodeRun& run);         // control plane + work lists, on the host lane
  bool layout_frames(const size_t* nbytes, int nstreams);
  // called when the calls' {status, ordinal} are on the host (h_info_) -- early in the split scan, again after a re-scan.  A fresh decode runs stage A from here
  bool layout_and_a(DecodeRun& run) { return layout_frames(run.nbytes, run.nstreams) && (run.cont || stage_a(run)); }
  // K1 (engine_scan.cpp): scan_begin = buffers, the plan (scan_) and the set-up launch; scan_chain = the split scan's launches; scan_fetch = the results the
  // host needs, awaited; scan_again = the streams that broke the chain's assumption once more, in the reference's order
  bool scan_streams(const uint8_t* const* iq, bool on_device, bool full_scan, DecodeRun& run);
  bool scan_begin(const uint8_t* const* iq, bool on_device, bool full_scan, const DecodeRun& run);
  bool scan_chain(bool cont);
  bool scan_fetch();
  bool scan_again(DecodeRun& run);
  SyncArgs sync_args(int nstreams, int max_calls) const;   // the block K1's launches share (kernels.hpp)
  // host-fed decode: the streams' bytes into d_iq_own_ (ptrs[b] = where stream b landed), queued on the main stream
  bool upload_iq(const uint8_t* const* iq, const size_t* nbytes, int nstreams, const uint8_t** ptrs);
  bool carry_and_reserve(const SegmentLayout& seg);
  // Several small host arrays to the device in one launch per four of them (launch_host_words: the kernel reads page-locked host memory itself) instead
  // of one copy-engine command each -- a small decode is made of those commands and the 5 .. 10 us of idle GPU between two of them.  Arrays that are
  // not page-locked are staged in `staging` first.  The staging words and the page-locked sources are read when the launch RUNS, not when it is queued:
  // every call site has its own SmallStage, whose event marks the end of its last launch -- a call that finds that launch still in flight waits for it
  // before it overwrites the words (no caller does that today: every one drains its stream in between; the wait turns a silent overwrite into a stall).  Large lists
  // (more than kSmallUploadBytes in all) go as plain asynchronous copies, as before.  dst: device memory, reserved by the caller.
  struct SmallUpload {
    const void* src;
    void* dst;
    size_t bytes;
    bool pinned;
  };
  static constexpr size_t kSmallUploadBytes = 256 * 1024;
  struct SmallStage {
    PinnedBuffer<uint32_t> words;
    Event done;                              // recorded behind the stage's last launch
    bool armed = false;
  };
  bool upload_small(const SmallUpload* items, int n, hipStream_t s, SmallStage& staging);
  // MSC decode batch (its work lists uploaded: msc_upload): regroup + Viterbi launches
  bool launch_decode_batch(const DecodeBatch& b, const uint32_t* bits, const int* d_stream_cif_base, const uint32_t* prbs, uint8_t* out,
                           int record_stride);
  bool msc_launch_async(const MscWork& w);   // K4 + K5 queued, nothing awaited
  void msc_collect();                        // their stage times, once the stream has been awaited
  bool unpack_tf_slot(int slot, uint8_t* fic_bytes, uint8_t* msc_bytes);

  // parity guard plumbing: list + counter for one launch, fix-up after it, entry count to the host (checked at the end)
  bool guard_active() const { return guard_level_ > 0 && soft_bits_ == 0 && !afc_; }
  int guard_rule_level() const { return guard_level_ > 0 ? guard_level_ : kDefaultGuardLevel; }   // the rule the audits count with when the guard is off
  bool guard_begin(int ntf_in_launch, GuardArgs* out);
  // the launch just queued covered frames [first, first + n) of the frame list, data symbols [sym_a, sym_b); skip_fic: another launch owns symbols 1..3
  bool guard_finish(bool planar, int first, int n, int sym_a, int sym_b, bool skip_fic);
  bool guard_download();
  bool guard_reserve_counters(int ntf);
  bool guard_check();
  // the OFDM stage's launches over frames [first, first + n) of the frame list: fused_parts = the one-kernel stage's data symbols [sym_a, sym_b);
  // ofdm_msc_part = the 72 MSC symbols through the configured stage (fused / two-kernel, hard / soft, guard as set) in chunks of `chunk` frames,
  // with three timing events per chunk from chunk_ev_[3 * ev_base] on when ev_base >= 0
  FrameListArgs frame_list() const;    // the block those launches share, from the buffers as they stand now (kernels.hpp)
  // stage entries and the S2 seam: n frames of ONE stream (d_iq) become the frame list -- frame j = call j (descs[j]: the caller's, alive until it has
  // awaited the stream; null: slots and rows only), TF slot j, MSC rows from row_lead + 4 j; bit_rows: those slots' rows are reserved
  bool set_frame_list(const uint8_t* d_iq, const CallDesc* descs, int n, int row_lead, bool bit_rows);
  const uint8_t* frames_on_device(const uint8_t* frames, int nframes, bool on_device);   // host frames into d_iq_own_; null: failed
  // a new run of guarded launches: their counters start over (guard_new_count: the flagged decisions' count too)
  void guard_new_run() { guard_launches_ = 0; guard_counters_clear_ = false; }
  void guard_new_count() { guard_new_run(); guard_flagged_ = 0; }
  GuardArgs soft_guard_args() const;   // soft decisions, two-kernel stage: K2b reads the energies K2 left, lists nothing
  bool fused_parts(int first, int n, int sym_a, int sym_b, int nparts);
  bool ofdm_msc_part(int first, int n, int chunk, int ev_base);
  bool complete_deferred();            // read_demapped_tf: the MSC part of the last decode's deferred frames, awaited
  bool tii_tables();                   // the mixer's table on the device, the timing events
  bool tii_begin(int nstreams, bool cont);   // the sums' rows reserved, and cleared unless a session goes on
  bool tii_launch();                   // over the scan's descriptors as they stand, timed

  bool ok_ = false;
  bool afc_ = false, fused_ = true;
  bool demod_all_ = std::getenv("DABHIP_DEMOD_ALL") != nullptr && std::atoi(std::getenv("DABHIP_DEMOD_ALL")) != 0;
  int guard_level_ = kDefaultGuardLevel;
  uint64_t subch_keep_ = ~0ull;
  int soft_bits_ = 0;
  FormKnobs knobs_;                            // decoder_form.hpp: the thresholds of the forms' rule, environment overrides applied
  int msc_form_ = -1, fic_form_ = -1;          // set_decoder_forms: -1 = the rules above
  std::atomic<uint32_t> msc_ran_{0}, fic_ran_{0};
  std::unique_ptr<ThreadPool> pool_;   // host threads for per-stream control-plane work
  std::unique_ptr<AsyncLane> host_lane_;   // the control-plane pass of a decode, beside its GPU work
  int device_ = 0, numa_node_ = -1;
  std::vector<int> host_cpus_;
  hipStream_t stream_ = nullptr, copy_stream_ = nullptr;   // copy_stream_: work-list uploads from the control-plane thread
  Event ev_[4], ev_upload_, ev_fic_, ev_fic_done_, ev_fibs_, ev_part0_, ev_chain_, ev_info_, ev_msc_[4], ev_h2d_[2];
  hipStream_t d2h_stream_ = nullptr;           // eti_fetch_async
  Event ev_eti_fetch_[2];                      // one per outstanding fetch (at most two; no timing)
  std::atomic<uint64_t> eti_fetch_issued_{0}, eti_fetch_waited_{0};   // (issued: the decoding thread; waited: whichever thread waits -- the CLI's writer)
  // page-locked staging ring for uploads from pageable memory: the host pool copies piece n + 1 into one buffer while the DMA of
  // piece n drains another
  static constexpr int kStageBufs = 4;
  PinnedBuffer<uint8_t> stage_buf_[kStageBufs];
  Event stage_ev_[kStageBufs];                 // (no timing)
  bool msc_queued_ = false;
  std::vector<Event> chunk_ev_;

  // constant tables
  DeviceBuffer<double2> d_tw2048_, d_tw1536_;
  DeviceBuffer<uint8_t> d_prs_;
  DeviceBuffer<float2> d_twf_;
  DeviceBuffer<uint16_t> d_qpsk_, d_crc_tab_, d_crc_shift_;
  DeviceBuffer<uint32_t> d_prbs_, d_zero_words_;

  // batch state
  DeviceBuffer<uint8_t> d_iq_own_;
  DeviceBuffer<const uint8_t*> d_iq_ptrs_;
  DeviceBuffer<int64_t> d_nbytes_;
  DeviceBuffer<StreamState> d_states_, d_states_prev_;
  // the streams' tail bytes (device_types.hpp: kTailBytes): carried like the states, the incoming ones kept for a rescan, and one copy per call
  DeviceBuffer<uint8_t> d_tail_state_, d_tail_prev_, d_tail_images_;
  DeviceBuffer<int> d_viol_, d_redo_, d_calls_before_;
  PinnedBuffer<int> h_viol_, h_calls_before_;
  SmallStage h_small_fic_, h_small_msc_;   // staging of upload_small, one per call site
  // the look-ahead schedule of the K1 chain (small batches; k_sync.hip: sync_ahead_kernel): the estimators' table, the predicted start positions, the descriptor base
  DeviceBuffer<int2> d_spec_table_;
  DeviceBuffer<int64_t> d_spec_src0_;
  DeviceBuffer<int> d_spec_ctl_;
  PinnedBuffer<int> h_spec_hits_;
  int spec_mode_ = std::getenv("DABHIP_K1_SPEC") ? (std::atoi(std::getenv("DABHIP_K1_SPEC")) > 0 ? 1 : 0) : -1;
  int sync_rescanned_ = 0;            // streams the split scan had to scan again in full (last decode)
  DeviceBuffer<CallDesc> d_descs_;
  DeviceBuffer<int2> d_info_;
  DeviceBuffer<int2> d_frames_;
  DeviceBuffer<int> d_frame_slot_, d_frame_cif_row_, d_stream_cif_base_;
  DeviceBuffer<float2> d_spectra_;
  DeviceBuffer<uint32_t> d_fic_bits_, d_msc_bits_;
  DeviceBuffer<uint8_t> d_fibs_, d_fib_ok_;
  DeviceBuffer<DecodeJob> d_jobs_;
  DeviceBuffer<WaveGroup> d_groups_;
  DeviceBuffer<int> d_job_ids_;
  DeviceBuffer<CodewordPlan> d_plans_;
  DeviceBuffer<uint4> d_steps_;
  DeviceBuffer<uint32_t> d_grouped_;
  DeviceBuffer<uint2> d_decisions_;
  DeviceBuffer<EtiFrameMeta> d_meta_;
  DeviceBuffer<uint8_t> d_headers_, d_eti_, d_bytes_;
  int tf_slots_ = 0, msc_rows_ = 0;

  std::vector<JobList> stream_jobs_;
  MscWork work_, work_s3_;
  // session state (decode() resets it, feed() continues it)
  std::vector<ControlPlane> planes_;
  bool planes_fresh_ = false;      // a new session started: the planes are reset where they are first used
  PinnedBuffer<StreamState> h_states_;
  PinnedBuffer<int2> h_frames_;
  PinnedBuffer<const uint8_t*> h_ptrs_;
  PinnedBuffer<int64_t> h_nb_;
  PinnedBuffer<int> h_frame_slot_, h_frame_cif_row_;
  std::vector<StreamCarry> carry_;             // segment_layout.hpp: what a segment hands to the next
  // The last decode's layout: its frame list holds the frames whose MSC part ran at [0, seg_.nmsc) and the deferred ones (lock-in skip) behind them, up to
  // seg_.ntf.  pending: their samples, descriptors and the list are still those of that decode, so read_demapped_tf can complete them (in chunks of
  // `chunk` frames, like the decode); deferred = how many there were
  SegmentLayout seg_;
  struct { int chunk = 1, deferred = 0; bool pending = false; } last_;
  std::vector<int> seg_ncalls_, seg_defer_max_;   // layout_segment's per-stream inputs
  std::vector<int> scan_ncalls_;                  // plan_scan's: the complete calls every stream holds
  DeviceBuffer<float> d_delta_;
  DeviceBuffer<uint4> d_guard_list_;
  DeviceBuffer<uint32_t> d_guard_counter_;
  PinnedBuffer<uint32_t> h_guard_counts_;
  int guard_launches_ = 0;
  bool guard_counters_clear_ = false;   // the layout kernel of this decode has cleared the device counters
  uint32_t guard_cap_ = 0, guard_cap_override_ = 0;
  LaunchLimits limits_;
  LaunchReport report_;
  std::vector<uint32_t> guard_caps_;   // per guarded launch of the decode: the list capacity it ran with
  int64_t guard_flagged_ = 0, guard_decisions_ = 0;
  int guard_overflows_ = 0;          // launches of the last decode whose list overflowed (decided again in full, fp64)
  DeviceBuffer<uint8_t> d_carry_;
  DeviceBuffer<CopyDesc> d_copy_descs_;
  HostList<CopyDesc> carry_out_descs_, carry_in_descs_;   // page-locked: they go up without the host waiting for the stream

  PlanTable plan_table_;

  // transmitter identification: rows of kTiiRow words per stream (tii.hpp)
  bool tii_ = false, tii_ran_ = false;
  int tii_rows_ = 0;
  float tii_ms_ = 0;
  Event ev_tii_[2];
  DeviceBuffer<uint32_t> d_tii_nco_;
  DeviceBuffer<unsigned long long> d_tii_sums_, d_tii_stage_sums_;
  DeviceBuffer<CallDesc> d_tii_descs_;
  DeviceBuffer<const uint8_t*> d_tii_ptr_;
  DeviceBuffer<int32_t> d_tii_w0_;
  DeviceBuffer<uint32_t> d_tii_step_;

  PinnedBuffer<CallDesc> h_descs_;
  PinnedBuffer<int2> h_info_;
  PinnedBuffer<uint8_t> h_fibs_, h_fib_ok_;
  ScanPlan scan_;                    // the last scan's schedule (scan_plan.hpp); h_descs_ and h_info_ are [nstreams_][scan_.max_calls]
  int list_max_calls_ = 0;           // descriptor stride of the frame list now on the device (a decode's: scan_.max_calls; a stage entry's: its frames)
  int nstreams_ = 0;
  float scan_setup_ms_ = 0, layout_ms_ = 0;
  std::vector<int64_t> eti_base_, eti_count_;
  std::vector<uint32_t> stream_status_;
  int64_t total_eti_ = 0;
  StageTimes times_;
  int64_t fft_launches_ = 0, fft_tfs_ = 0;
  double fft_ms_ = 0;
};

}  // namespace dabhip
