// engine_scan.cpp — K1 of a decode: the IQ upload and the sync scan (see engine.hpp for the pipeline).
#include "engine_detail.hpp"

namespace dabhip {

// Host-fed decode (the reference's input arrives in host buffers: dab2eti.c:117-130,238).  Streams that live in page-locked memory
// (dabhip_host_alloc, hipHostMalloc / hipHostRegister of the caller's own) go up as plain asynchronous DMA, one copy per stream,
// back to back on the main stream.  Pageable memory cannot be DMA'd from: it is copied into a ring of page-locked staging buffers
// by the engine's host pool (all threads on one piece: a single core's memcpy is slower than the PCIe link) and each piece leaves
// as its own asynchronous copy, so the pool fills one buffer while up to three others drain.  K1 follows in stream order.
bool Engine::upload_iq(const uint8_t* const* iq, const size_t* nbytes, int nstreams, const uint8_t** ptrs)
{
  constexpr size_t kStageBytes = size_t(32) << 20, kPiece = size_t(1) << 20;
  if (!record(ev_h2d_[0], stream_)) return false;
  size_t off = 0;
  int next_buf = 0;
  size_t fill = 0;                             // bytes staged in the current buffer, not yet queued
  size_t fill_dst = 0;                         // device offset the current buffer's bytes go to (streams are laid out back to back)
  auto flush = [&]() -> bool {
    if (fill == 0) return true;
    const bool ok = check(hipMemcpyAsync(d_iq_own_.get() + fill_dst, stage_buf_[next_buf].data(), fill, hipMemcpyHostToDevice, stream_), "IQ upload") &&
                    check(hipEventRecord(stage_ev_[next_buf], stream_), "IQ upload");
    next_buf = (next_buf + 1) % kStageBufs;
    fill = 0;
    return ok;
  };
  for (int b = 0; b < nstreams; ++b) {
    uint8_t* const dst = d_iq_own_.get() + off;
    ptrs[b] = dst;
    const size_t n = nbytes[b], padded = (n + 15) & ~size_t(15);
    // memory the runtime knows (page-locked / registered host memory; also device or managed memory handed in by mistake as "host") is copied
    // by the copy engine directly; everything else is ordinary pageable memory
    hipPointerAttribute_t attr;
    const bool pinned = n && hipPointerGetAttributes(&attr, iq[b]) == hipSuccess &&
                        (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
    if (!pinned) (void)hipGetLastError();      // an unregistered pointer is reported as an error: that is the answer, not a failure
    times_.h2d_bytes += static_cast<double>(n);
    if (pinned) {
      if (!flush()) return false;              // keeps the copies in stream order (cheap: at most one partly filled buffer)
      times_.h2d_pinned_bytes += static_cast<double>(n);
      if (!check(hipMemcpyAsync(dst, iq[b], n, hipMemcpyDefault, stream_), "IQ upload")) return false;
    } else {
      // staged: a stream's bytes continue in the buffer where the previous stream's ended only when they are adjacent on the device
      // (they are, up to the 16-byte padding: a buffer is flushed at a stream boundary when the padding is not zero)
      size_t done = 0;
      while (done < n) {
        if (fill == 0) {
          if (!stage_buf_[next_buf].resize(kStageBytes)) return false;
          if (!check(hipEventSynchronize(stage_ev_[next_buf]), "IQ staging")) return false;   // its previous copy has left (never recorded: returns at once)
          fill_dst = off + done;
        }
        const size_t take = std::min(n - done, kStageBytes - fill);
        const uint8_t* src = iq[b] + done;
        uint8_t* stage = stage_buf_[next_buf].data() + fill;
        const int pieces = static_cast<int>((take + kPiece - 1) / kPiece);
        pool_->parallel_for(pieces, [&](int i) {
          const size_t a = static_cast<size_t>(i) * kPiece;
          std::memcpy(stage + a, src + a, std::min(kPiece, take - a));
        });
        fill += take;
        done += take;
        if (fill == kStageBytes && !flush()) return false;
      }
      if (padded != n && !flush()) return false;
    }
    off += padded;
  }
  if (!flush()) return false;
  if (!record(ev_h2d_[1], stream_)) return false;
  return true;
}

// the argument block of every K1 launch: THE one place that names these buffers (taken afresh before a launch: a reserve may move them)
SyncArgs Engine::sync_args(int nstreams, int max_calls) const
{
  return SyncArgs{d_iq_ptrs_.get(), d_nbytes_.get(), d_states_.get(), d_descs_.get(), d_info_.get(), nstreams, max_calls, d_tw2048_.get(), d_tw1536_.get(), d_prs_.get()};
}

// K1 over the calls that became complete: stages pointers / sizes / states, launches the scan, brings back {status, ordinal}
// per call and the front-end states (main stream, awaited) and the full descriptors (side stream, awaited by the caller's guard)
bool Engine::scan_streams(const uint8_t* const* iq, bool on_device, bool full_scan, DecodeRun& run)
{
  const int nstreams = run.nstreams;
  if (!scan_begin(iq, on_device, full_scan, run)) return false;
  const ScanPlan& p = scan_;
  sync_rescanned_ = 0;
  if (!record(ev_[0], stream_)) return false;
  if (!p.split) {
    // the reference's order, call after call: with the software AFC every call's NCO depends on the estimates of the call
    // before; and the fallback when the split scan's assumption failed
    SyncScanOpts o;
    o.afc = afc_ ? 1 : 0;
    o.tails = SyncTails{d_tail_state_.get(), d_tail_state_.get(), d_tail_images_.get(), kChunkBytes};
    if (!check(launch_sync_scan(sync_args(nstreams, p.max_calls), o, stream_), "sync scan launch")) return false;
  } else if (!scan_chain(run.cont)) {
    return false;
  }
  if (!record(ev_[1], stream_)) return false;
  // The host only needs {status, ordinal} of every call to lay the frames out: K1 writes those 8 bytes per call to a
  // compact array that comes back first; the full descriptors (trace API) follow on the side stream.
  if (p.split && (!check(hipEventSynchronize(ev_info_), "call info") || !layout_and_a(run))) return false;
  if (!scan_fetch()) return false;
  if (!p.split && !layout_and_a(run)) return false;
  if (p.split && !scan_again(run)) return false;
  if (!check(hipStreamWaitEvent(copy_stream_, ev_[1], 0), "desc download") ||
      !check(hipMemcpyAsync(h_descs_.data(), d_descs_.get(), p.ndesc * sizeof(CallDesc), hipMemcpyDeviceToHost, copy_stream_), "desc download"))
    return false;
  if (!elapsed(&times_.sync, ev_[0], ev_[1])) return false;
  for (int b = 0; b < nstreams; ++b)
    if (h_states_[b].overflow) { set_error("sync scan: stale-tail bookkeeping overflow (more than kMaxSeg nested short reads)"); return false; }
  return true;
}

// the streams' pointers, sizes and states staged, the scan planned (scan_), its buffers reserved, and the device side prepared in one launch
bool Engine::scan_begin(const uint8_t* const* iq, bool on_device, bool full_scan, const DecodeRun& run)
{
  const auto wall0 = std::chrono::steady_clock::now();
  const int nstreams = run.nstreams;
  if (!h_ptrs_.resize(nstreams) || !h_nb_.resize(nstreams) || !h_calls_before_.resize(nstreams)) return false;   // page-locked staging: asynchronous uploads
  const uint8_t** const ptrs = h_ptrs_.data();
  scan_ncalls_.resize(nstreams);
  size_t total = 0;
  for (int b = 0; b < nstreams; ++b) {
    h_nb_[b] = static_cast<int64_t>(run.nbytes[b]);
    scan_ncalls_[b] = static_cast<int>(run.nbytes[b] / kChunkBytes);
    h_calls_before_[b] = carry_[b].calls_done;
    total += (run.nbytes[b] + 15) & ~size_t(15);
  }
  static const ScanKnobs knobs = ScanKnobs::from_env();
  const ScanPlan p = plan_scan(nstreams, scan_ncalls_.data(), h_calls_before_.data(), afc_, full_scan, run.cont, spec_mode_, knobs);
  if (!h_descs_.resize(p.ndesc) || !h_info_.resize(p.ndesc)) return false;
  scan_ = p;                                               // (trace()'s stride: set with the array it indexes)
  if (on_device) {
    for (int b = 0; b < nstreams; ++b) ptrs[b] = iq[b];
  } else {
    if (!d_iq_own_.reserve(total) || !upload_iq(iq, run.nbytes, nstreams, ptrs)) return false;
  }
  if (!h_states_.resize(nstreams)) return false;
  StreamState* const states = h_states_.data();
  if (!run.cont) std::fill(states, states + nstreams, initial_state());
  static_assert(sizeof(CallDesc) % 16 == 0, "cleared in 16-byte pieces");
  if (!d_states_.reserve(nstreams) || !d_iq_ptrs_.reserve(nstreams) || !d_nbytes_.reserve(nstreams) || !d_descs_.reserve(p.ndesc) || !d_info_.reserve(p.ndesc + 1)) return false;
  if (!d_tail_state_.reserve(static_cast<size_t>(nstreams) * kTailBytes) || !d_tail_images_.reserve(p.ndesc * kTailBytes) ||
      (p.split && !d_tail_prev_.reserve(static_cast<size_t>(nstreams) * kTailBytes)))
    return false;
  if (p.ahead && (!d_spec_table_.reserve(static_cast<size_t>(nstreams) * p.nspec * p.nhyp) || !d_spec_src0_.reserve(static_cast<size_t>(nstreams) * p.nspec) ||
                  !d_spec_ctl_.reserve(nstreams + 1) || !h_spec_hits_.resize(1)))
    return false;
  // d_viol_[0 .. nstreams): first call of a stream that broke the chain's assumption; [nstreams]: calls the fp32 pass of the
  // verification left to the fp64 pass
  if (p.split && (!h_viol_.resize(nstreams + 1) || !d_viol_.reserve(nstreams + 1) || !d_states_prev_.reserve(nstreams) || !d_calls_before_.reserve(nstreams))) return false;
  // one launch instead of nine copies and fills (launch_scan_setup): the kernel reads the page-locked host arrays itself
  ScanSetupArgs a{};
  a.h_states = run.cont ? nullptr : states;
  a.h_ptrs = ptrs;
  a.h_nbytes = h_nb_.data();
  a.h_calls_before = p.split ? h_calls_before_.data() : nullptr;
  a.states = d_states_.get();
  a.states_prev = p.split ? d_states_prev_.get() : nullptr;
  a.iq_ptrs = d_iq_ptrs_.get();
  a.nbytes = d_nbytes_.get();
  a.calls_before = p.split ? d_calls_before_.get() : nullptr;
  a.viol = p.split ? d_viol_.get() : nullptr;
  a.descs = reinterpret_cast<uint4*>(d_descs_.get());
  a.desc_vec = p.ndesc * (sizeof(CallDesc) / 16);
  a.info = reinterpret_cast<uint4*>(d_info_.get());
  a.info_vec = (p.ndesc + 1) / 2;
  a.nstreams = nstreams;
  a.tail_state = d_tail_state_.get();
  a.tail_state_prev = p.split ? d_tail_prev_.get() : nullptr;
  if (!check(launch_scan_setup(a, stream_), "scan setup launch")) return false;
  scan_setup_ms_ = ms_since(wall0);
  return true;
}

// Split scan: the per-stream chain carries only what the next call depends on (FIFO, coarse and fine time) and assumes the
// coarse frequency offset of every frame within +-1 carrier (input_sdr.c:105-109: otherwise the frame is dropped and a
// resync forced); both frequency estimates are then computed for all frames in parallel (sync_verify_kernel).  A stream that
// breaks the assumption (a capture more than a carrier off tune, noise) is scanned again from its incoming state in the
// reference's order, so the result is the same in every case.  (Tried and dropped: the verification on a second stream beside
// the OFDM stage, and -- after the LDS bank conflicts were gone -- the chain in 2..16 chunks of calls with each chunk's
// verification beside the next chunk: 1.28 -> 1.30..1.40 ms.  A chain workgroup holds half of a CU's LDS, so the verification
// beside it runs at half its rate and slows the chain.  Round 3, with the fp32 verification (39.5 KB of LDS, 54 VGPRs): on its own stream beside the FIC
// symbols' OFDM launch -- step unchanged, 10.4 ms: both are issue-bound, the work only moves.)
bool Engine::scan_chain(bool cont)
{
  const ScanPlan& p = scan_;
  const SyncArgs a = sync_args(nstreams_, p.max_calls);
  SyncScanOpts o;
  o.chain_only = true;
  o.tails = SyncTails{d_tail_state_.get(), d_tail_state_.get(), d_tail_images_.get(), kChunkBytes};
  auto chain = [&]() { return check(launch_sync_scan(a, o, stream_), "sync chain launch"); };
  if (p.ahead) {
    // a short chain to lock on (scan_plan.hpp: first_limit), then passes over all remaining calls at once, each followed by the chain launch that looks
    // its calls up (a long stream: several passes, each predicting from where the chain really got to)
    SpecArgs& sp = o.spec;
    sp.table = d_spec_table_.get();
    sp.src0 = d_spec_src0_.get();
    sp.ctl = d_spec_ctl_.get();
    sp.nspec = p.nspec;
    sp.nstreams = nstreams_;
    sp.nhyp = p.nhyp;
    sp.call_limit = p.first_limit;
    sp.record_base = 1;
    if (!chain()) return false;
    sp.record_base = 0;
    sp.lookup = 1;
    for (int r = 0; r < p.passes; ++r) {
      sp.call_limit = p.pass_limit(r);
      if (!check(launch_sync_ahead(a, sp, stream_), "sync look-ahead launch") || !chain()) return false;
    }
  } else if (!chain()) {
    return false;
  }
  // {status, ordinal} of every call are final once the chain is through (a stream that breaks its assumption is scanned again
  // later): they come back on the side stream while the verification runs, and the caller lays the frames out beside it
  return check(hipEventRecord(ev_chain_, stream_), "chain event") && check(hipStreamWaitEvent(copy_stream_, ev_chain_, 0), "chain event") &&
         check(hipMemcpyAsync(h_info_.data(), d_info_.get(), p.ndesc * sizeof(int2), hipMemcpyDeviceToHost, copy_stream_), "call info download") &&
         check(hipEventRecord(ev_info_, copy_stream_), "call info event") &&
         check(launch_sync_verify(a, d_calls_before_.get(), d_viol_.get(), false, stream_), "sync verify launch") &&
         // fine_freq_shift carried through the calls that did not demodulate (the kernel skips streams with a violation)
         check(launch_sync_verify(a, d_calls_before_.get(), d_viol_.get(), true, stream_), "sync carry launch");
  // (the violation marks come back on the side stream, in scan_fetch: a copy on the main stream sits between K1 and the first OFDM launch)
}

// What the host needs of the scan, awaited: violation marks and look-ahead hits (split scan), {status, ordinal} of every call, the front-end states.
// (on the side stream, behind the scan's last kernel: what the layout may have queued on the main stream meanwhile -- the
// first OFDM launch -- is not waited for)
bool Engine::scan_fetch()
{
  const ScanPlan& p = scan_;
  const int nstreams = nstreams_;
  StreamState* const states = h_states_.data();
  // Small scans: the four downloads as ONE kernel that writes the page-locked host arrays itself (launch_host_words works in either direction: both
  // sides are addresses the device can reach) instead of four copy-engine commands in a row, each some microseconds of the host waiting.
  ++report_.fetches;
  report_.fetch_form = p.result_words <= static_cast<size_t>(limits_.fetch_words) ? kFetchKernel : kFetchCopyEngine;
  if (report_.fetch_form == kFetchKernel) {
    HostWordsArgs hw{};
    int k = 0;
    auto add = [&](const void* src, void* dst, size_t n) { hw.set(k++, src, dst, n); };
    if (p.split) add(d_viol_.get(), h_viol_.data(), nstreams + 1);
    if (p.ahead) add(d_spec_ctl_.get() + nstreams, h_spec_hits_.data(), 1);
    add(d_info_.get(), h_info_.data(), p.ndesc * 2);
    add(d_states_.get(), states, static_cast<size_t>(nstreams) * (sizeof(StreamState) / 4));
    return check(hipStreamWaitEvent(copy_stream_, ev_[1], 0), "scan event") && check(launch_host_words(hw, copy_stream_), "scan results download") &&
           check(hipStreamSynchronize(copy_stream_), "sync scan");
  }
  return check(hipStreamWaitEvent(copy_stream_, ev_[1], 0), "scan event") &&
         (!p.split || check(hipMemcpyAsync(h_viol_.data(), d_viol_.get(), (nstreams + 1) * sizeof(int), hipMemcpyDeviceToHost, copy_stream_), "violation download")) &&
         (!p.ahead || check(hipMemcpyAsync(h_spec_hits_.data(), d_spec_ctl_.get() + nstreams, sizeof(int), hipMemcpyDeviceToHost, copy_stream_), "look-ahead hits download")) &&
         check(hipMemcpyAsync(h_info_.data(), d_info_.get(), p.ndesc * sizeof(int2), hipMemcpyDeviceToHost, copy_stream_), "call info download") &&
         check(hipMemcpyAsync(states, d_states_.get(), nstreams * sizeof(StreamState), hipMemcpyDeviceToHost, copy_stream_), "state download") &&
         check(hipStreamSynchronize(copy_stream_), "sync scan");
}

// behind the split scan's fetch: the streams that broke the chain's assumption again, in the reference's order, from their incoming state (rare)
bool Engine::scan_again(DecodeRun& run)
{
  const int nstreams = nstreams_;
  std::vector<int> redo;
  for (int b = 0; b < nstreams; ++b)
    if (h_viol_[b] != 0x7f7f7f7f) redo.push_back(b);
  sync_rescanned_ = static_cast<int>(redo.size());
  times_.sync_fp64_calls = static_cast<float>(h_viol_[nstreams]);
  times_.sync_spec_calls = scan_.ahead ? static_cast<float>(h_spec_hits_[0]) : 0.0f;
  if (redo.empty()) return true;
  // (what the first layout queued -- its set-up kernel reads the page-locked frame lists when it RUNS -- is through before the lists are rewritten)
  // (the guarded launches of the first layout have run; they are made again for the new frame list: their counters and counts start over --
  // the second layout's set-up kernel clears the device side again)
  guard_new_run();
  SyncScanOpts o;
  o.states_in = d_states_prev_.get();
  o.tails = SyncTails{d_tail_prev_.get(), d_tail_state_.get(), d_tail_images_.get(), kChunkBytes};
  if (!check(hipStreamSynchronize(stream_), "before the rescan") || !d_redo_.upload(redo, stream_)) return false;
  o.stream_list = d_redo_.get();
  return check(launch_sync_scan(sync_args(sync_rescanned_, scan_.max_calls), o, stream_), "sync rescan launch") && record(ev_[1], stream_) && scan_fetch() &&
         layout_and_a(run);                                // the frames of those streams may have changed
}

}  // namespace dabhip
