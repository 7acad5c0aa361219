// stage_frame.hpp — what the handle of a side stage is made of besides its own buffers: the device, a non-blocking stream of its own, the events
// around its N timed stages and their times.  The stages of raw samples (dabhip_ingest, dabhip_scan), of ETI frames (dabhip_dabplus,
// dabhip_packet, dabhip_ts, dabhip_dir, dabhip_edi) and of EDI packets (dabhip_edirx) all have one; the first two kinds also take their push's
// host-side plan (sample_push.hpp, eti_push.hpp) to the device here.  A handle declares its frame LAST, so that the frame goes first: the stream
// is idle and gone before the buffers are freed.
#pragma once

#include <algorithm>
#include <utility>

#include "../../include/dabhip.h"
#include "eti_push.hpp"
#include "hip_util.hpp"
#include "sample_push.hpp"

namespace dabhip {

template <int N>
struct StageFrame {
  const char* const prefix;                        // in front of every HIP error: "ingest", "scan", "dabplus", ...
  const char* const* const names;                  // the N stages
  int device = 0;
  hipStream_t stream = nullptr;
  Event ev[N + 1];                                 // stage k lies between ev[k] and ev[k + 1]
  float ms[N] = {};

  StageFrame(const char* prefix_, const char* const (&names_)[N]) : prefix(prefix_), names(names_) {}
  StageFrame(const StageFrame&) = delete;
  ~StageFrame()
  {
    if (!stream) return;                           // (events exist only behind a stream)
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
    for (Event& e : ev) Event(std::move(e));       // destroyed here, before the stream
    (void)hipStreamDestroy(stream);
  }

  bool ok(hipError_t e, const char* what) const
  {
    if (e == hipSuccess) return true;
    set_error(std::string(prefix) + ": " + what + ": " + hipGetErrorString(e));
    return false;
  }
  // no_device: the whole text where there is no GPU; bad_index: a text of its own for a device index out of range (else hipSetDevice's)
  bool open(int dev, const std::string& no_device, const char* bad_index = nullptr)
  {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); set_error(no_device); return false; }
    if (bad_index && (dev < 0 || dev >= ndev)) { set_error(bad_index); return false; }
    if (!ok(hipSetDevice(dev), "hipSetDevice")) return false;
    device = dev;
    bool good = ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
    for (Event& e : ev) good = good && ok(e.create(), "hipEventCreate");
    return good;
  }
  bool use_device() const { return ok(hipSetDevice(device), "hipSetDevice"); }
  bool mark(int k) { return ok(hipEventRecord(ev[k], stream), "event"); }
  // the end of a push: the stream drained, then the stages' times
  bool finish()
  {
    if (!ok(hipStreamSynchronize(stream), "push")) return false;
    for (int k = 0; k < N; ++k)
      if (!ok(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]), "hipEventElapsedTime")) return false;
    return true;
  }
  // the *_stage_ms entries: at most cap of the N (name, time) pairs, into the arrays that are there; returns min(cap, N)
  int stage_ms(const char** names_out, float* ms_out, int cap) const
  {
    const int n = std::min(cap, N);
    for (int k = 0; k < n; ++k) {
      if (names_out) names_out[k] = names[k];
      if (ms_out) ms_out[k] = ms[k];
    }
    return n;
  }
  // the host path of a sample push (sample_push.hpp): ev[0], then every stream's bytes to its place in `stage`.  dev[b]: where stream b lies then
  bool upload(DeviceBuffer<uint8_t>& stage, const SamplePush& p, const void* const* src, std::vector<const void*>& dev)
  {
    if (!stage.reserve(p.stage_total ? p.stage_total : 1) || !mark(0)) return false;
    for (size_t b = 0; b < dev.size(); ++b) {
      dev[b] = stage.get() + p.offset[b];
      if (p.upload[b] && !ok(hipMemcpyAsync(stage.get() + p.offset[b], src[b], p.upload[b], hipMemcpyHostToDevice, stream), "upload")) return false;
    }
    return true;
  }
  // the device side of a push of ETI frames (eti_push.hpp): the host frames to `staging`, unless they lie on the device already, and the plan's
  // block to `meta`.  fr: the frames as the kernels take them; ncarry: where the block's third column lies (DAB+)
  bool place(const EtiPush& p, const uint8_t* frames, int on_device, DeviceBuffer<uint8_t>& staging, DeviceBuffer<uint8_t>& meta, EtiFrames& fr, const int** ncarry = nullptr)
  {
    fr.frames = frames;
    if (p.total > 0 && !on_device) {
      const size_t bytes = static_cast<size_t>(p.total) * DABHIP_ETI_BYTES;
      if (!staging.reserve(bytes) || !ok(hipMemcpyAsync(staging.get(), frames, bytes, hipMemcpyHostToDevice, stream), "upload")) return false;
      fr.frames = staging.get();
    }
    // the plan must outlive the asynchronous copy of its block: hipMemcpy from pageable memory returns once the bytes are staged
    if (!meta.reserve(p.meta.size()) || !ok(hipMemcpyAsync(meta.get(), p.meta.data(), p.meta.size(), hipMemcpyHostToDevice, stream), "upload") ||
        !ok(hipStreamSynchronize(stream), "upload"))
      return false;
    const size_t ns = static_cast<size_t>(p.nstreams);
    fr.base = reinterpret_cast<const int64_t*>(meta.get());
    fr.nnew = reinterpret_cast<const int*>(meta.get() + 8 * ns);
    if (ncarry) *ncarry = p.carries ? reinterpret_cast<const int*>(meta.get() + 12 * ns) : nullptr;
    return true;
  }
};

}  // namespace dabhip
