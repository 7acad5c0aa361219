// edirx.cpp — dabhip_edirx: the stateful consumer of EDI packets that gives ETI frames back (dabhip.h).  Each push or flush runs the kernels of
// k_edirx.hip on its own HIP stream over the packets where they lie (device) or after one upload (host); between calls it keeps every
// stream's window and the bytes of its open groups on the device.  The frames, their records and the counters stay there until asked for.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "edirx.hpp"
#include "stage_frame.hpp"

using namespace dabhip;

static_assert(sizeof(dabhip_edirx_rec) == 32, "dabhip_edirx_rec layout");
static_assert(DABHIP_EDIRX_COUNTERS == kEdirxCntN, "the counters of dabhip.h");

namespace {
constexpr int kNStages = 7;
const char* const kStages[kNStages] = {"parse", "window", "gather", "rs", "frame", "emit", "carry"};
}  // namespace

struct dabhip_edirx {
  int nstreams = 0, depth = 0;
  DeviceBuffer<EdirxStream> state;
  DeviceBuffer<int64_t> counters, sums, bases, off;
  DeviceBuffer<uint8_t> gf, carry, staging, work, ers, candframes, out;
  DeviceBuffer<int32_t> info, fin, joined, list, nlist, rsfail, outmap, nframes;
  DeviceBuffer<EdirxHdr> hdr;
  DeviceBuffer<EdirxMeta> meta;
  DeviceBuffer<EdirxCand> cands;
  DeviceBuffer<EdirxVerdict> verdict;
  DeviceBuffer<dabhip_edirx_rec> recs;
  std::vector<int64_t> h_bases;                          // of the last call: groups touched and candidates in front of every stream, the totals last
  std::vector<int32_t> h_nframes;
  StageFrame<kNStages> f{"edirx", kStages};

  bool stream_ok(int s) const
  {
    if (s < 0 || s >= nstreams) { set_error("edirx: no such stream"); return false; }
    return true;
  }
  int64_t run(const uint8_t* data, const int32_t* lengths, const int64_t* counts, int on_device, int flush);
};

int64_t dabhip_edirx::run(const uint8_t* data, const int32_t* lengths, const int64_t* counts, int on_device, int flush)
{
  const auto ok = [this](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!f.use_device()) return -1;
  const int ns = nstreams;
  std::vector<int32_t> hinfo(2 * static_cast<size_t>(ns), 0);
  int64_t total = 0;
  for (int s = 0; counts && s < ns; ++s) {
    if (counts[s] < 0 || counts[s] > kEdirxMaxPushPackets) { set_error("edirx_push: bad packet count"); return -1; }
    hinfo[s] = static_cast<int32_t>(total);
    hinfo[ns + s] = static_cast<int32_t>(counts[s]);
    total += counts[s];
    if (total > kEdirxMaxPushPackets) { set_error("edirx_push: too many packets for one push"); return -1; }
  }
  if (total > 0 && (!data || !lengths)) { set_error("edirx_push: null argument"); return -1; }
  std::vector<int64_t> hoff(static_cast<size_t>(total) + 1, 0);
  for (int64_t i = 0; i < total; ++i) {
    if (lengths[i] < 0) { set_error("edirx_push: bad packet length"); return -1; }
    hoff[i + 1] = hoff[i] + lengths[i];
  }
  const int64_t nbytes = hoff[total];
  if (nbytes > 0x7FFFFFFF) { set_error("edirx_push: too many bytes for one push"); return -1; }
  std::fill(h_bases.begin(), h_bases.end(), 0);
  std::fill(h_nframes.begin(), h_nframes.end(), 0);
  const uint8_t* src = data;
  if (nbytes > 0 && !on_device) {
    if (!staging.reserve(static_cast<size_t>(nbytes)) || !ok(hipMemcpyAsync(staging.get(), data, static_cast<size_t>(nbytes), hipMemcpyHostToDevice, f.stream), "upload")) return -1;
    src = staging.get();
  }
  const size_t slots = static_cast<size_t>(total) + static_cast<size_t>(ns) * depth;
  const size_t np1 = static_cast<size_t>(std::max<int64_t>(total, 1));
  if (!info.reserve(hinfo.size()) || !off.reserve(hoff.size()) || !hdr.reserve(np1) || !joined.reserve(np1) || !meta.reserve(slots) || !fin.reserve(slots)) return -1;
  // the host copies must outlive the asynchronous copies: the stream is drained below, before they go
  if (!ok(hipMemcpyAsync(info.get(), hinfo.data(), sizeof(int32_t) * hinfo.size(), hipMemcpyHostToDevice, f.stream), "upload") ||
      !ok(hipMemcpyAsync(off.get(), hoff.data(), sizeof(int64_t) * hoff.size(), hipMemcpyHostToDevice, f.stream), "upload"))
    return -1;
  EdirxPush p = {src, off.get(), info.get(), info.get() + ns, ns, depth, static_cast<int>(total), flush};
  hipStream_t st = f.stream;
  std::vector<int64_t> hb(h_bases.size(), 0);
  bool good = f.mark(0) && ok(launch_edirx_parse(p, hdr.get(), st), "parse") && f.mark(1) &&
              ok(launch_edirx_window(p, hdr.get(), state.get(), counters.get(), meta.get(), fin.get(), joined.get(), sums.get(), bases.get(), st), "window") && f.mark(2) &&
              ok(hipMemcpyAsync(hb.data(), bases.get(), sizeof(int64_t) * hb.size(), hipMemcpyDeviceToHost, st), "totals") && ok(hipStreamSynchronize(st), "window stage");
  if (!good) return -1;
  const int64_t ntouched = hb[2 * static_cast<size_t>(ns)], ncand = hb[2 * static_cast<size_t>(ns) + 1];
  const size_t nt1 = static_cast<size_t>(std::max<int64_t>(ntouched, 1)), nc1 = static_cast<size_t>(std::max<int64_t>(ncand, 1));
  good = work.reserve(nt1 * kEdirxStride) && cands.reserve(nc1) && ers.reserve(nc1 * kEdirxMaxWords) && list.reserve(nc1 * kEdirxMaxWords) && rsfail.reserve(nc1) &&
         verdict.reserve(nc1) && candframes.reserve(nc1 * DABHIP_ETI_BYTES) && out.reserve(nc1 * DABHIP_ETI_BYTES) && recs.reserve(nc1) && outmap.reserve(nc1) &&
         ok(launch_edirx_gather(p, ntouched, hdr.get(), meta.get(), joined.get(), bases.get(), carry.get(), work.get(), st), "gather") && f.mark(3) &&
         ok(launch_edirx_rs(p, ncand, meta.get(), fin.get(), bases.get(), gf.get(), cands.get(), ers.get(), list.get(), nlist.get(), rsfail.get(), work.get(), st), "rs") &&
         f.mark(4) && ok(launch_edirx_frame(ncand, meta.get(), cands.get(), ers.get(), rsfail.get(), work.get(), candframes.get(), verdict.get(), st), "frame") && f.mark(5) &&
         ok(launch_edirx_emit(p, ncand, meta.get(), cands.get(), verdict.get(), bases.get(), candframes.get(), counters.get(), outmap.get(), nframes.get(), recs.get(),
                              out.get(), st), "emit") &&
         f.mark(6) && ok(launch_edirx_carry(p, ntouched, meta.get(), bases.get(), work.get(), carry.get(), st), "carry") && f.mark(7) &&
         ok(hipMemcpyAsync(h_nframes.data(), nframes.get(), sizeof(int32_t) * static_cast<size_t>(ns), hipMemcpyDeviceToHost, st), "frame counts") && f.finish();
  if (!good) {
    std::fill(h_nframes.begin(), h_nframes.end(), 0);
    return -1;
  }
  h_bases = hb;
  int64_t frames = 0;
  for (int32_t n : h_nframes) frames += n;
  return frames;
}

extern "C" dabhip_edirx* dabhip_edirx_create(int device, int nstreams, int depth)
{
  std::unique_ptr<dabhip_edirx> d(new dabhip_edirx);
  StageFrame<kNStages>& f = d->f;
  if (!f.open(device, "no HIP device: the EDI receiving stage runs on the GPU only", "edirx_create: device index out of range")) return nullptr;
  if (nstreams <= 0 || nstreams > (1 << 16) || depth < 1 || depth > kEdirxMaxDepth) { set_error("edirx_create: bad arguments"); return nullptr; }
  d->nstreams = nstreams;
  d->depth = depth;
  const size_t ns = static_cast<size_t>(nstreams);
  std::vector<uint8_t> gf(768);
  edirx_gf_fill(gf.data(), gf.data() + 512);
  d->h_bases.assign(2 * ns + 2, 0);
  d->h_nframes.assign(ns, 0);
  const bool good = d->state.reserve(ns) && d->counters.reserve(ns * kEdirxCntN) && d->sums.reserve(2 * ns) && d->bases.reserve(2 * ns + 2) && d->gf.reserve(gf.size()) &&
                    d->nlist.reserve(1) && d->nframes.reserve(ns) && d->carry.reserve(ns * depth * kEdirxStride) &&
                    f.ok(hipMemset(d->state.get(), 0, sizeof(EdirxStream) * ns), "clear") && f.ok(hipMemset(d->counters.get(), 0, sizeof(int64_t) * ns * kEdirxCntN), "clear") &&
                    f.ok(hipMemcpy(d->gf.get(), gf.data(), gf.size(), hipMemcpyHostToDevice), "upload");
  return good ? d.release() : nullptr;
}

extern "C" void dabhip_edirx_destroy(dabhip_edirx* d) { delete d; }

extern "C" int64_t dabhip_edirx_push(dabhip_edirx* d, const uint8_t* data, const int32_t* lengths, const int64_t* counts, int on_device)
{
  if (!d || !counts) { set_error("edirx_push: null argument"); return -1; }
  return d->run(data, lengths, counts, on_device, -2);
}

extern "C" int64_t dabhip_edirx_flush(dabhip_edirx* d, int stream)
{
  if (!d) { set_error("edirx_flush: null argument"); return -1; }
  if (stream != -1 && !d->stream_ok(stream)) return -1;
  return d->run(nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int64_t dabhip_edirx_records(const dabhip_edirx* d, int stream, dabhip_edirx_rec* out, int64_t cap)
{
  if (!d) { set_error("edirx_records: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  const int64_t a = d->h_bases[2 * static_cast<size_t>(stream) + 1], n = d->h_nframes[static_cast<size_t>(stream)];
  const int64_t take = out ? std::min(n, std::max<int64_t>(cap, 0)) : 0;
  if (take > 0 && !d->f.ok(blocking_copy(out, d->recs.get() + a, sizeof(dabhip_edirx_rec) * static_cast<size_t>(take), hipMemcpyDeviceToHost), "records")) return -1;
  return n;
}

extern "C" int64_t dabhip_edirx_frames(const dabhip_edirx* d, int stream, uint8_t* dst, int64_t cap)
{
  if (!d) { set_error("edirx_frames: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  const int64_t a = d->h_bases[2 * static_cast<size_t>(stream) + 1], n = d->h_nframes[static_cast<size_t>(stream)];
  const int64_t take = dst ? std::min(n, std::max<int64_t>(cap, 0) / DABHIP_ETI_BYTES) : 0;
  if (take > 0 && !d->f.ok(blocking_copy(dst, d->out.get() + a * DABHIP_ETI_BYTES, static_cast<size_t>(take) * DABHIP_ETI_BYTES, hipMemcpyDeviceToHost), "frames")) return -1;
  return n;
}

extern "C" int dabhip_edirx_reset(dabhip_edirx* d, int stream)
{
  if (!d) { set_error("edirx_reset: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  // the counters (and with them the frame numbers) go on; the window and its open groups return to nothing
  return d->f.ok(hipMemset(d->state.get() + stream, 0, sizeof(EdirxStream)), "reset") ? 0 : -1;
}

extern "C" int dabhip_edirx_stats(const dabhip_edirx* d, int stream, int64_t* counters, int cap)
{
  if (!d || !counters) { set_error("edirx_stats: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  const int n = std::min(std::max(cap, 0), static_cast<int>(kEdirxCntN));
  if (n > 0 && !d->f.ok(blocking_copy(counters, d->counters.get() + static_cast<size_t>(stream) * kEdirxCntN, sizeof(int64_t) * n, hipMemcpyDeviceToHost), "counters")) return -1;
  return n;
}

extern "C" int dabhip_edirx_stage_ms(const dabhip_edirx* d, const char** names, float* ms, int cap)
{
  if (!d) return -1;
  return d->f.stage_ms(names, ms, cap);
}
