// scan.cpp — the block scan's host object (include/dabhip.h: dabhip_scan): per stream the positions, the carried samples of an unfinished segment and
// the spectrum; per push the plan (scan_blocks.hpp), the uploads and one launch of k_scan.hip's transform for all streams.  Every push ends in a
// stream synchronise (engine.hpp: what the runtime keeps of a stream that nobody synchronises).
#include <new>
#include <string>
#include <vector>

#include "capi_detail.hpp"
#include "engine.hpp"
#include "ingest_plan.hpp"
#include "scan.hpp"
#include "scan_blocks.hpp"

using namespace dabhip;

struct dabhip_scan {
  int device = 0, nstreams = 0, format = 0, sample_bytes = 0, nsegments = 0;
  int64_t rate = 0;
  std::vector<ScanStreamState> st;
  DeviceBuffer<uint32_t> nco;
  DeviceBuffer<uint8_t> carry[2], stage;
  DeviceBuffer<ScanDesc> descs;
  DeviceBuffer<unsigned long long> power;          // nstreams spectra of 4096 bins
  size_t carry_stride = 0;
  int cur = 0;                                     // carry[cur] holds what the last push kept
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {};
  float ms[3] = {0, 0, 0};
  ~dabhip_scan()
  {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {
bool ok(hipError_t e, const char* what)
{
  if (e == hipSuccess) return true;
  set_error(std::string("scan: ") + what + ": " + hipGetErrorString(e));
  return false;
}
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the push proper: nsamples[b] samples of stream b at src[b] (device memory, aligned to a sample).  Returns the segments accumulated, < 0 on error.
int64_t push_device(dabhip_scan* d, const std::vector<const void*>& src, const std::vector<int64_t>& nsamples, bool uploaded)
{
  const int ns = d->nstreams;
  std::vector<ScanStreamState> next = d->st;
  std::vector<ScanDesc> h(static_cast<size_t>(ns));
  int64_t max_nseg = 0, max_keep = 0, total = 0;
  for (int b = 0; b < ns; ++b) {
    const ScanPush p = scan_plan_push(d->nsegments, next[static_cast<size_t>(b)], nsamples[static_cast<size_t>(b)]);
    if (static_cast<size_t>(p.keep) * d->sample_bytes > d->carry_stride) { set_error("scan_push: internal: the carry outgrew its buffer"); return -1; }
    ScanDesc& x = h[static_cast<size_t>(b)];
    x.carry = d->carry[d->cur].get() + static_cast<size_t>(b) * d->carry_stride;
    x.keep = d->carry[d->cur ^ 1].get() + static_cast<size_t>(b) * d->carry_stride;
    x.src = src[static_cast<size_t>(b)];
    x.power = d->power.get() + static_cast<size_t>(b) * kScanSize;
    x.carry_from = p.carry_from;
    x.new_from = p.new_from;
    x.end = p.end;
    x.first_seg = p.first_seg;
    x.keep_from = p.keep_from;
    x.nseg = static_cast<int32_t>(p.nseg);
    x.pad = 0;
    max_nseg = std::max(max_nseg, p.nseg);
    max_keep = std::max(max_keep, p.keep);
    total += p.nseg;
  }
  hipStream_t st = d->stream;
  if (!d->descs.reserve(h.size())) return -1;
  if (!uploaded && !ok(hipEventRecord(d->ev[0], st), "event")) return -1;
  if (!ok(hipEventRecord(d->ev[1], st), "event") || !ok(hipMemcpyAsync(d->descs.get(), h.data(), h.size() * sizeof(ScanDesc), hipMemcpyHostToDevice, st), "descriptors") ||
      !ok(launch_scan_transform(d->format, d->descs.get(), ns, max_nseg, d->nco.get(), st), "transform launch") || !ok(hipEventRecord(d->ev[2], st), "event") ||
      !ok(launch_scan_keep(d->format, d->descs.get(), ns, max_keep, st), "keep launch") || !ok(hipEventRecord(d->ev[3], st), "event") || !ok(hipStreamSynchronize(st), "push"))
    return -1;
  for (int k = 0; k < 3; ++k)
    if (!ok(hipEventElapsedTime(&d->ms[k], d->ev[k], d->ev[k + 1]), "hipEventElapsedTime")) return -1;
  d->st = next;
  d->cur ^= 1;
  return total;
}
}  // namespace

extern "C" dabhip_scan* dabhip_scan_create(int device, int nstreams, int format, int64_t rate_hz, int nsegments)
{
  const std::string why = scan_check(nstreams, format, rate_hz, nsegments);
  if (!why.empty()) { set_error("scan_create: " + why); return nullptr; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); set_error("scan_create: no HIP device"); return nullptr; }
  if (!ok(hipSetDevice(device), "hipSetDevice")) return nullptr;
  dabhip_scan* d = new (std::nothrow) dabhip_scan;
  if (!d) return nullptr;
  d->device = device;
  d->nstreams = nstreams;
  d->format = format;
  d->sample_bytes = ingest_sample_bytes(format);
  d->rate = rate_hz;
  d->nsegments = nsegments;
  d->st.assign(static_cast<size_t>(nstreams), ScanStreamState{});
  d->carry_stride = static_cast<size_t>(kScanSize) * d->sample_bytes;      // at most 4095 samples are carried
  const std::vector<int16_t> cs = ingest_tune_nco();
  std::vector<uint32_t> nco;
  for (int i = 0; i < kTuneNcoSize; ++i) nco.push_back(static_cast<uint16_t>(cs[static_cast<size_t>(2 * i)]) | static_cast<uint32_t>(static_cast<uint16_t>(cs[static_cast<size_t>(2 * i + 1)])) << 16);
  bool good = ok(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking), "hipStreamCreate");
  for (hipEvent_t& e : d->ev) good = good && ok(hipEventCreate(&e), "hipEventCreate");
  good = good && d->nco.reserve(nco.size()) && d->carry[0].reserve(d->carry_stride * nstreams) && d->carry[1].reserve(d->carry_stride * nstreams) &&
         d->power.reserve(static_cast<size_t>(nstreams) * kScanSize) && ok(hipMemcpyAsync(d->nco.get(), nco.data(), nco.size() * 4, hipMemcpyHostToDevice, d->stream), "NCO table upload") &&
         ok(hipMemsetAsync(d->power.get(), 0, static_cast<size_t>(nstreams) * kScanSize * sizeof(unsigned long long), d->stream), "spectrum") &&
         ok(hipStreamSynchronize(d->stream), "table upload");
  if (!good) { delete d; return nullptr; }
  return d;
}

extern "C" void dabhip_scan_destroy(dabhip_scan* d) { delete d; }

extern "C" int64_t dabhip_scan_push(dabhip_scan* d, const void* const* src, const size_t* nbytes, int on_device)
{
  if (!d || !src || !nbytes) { set_error("scan_push: null argument"); return -1; }
  const int ns = d->nstreams;
  const size_t sb = static_cast<size_t>(d->sample_bytes);
  std::vector<const void*> dev(static_cast<size_t>(ns), nullptr);
  std::vector<int64_t> nsamples(static_cast<size_t>(ns), 0);
  size_t stage_total = 0;
  for (int b = 0; b < ns; ++b) {
    if (nbytes[b] % sb) { set_error("scan_push: stream " + std::to_string(b) + ": " + std::to_string(nbytes[b]) + " bytes are no whole number of " + std::to_string(sb) + "-byte samples"); return -1; }
    if (nbytes[b] && !src[b]) { set_error("scan_push: null input"); return -1; }
    if (on_device && nbytes[b] && reinterpret_cast<uintptr_t>(src[b]) % sb) { set_error("scan_push: a device input must be aligned to its sample size"); return -1; }
    nsamples[static_cast<size_t>(b)] = static_cast<int64_t>(nbytes[b] / sb);
    // the host path uploads only what the window can still use: the unfinished segment and the segments that are missing
    if (!on_device) {
      const ScanStreamState& s = d->st[static_cast<size_t>(b)];
      const int64_t wanted = s.done == d->nsegments ? 0 : static_cast<int64_t>(d->nsegments) * kScanSize - s.pushed;
      stage_total += round_up(static_cast<size_t>(std::min<int64_t>(nsamples[static_cast<size_t>(b)], std::max<int64_t>(wanted, 0))) * sb, 16);
    }
  }
  if (!ok(hipSetDevice(d->device), "hipSetDevice")) return -1;
  if (on_device) {
    for (int b = 0; b < ns; ++b) dev[static_cast<size_t>(b)] = src[b];
    return push_device(d, dev, nsamples, false);
  }
  if (!d->stage.reserve(stage_total ? stage_total : 1) || !ok(hipEventRecord(d->ev[0], d->stream), "event")) return -1;
  size_t at = 0;
  for (int b = 0; b < ns; ++b) {
    const ScanStreamState& s = d->st[static_cast<size_t>(b)];
    const int64_t wanted = s.done == d->nsegments ? 0 : static_cast<int64_t>(d->nsegments) * kScanSize - s.pushed;
    const size_t up = static_cast<size_t>(std::min<int64_t>(nsamples[static_cast<size_t>(b)], std::max<int64_t>(wanted, 0))) * sb;
    dev[static_cast<size_t>(b)] = d->stage.get() + at;
    if (up && !ok(hipMemcpyAsync(d->stage.get() + at, src[b], up, hipMemcpyHostToDevice, d->stream), "upload")) return -1;
    at += round_up(up, 16);
  }
  return push_device(d, dev, nsamples, true);
}

extern "C" int dabhip_scan_spectrum(const dabhip_scan* d, int stream, uint64_t* P, int* nsegments_done)
{
  if (!d || stream < 0 || stream >= d->nstreams || !P) { set_error("scan_spectrum: bad argument"); return -1; }
  if (!ok(hipSetDevice(d->device), "hipSetDevice")) return -1;
  if (!ok(blocking_copy(P, d->power.get() + static_cast<size_t>(stream) * kScanSize, kScanSize * sizeof(uint64_t), hipMemcpyDeviceToHost), "read")) return -1;
  if (nsegments_done) *nsegments_done = static_cast<int>(d->st[static_cast<size_t>(stream)].done);
  return 0;
}

extern "C" int dabhip_scan_blocks(const dabhip_scan* d, int stream, int64_t center_hz, dabhip_scan_block* out, int cap)
{
  if (!d || (!out && cap > 0) || cap < 0) { set_error("scan_blocks: bad argument"); return -1; }
  std::vector<uint64_t> P(static_cast<size_t>(kScanSize));
  if (dabhip_scan_spectrum(d, stream, P.data(), nullptr) != 0) return -1;
  return dabhip_scan_detect(P.data(), d->rate, center_hz, out, cap);
}

extern "C" int dabhip_scan_stage_ms(const dabhip_scan* d, const char** names, float* ms, int cap)
{
  static const char* const kNames[3] = {"upload", "transform", "keep"};
  if (!d || !names || !ms) { set_error("scan_stage_ms: null argument"); return -1; }
  for (int k = 0; k < 3 && k < cap; ++k) { names[k] = kNames[k]; ms[k] = d->ms[k]; }
  return std::min(cap, 3);
}
