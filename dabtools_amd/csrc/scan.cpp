// scan.cpp — the block scan's host object (include/dabhip.h: dabhip_scan): per stream the positions, the carried samples of an unfinished segment and
// the spectrum; per push the plan (scan_blocks.hpp), the uploads and one launch of k_scan.hip's transform for all streams.  Every push ends in a
// stream synchronise (hip_util.hpp: what the runtime keeps of a stream that nobody synchronises).
#include <new>
#include <string>
#include <vector>

#include "capi_detail.hpp"
#include "ingest_plan.hpp"
#include "scan.hpp"
#include "scan_blocks.hpp"
#include "stage_frame.hpp"

using namespace dabhip;

namespace {
const char* const kStages[3] = {"upload", "transform", "keep"};
}

struct dabhip_scan {
  int nstreams = 0, format = 0, sample_bytes = 0, nsegments = 0;
  int64_t rate = 0;
  std::vector<ScanStreamState> st;
  DeviceBuffer<uint32_t> nco;
  DeviceBuffer<uint8_t> carry[2], stage;
  DeviceBuffer<ScanDesc> descs;
  DeviceBuffer<unsigned long long> power;          // nstreams spectra of 4096 bins
  size_t carry_stride = 0;
  int cur = 0;                                     // carry[cur] holds what the last push kept
  StageFrame<3> f{"scan", kStages};
};

namespace {
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
  StageFrame<3>& f = d->f;
  if (!d->descs.reserve(h.size())) return -1;
  if (!uploaded && !f.mark(0)) return -1;
  if (!f.mark(1) || !f.ok(hipMemcpyAsync(d->descs.get(), h.data(), h.size() * sizeof(ScanDesc), hipMemcpyHostToDevice, f.stream), "descriptors") ||
      !f.ok(launch_scan_transform(d->format, d->descs.get(), ns, max_nseg, d->nco.get(), f.stream), "transform launch") || !f.mark(2) ||
      !f.ok(launch_scan_keep(d->format, d->descs.get(), ns, max_keep, f.stream), "keep launch") || !f.mark(3) || !f.finish())
    return -1;
  d->st = next;
  d->cur ^= 1;
  return total;
}
}  // namespace

extern "C" dabhip_scan* dabhip_scan_create(int device, int nstreams, int format, int64_t rate_hz, int nsegments)
{
  const std::string why = scan_check(nstreams, format, rate_hz, nsegments);
  if (!why.empty()) { set_error("scan_create: " + why); return nullptr; }
  dabhip_scan* d = new (std::nothrow) dabhip_scan;
  if (!d) return nullptr;
  StageFrame<3>& f = d->f;
  d->nstreams = nstreams;
  d->format = format;
  d->sample_bytes = ingest_sample_bytes(format);
  d->rate = rate_hz;
  d->nsegments = nsegments;
  d->st.assign(static_cast<size_t>(nstreams), ScanStreamState{});
  d->carry_stride = static_cast<size_t>(kScanSize) * d->sample_bytes;      // at most 4095 samples are carried
  const std::vector<uint32_t> nco = ingest_tune_nco_words();
  const bool good = f.open(device, "scan_create: no HIP device") && d->nco.reserve(nco.size()) && d->carry[0].reserve(d->carry_stride * nstreams) &&
                    d->carry[1].reserve(d->carry_stride * nstreams) && d->power.reserve(static_cast<size_t>(nstreams) * kScanSize) &&
                    f.ok(hipMemcpyAsync(d->nco.get(), nco.data(), nco.size() * 4, hipMemcpyHostToDevice, f.stream), "NCO table upload") &&
                    f.ok(hipMemsetAsync(d->power.get(), 0, static_cast<size_t>(nstreams) * kScanSize * sizeof(unsigned long long), f.stream), "spectrum") &&
                    f.ok(hipStreamSynchronize(f.stream), "table upload");
  if (!good) { delete d; return nullptr; }
  return d;
}

extern "C" void dabhip_scan_destroy(dabhip_scan* d) { delete d; }

extern "C" int64_t dabhip_scan_push(dabhip_scan* d, const void* const* src, const size_t* nbytes, int on_device)
{
  if (!d || !src || !nbytes) { set_error("scan_push: null argument"); return -1; }
  const SamplePush p = plan_sample_push("scan_push", static_cast<size_t>(d->sample_bytes), src, nbytes, on_device != 0, d->nstreams,
                                        [&](int b, int64_t n) { return scan_upload_samples(d->nsegments, d->st[static_cast<size_t>(b)], n); });
  if (!p.refusal.empty()) { set_error(p.refusal); return -1; }
  std::vector<const void*> dev(src, src + d->nstreams);
  if (!d->f.use_device() || (!on_device && !d->f.upload(d->stage, p, src, dev))) return -1;
  return push_device(d, dev, p.nsamples, !on_device);
}

extern "C" int dabhip_scan_spectrum(const dabhip_scan* d, int stream, uint64_t* P, int* nsegments_done)
{
  if (!d || stream < 0 || stream >= d->nstreams || !P) { set_error("scan_spectrum: bad argument"); return -1; }
  if (!d->f.use_device()) return -1;
  if (!d->f.ok(blocking_copy(P, d->power.get() + static_cast<size_t>(stream) * kScanSize, kScanSize * sizeof(uint64_t), hipMemcpyDeviceToHost), "read")) return -1;
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
  if (!d || !names || !ms) { set_error("scan_stage_ms: null argument"); return -1; }
  return d->f.stage_ms(names, ms, cap);
}
