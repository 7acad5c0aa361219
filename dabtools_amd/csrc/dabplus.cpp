// dabplus.cpp — dabhip_dabplus: the stateful DAB+ consumer of ETI frames (dabhip.h).  Each push runs the kernels of k_dabplus.hip on its own
// HIP stream over the frames where they lie (device) or after one upload (host); between pushes it keeps the last 4 frames of every stream in
// one of two carry buffers and the sync state of every (stream, sub-channel) on the device.  The records, corrected bytes and counters stay on
// the device until asked for.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "dab_bits.hpp"
#include "dabplus.hpp"
#include "eti_lanes.hpp"
#include "kernels.hpp"

using namespace dabhip;

namespace {
const char* const kStages[5] = {"locate", "sync", "rs", "au", "carry"};
}

struct dabhip_dabplus {
  EtiLanes lanes{"dabplus"};                        // its host copy: the lanes' first superframes (lane_sf_base)
  DeviceBuffer<DabPlusSync> sync;
  DeviceBuffer<int64_t> counters;
  DeviceBuffer<uint8_t> carry[2];
  int cur = 0;
  std::vector<int> ncarry;
  DeviceBuffer<uint8_t> staging;
  DeviceBuffer<uint8_t> meta;                       // base (int64) | nnew (int) | ncarry (int), per stream
  DeviceBuffer<DabPlusLoc> loc;
  DeviceBuffer<DabPlusCand> cand;
  DeviceBuffer<int> ncand, lane_cw, lane_sf_base, lane_cw_base, totals;
  DeviceBuffer<DabPlusJob> jobs;
  DeviceBuffer<uint8_t> data, cw_status, gf;
  DeviceBuffer<uint32_t> syn;
  DeviceBuffer<uint16_t> crc_tab;
  DeviceBuffer<dabhip_dabplus_sf> recs;
  int64_t nsf = 0, ncw = 0;
  // host copies of the last push's records, fetched on first use
  mutable std::vector<dabhip_dabplus_sf> h_recs;
  mutable std::vector<int64_t> h_data_base;   // per superframe, and the total at the end
  StageFrame<5> f{"dabplus", kStages};

  // lane l's superframes of the last push, [a, a + n) of h_recs
  bool lane_range(int stream, int sub, int64_t& a, int64_t& n) const
  {
    if (!lanes.lane_ok(stream, sub)) return false;
    if (!lanes.fetched) {
      if (!f.use_device()) return false;
      h_recs.resize(static_cast<size_t>(nsf));
      if (nsf > 0 && !f.ok(blocking_copy(h_recs.data(), recs.get(), sizeof(dabhip_dabplus_sf) * static_cast<size_t>(nsf), hipMemcpyDeviceToHost), "records")) return false;
      h_data_base.assign(static_cast<size_t>(nsf) + 1, 0);
      for (int64_t i = 0; i < nsf; ++i) h_data_base[i + 1] = h_data_base[i] + static_cast<int64_t>(kRsK) * h_recs[i].s;
      if (!lanes.fetch(f, lane_sf_base.get(), nsf > 0)) return false;
    }
    lanes.range(stream, sub, a, n);
    return true;
  }
};

extern "C" dabhip_dabplus* dabhip_dabplus_create(int device, int nstreams, const int32_t* subch_ids, int nsub)
{
  std::unique_ptr<dabhip_dabplus> d(new dabhip_dabplus);
  StageFrame<5>& f = d->f;
  if (!f.open(device, "no HIP device: the DAB+ stage runs on the GPU only", "dabplus_create: device index out of range")) return nullptr;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!d->lanes.create(f, nstreams, subch_ids, nsub, true, 0)) return nullptr;
  d->ncarry.assign(static_cast<size_t>(nstreams), 0);
  const size_t nlanes = d->lanes.count();
  std::vector<uint16_t> crc(256 + kRsK * kMaxS);
  for (int v = 0; v < 256; ++v) {
    const uint8_t b = static_cast<uint8_t>(v);
    crc[v] = crc16_ccitt(&b, 1, 0);   // the CRC register after byte v from 0: the kernel's table-driven step
  }
  // x^(8 n) mod G, G = x^16 + x^12 + x^5 + 1: the register of n zero bytes from 1
  uint32_t r = 1;
  for (int n = 0; n < kRsK * kMaxS; ++n) {
    crc[256 + n] = static_cast<uint16_t>(r);
    for (int b = 0; b < 8; ++b) r = (r & 0x8000u) ? ((r << 1) ^ 0x1021u) & 0xffffu : (r << 1) & 0xffffu;
  }
  bool good = d->sync.reserve(nlanes) && d->counters.reserve(nlanes * kCntN) && d->crc_tab.reserve(crc.size()) &&
         d->carry[0].reserve(static_cast<size_t>(nstreams) * 4 * DABHIP_ETI_BYTES) && d->carry[1].reserve(static_cast<size_t>(nstreams) * 4 * DABHIP_ETI_BYTES) &&
         d->totals.reserve(2);
  good = good && ok(hipMemset(d->sync.get(), 0, sizeof(DabPlusSync) * nlanes), "clear") && ok(hipMemset(d->counters.get(), 0, sizeof(int64_t) * nlanes * kCntN), "clear") &&
         upload_rs_tables<kRsRoots>(f, d->gf) && ok(hipMemcpy(d->crc_tab.get(), crc.data(), crc.size() * 2, hipMemcpyHostToDevice), "upload");
  return good ? d.release() : nullptr;
}

extern "C" void dabhip_dabplus_destroy(dabhip_dabplus* d) { delete d; }

extern "C" int64_t dabhip_dabplus_push(dabhip_dabplus* d, const uint8_t* frames, const int64_t* counts, int on_device)
{
  if (!d || !counts) { set_error("dabplus_push: null argument"); return -1; }
  StageFrame<5>& f = d->f;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!f.use_device()) return -1;
  const int ns = d->lanes.nstreams, nsub = d->lanes.nsub;
  const EtiPush p = plan_eti_push("dabplus_push", counts, ns, !frames, 1 << 24, kEtiNoTotalBound, d->ncarry.data());
  if (!p.refusal.empty()) { set_error(p.refusal); return -1; }
  EtiFrames e;
  const int* ncarry = nullptr;
  if (!f.place(p, frames, on_device, d->staging, d->meta, e, &ncarry)) return -1;
  const DabPlusFrames fr{e.frames, d->carry[d->cur].get(), e.base, e.nnew, ncarry, (reinterpret_cast<uintptr_t>(e.frames) & 15) == 0};
  const size_t nlanes = d->lanes.count();
  const int maxv = p.maxv, cap = maxv / kSfFrames + 1;
  if (!d->loc.reserve(static_cast<size_t>(ns) * std::max(maxv, 1) * nsub) || !d->cand.reserve(nlanes * cap) || !d->jobs.reserve(nlanes * cap) || !d->ncand.reserve(nlanes) ||
      !d->lane_cw.reserve(nlanes) || !d->lane_sf_base.reserve(nlanes + 1) || !d->lane_cw_base.reserve(nlanes))
    return -1;
  hipStream_t st = f.stream;
  int totals[2] = {0, 0};
  bool good = f.mark(0) && ok(launch_dabplus_locate(fr, d->lanes.subch.get(), nsub, ns, maxv, d->loc.get(), st), "locate") &&
              f.mark(1) &&
              ok(launch_dabplus_sync(fr, ns, nsub, maxv, d->loc.get(), d->sync.get(), d->cand.get(), cap, d->ncand.get(), d->lane_cw.get(), d->counters.get(), d->jobs.get(),
                                     d->lane_sf_base.get(), d->lane_cw_base.get(), d->totals.get(), st), "sync") &&
              f.mark(2) && ok(hipMemcpyAsync(totals, d->totals.get(), sizeof totals, hipMemcpyDeviceToHost, st), "totals") &&
              ok(hipStreamSynchronize(st), "sync stage");
  if (!good) return -1;
  d->nsf = totals[0];
  d->ncw = totals[1];
  d->lanes.fetched = false;
  good = d->data.reserve(static_cast<size_t>(d->ncw) * kRsK + 16) && d->cw_status.reserve(static_cast<size_t>(d->ncw ? d->ncw : 1)) && d->recs.reserve(static_cast<size_t>(d->nsf ? d->nsf : 1)) &&
         d->syn.reserve(static_cast<size_t>(d->ncw ? d->ncw * 4 : 1)) &&
         ok(launch_dabplus_rs(d->jobs.get(), d->totals.get(), static_cast<int>(d->ncw), d->loc.get(), maxv, nsub, d->gf.get(), d->data.get(), d->cw_status.get(), d->syn.get(), st),
            "rs") &&
         f.mark(3) &&
         ok(launch_dabplus_au(d->jobs.get(), static_cast<int>(d->nsf), d->loc.get(), maxv, nsub, d->data.get(), d->cw_status.get(), d->crc_tab.get(), d->recs.get(), d->counters.get(), st),
            "au") &&
         f.mark(4) && ok(launch_dabplus_carry(fr, ns, d->carry[d->cur ^ 1].get(), st), "carry") &&
         f.mark(5) && f.finish();
  if (!good) return -1;
  d->cur ^= 1;
  for (int s = 0; s < ns; ++s) d->ncarry[s] = std::min(4, d->ncarry[s] + static_cast<int>(counts[s]));
  return d->nsf;
}

extern "C" int64_t dabhip_dabplus_superframes(const dabhip_dabplus* d, int stream, int sub, dabhip_dabplus_sf* out, int64_t cap)
{
  int64_t a = 0, n = 0;
  if (!d || !d->lane_range(stream, sub, a, n)) return -1;
  if (out && cap > 0) std::memcpy(out, d->h_recs.data() + a, sizeof(dabhip_dabplus_sf) * static_cast<size_t>(std::min(n, cap)));
  return n;
}

namespace {
// the corrected bytes of one (stream, sub-channel) of the last push, on the host
bool lane_data(const dabhip_dabplus* d, int stream, int sub, std::vector<uint8_t>& out, int64_t* first_sf, int64_t* nsf)
{
  if (!d || !d->lane_range(stream, sub, *first_sf, *nsf)) return false;
  const int64_t a = d->h_data_base[*first_sf], b = d->h_data_base[*first_sf + *nsf];
  out.resize(static_cast<size_t>(b - a));
  return b == a || d->f.ok(blocking_copy(out.data(), d->data.get() + a, static_cast<size_t>(b - a), hipMemcpyDeviceToHost), "data");
}
}  // namespace

extern "C" int64_t dabhip_dabplus_data(const dabhip_dabplus* d, int stream, int sub, uint8_t* dst, int64_t cap)
{
  std::vector<uint8_t> bytes;
  int64_t a = 0, n = 0;
  if (!lane_data(d, stream, sub, bytes, &a, &n)) return -1;
  if (dst && cap > 0) std::memcpy(dst, bytes.data(), static_cast<size_t>(std::min<int64_t>(cap, static_cast<int64_t>(bytes.size()))));
  return static_cast<int64_t>(bytes.size());
}

extern "C" int64_t dabhip_dabplus_au_bytes(const dabhip_dabplus* d, int stream, int sub, uint8_t* dst, int64_t cap)
{
  std::vector<uint8_t> bytes;
  int64_t a = 0, n = 0;
  if (!lane_data(d, stream, sub, bytes, &a, &n)) return -1;
  int64_t w = 0, off = 0;
  for (int64_t i = 0; i < n; ++i) {
    const dabhip_dabplus_sf& r = d->h_recs[a + i];
    if (r.layout_ok)
      for (int k = 0; k < r.num_aus; ++k) {
        if (!(r.crc_ok >> k & 1)) continue;
        const int64_t len = r.au_len[k] - 2;
        if (dst && w + len <= cap) std::memcpy(dst + w, bytes.data() + off + r.au_start[k], static_cast<size_t>(len));
        w += len;
      }
    off += static_cast<int64_t>(kRsK) * r.s;
  }
  return w;
}

extern "C" int dabhip_dabplus_stats(const dabhip_dabplus* d, int stream, int sub, int64_t* counters7)
{
  if (!d || !counters7) { set_error("dabplus_stats: null argument"); return -1; }
  return d->lanes.lane_counters(d->f, stream, sub, d->counters.get(), kCntN, counters7, 7);
}

extern "C" int dabhip_dabplus_stage_ms(const dabhip_dabplus* d, const char** names, float* ms, int cap)
{
  if (!d) return -1;
  d->f.stage_ms(names, ms, cap);
  return 5;
}
