// ts.cpp — dabhip_ts: the stateful consumer of ETI frames that carries MPEG-2 TS sub-channels (dabhip.h).  Each push runs the kernels of
// k_ts.hip on its own HIP stream over the frames where they lie (device) or after one upload (host); between pushes it keeps the unconsumed
// bytes of every (stream, sub-channel), 2447 at most, in one of two carry buffers and the sync state on the device.  The records, the packets'
// bytes and the counters stay on the device until asked for.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "kernels.hpp"
#include "rs_code.hpp"
#include "stage_frame.hpp"
#include "ts.hpp"

using namespace dabhip;

namespace {
constexpr int kNStages = 9;
const char* const kStages[kNStages] = {"locate", "runs", "sync", "jobs", "gather", "syndrome", "decode", "parse", "carry"};
}

struct dabhip_ts {
  int nstreams = 0, nsub = 0;
  DeviceBuffer<int32_t> subch;
  DeviceBuffer<TsSync> sync;
  DeviceBuffer<TsLane> lanes;
  DeviceBuffer<int64_t> counters;
  DeviceBuffer<uint8_t> carry[2];
  int cur = 0;
  DeviceBuffer<uint8_t> staging;
  DeviceBuffer<uint8_t> meta;                       // base (int64) | nnew (int), per stream
  DeviceBuffer<TsLoc> loc;
  DeviceBuffer<uint64_t> flags;
  DeviceBuffer<TsSlot> slots;
  DeviceBuffer<TsUnit> units;
  DeviceBuffer<int> nunits, lane_unit_base, totals;
  DeviceBuffer<uint8_t> words, data, cw_status, gf;
  DeviceBuffer<uint32_t> syn;
  DeviceBuffer<dabhip_ts_rec> recs;
  int64_t n_units = 0;
  // host copy of the last push's lane bases, fetched on first use
  mutable bool fetched = false;
  mutable std::vector<int> h_base;
  StageFrame<kNStages> f{"ts", kStages};

  bool fetch() const
  {
    if (fetched) return true;
    if (!f.use_device()) return false;
    const size_t nlanes = static_cast<size_t>(nstreams) * nsub;
    h_base.assign(nlanes + 1, 0);
    if (n_units > 0 && !f.ok(blocking_copy(h_base.data(), lane_unit_base.get(), sizeof(int) * (nlanes + 1), hipMemcpyDeviceToHost), "records")) return false;
    fetched = true;
    return true;
  }

  bool lane_ok(int s, int q) const
  {
    if (s < 0 || s >= nstreams || q < 0 || q >= nsub) { set_error("ts: no such stream / sub-channel"); return false; }
    return true;
  }

  // the units of one lane of the last push: [a, a + n) of the push's list
  bool lane_range(int stream, int sub, int64_t& a, int64_t& n) const
  {
    if (!lane_ok(stream, sub) || !fetch()) return false;
    const int l = stream * nsub + sub;
    a = h_base[l];
    n = h_base[l + 1] - a;
    return true;
  }
};

extern "C" dabhip_ts* dabhip_ts_create(int device, int nstreams, const int32_t* subch_ids, int nsub)
{
  std::unique_ptr<dabhip_ts> d(new dabhip_ts);
  StageFrame<kNStages>& f = d->f;
  if (!f.open(device, "no HIP device: the MPEG-2 TS stage runs on the GPU only", "ts_create: device index out of range")) return nullptr;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (nstreams <= 0 || nsub <= 0 || nsub > 64 || !subch_ids) { set_error("ts_create: bad arguments"); return nullptr; }
  for (int q = 0; q < nsub; ++q)
    if (subch_ids[q] < 0 || subch_ids[q] > 63) { set_error("ts_create: SubChId out of range"); return nullptr; }
  if (static_cast<int64_t>(nstreams) * nsub > (1 << 18)) { set_error("ts_create: too many (stream, sub-channel) pairs"); return nullptr; }
  d->nstreams = nstreams;
  d->nsub = nsub;
  const size_t nlanes = static_cast<size_t>(nstreams) * nsub;
  GfRs<kPkRoots> gf;
  rs_tables_fill(gf);
  const size_t carry_bytes = nlanes * kTsCarryStride;
  bool good = d->subch.reserve(nsub) && d->sync.reserve(nlanes) && d->lanes.reserve(nlanes) && d->counters.reserve(nlanes * kTsCntN) && d->gf.reserve(sizeof gf) &&
              d->carry[0].reserve(carry_bytes) && d->carry[1].reserve(carry_bytes) && d->totals.reserve(kTsTotN) && d->nunits.reserve(nlanes) &&
              d->lane_unit_base.reserve(nlanes + 1);
  good = good && ok(hipMemcpy(d->subch.get(), subch_ids, sizeof(int32_t) * nsub, hipMemcpyHostToDevice), "upload") &&
         ok(hipMemset(d->sync.get(), 0, sizeof(TsSync) * nlanes), "clear") && ok(hipMemset(d->counters.get(), 0, sizeof(int64_t) * nlanes * kTsCntN), "clear") &&
         ok(hipMemcpy(d->gf.get(), &gf, sizeof gf, hipMemcpyHostToDevice), "upload");
  return good ? d.release() : nullptr;
}

extern "C" void dabhip_ts_destroy(dabhip_ts* d) { delete d; }

extern "C" int64_t dabhip_ts_push(dabhip_ts* d, const uint8_t* frames, const int64_t* counts, int on_device)
{
  if (!d || !counts) { set_error("ts_push: null argument"); return -1; }
  StageFrame<kNStages>& f = d->f;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!f.use_device()) return -1;
  const int ns = d->nstreams, nsub = d->nsub;
  std::vector<int64_t> base(static_cast<size_t>(ns));
  int64_t total = 0;
  int maxv = 0;
  for (int s = 0; s < ns; ++s) {
    if (counts[s] < 0 || counts[s] > (1 << 16)) { set_error("ts_push: bad frame count"); return -1; }
    base[s] = total;
    total += counts[s];
    maxv = std::max<int>(maxv, static_cast<int>(counts[s]));
  }
  if (total > 0 && !frames) { set_error("ts_push: null frames"); return -1; }
  const uint8_t* src = frames;
  if (total > 0 && !on_device) {
    const size_t bytes = static_cast<size_t>(total) * DABHIP_ETI_BYTES;
    if (!d->staging.reserve(bytes) || !ok(hipMemcpyAsync(d->staging.get(), frames, bytes, hipMemcpyHostToDevice, f.stream), "upload")) return -1;
    src = d->staging.get();
  }
  // per-stream metadata in one upload: base | nnew
  std::vector<uint8_t> meta(static_cast<size_t>(ns) * 12);
  std::memcpy(meta.data(), base.data(), sizeof(int64_t) * ns);
  for (int s = 0; s < ns; ++s) {
    const int n = static_cast<int>(counts[s]);
    std::memcpy(meta.data() + 8 * ns + 4 * s, &n, 4);
  }
  const int64_t nlanes = static_cast<int64_t>(ns) * nsub;
  // What the push can hold at most.  The sub-channels of one frame do not overlap, so the lanes of a stream share its frames' 6144 bytes: all
  // lanes together have their carried bytes and the frames' bytes.  A flag word covers 64 positions of one lane (one more for its ragged end); a
  // unit needs 204 bytes of its own lane.  One lane alone can give ts_unit_bound of its carried bytes and maxv frames at the largest STL.
  const int64_t all_bytes = nlanes * kTsCarry + total * DABHIP_ETI_BYTES;
  const int64_t flag_cap = all_bytes / 64 + nlanes;
  const int64_t unit_cap = all_bytes / kTsSlot + 1;
  const int cap = static_cast<int>(ts_unit_bound(kTsCarry, maxv, kTsStlMax)) + 1;
  if (all_bytes >= (int64_t{1} << 31) || flag_cap >= (int64_t{1} << 31) || nlanes * cap >= (int64_t{1} << 31)) { set_error("ts_push: too many frames for one push"); return -1; }
  if (!d->meta.reserve(meta.size()) || !d->loc.reserve(static_cast<size_t>(ns) * std::max(maxv, 1) * nsub) || !d->flags.reserve(static_cast<size_t>(flag_cap)) ||
      !d->slots.reserve(static_cast<size_t>(nlanes) * cap) || !d->units.reserve(static_cast<size_t>(unit_cap)))
    return -1;
  // the host copy of meta must outlive the asynchronous copy: hipMemcpy from pageable memory returns once the bytes are staged
  if (!ok(hipMemcpyAsync(d->meta.get(), meta.data(), meta.size(), hipMemcpyHostToDevice, f.stream), "upload") || !ok(hipStreamSynchronize(f.stream), "upload"))
    return -1;
  PacketFrames fr;
  fr.frames = src;
  fr.base = reinterpret_cast<const int64_t*>(d->meta.get());
  fr.nnew = reinterpret_cast<const int*>(d->meta.get() + 8 * ns);
  hipStream_t st = f.stream;
  const uint8_t* carry = d->carry[d->cur].get();
  // the runs kernel's workgroups per lane: about 8 words of flags per wave for a lane at the largest rate, 64 at most
  const int per_lane = static_cast<int>(std::min<int64_t>(64, std::max<int64_t>(1, (kTsCarry + static_cast<int64_t>(maxv) * kTsFrameBytesMax) / (64 * 4 * 8))));
  int totals[kTsTotN] = {0, 0, 0, 0};
  const int nl = static_cast<int>(nlanes);
  bool good = ok(hipMemsetAsync(d->totals.get(), 0, sizeof totals, st), "clear") && f.mark(0) &&
              ok(launch_ts_locate(fr, d->subch.get(), nsub, ns, maxv, d->loc.get(), d->sync.get(), d->lanes.get(), static_cast<int>(flag_cap), d->totals.get(), st), "locate") &&
              f.mark(1) && ok(launch_ts_runs(fr, nl, nsub, maxv, per_lane, d->loc.get(), d->lanes.get(), carry, d->totals.get(), d->flags.get(), st), "runs") &&
              f.mark(2) &&
              ok(launch_ts_sync(fr, nl, nsub, maxv, d->loc.get(), d->sync.get(), d->lanes.get(), carry, d->flags.get(), d->slots.get(), cap, d->nunits.get(),
                                d->counters.get(), d->totals.get(), st), "sync") &&
              f.mark(3) &&
              ok(launch_ts_jobs(nl, d->slots.get(), cap, d->nunits.get(), d->lane_unit_base.get(), d->sync.get(), d->lanes.get(), d->units.get(), unit_cap,
                                d->totals.get(), st), "jobs") &&
              f.mark(4) && ok(hipMemcpyAsync(totals, d->totals.get(), sizeof totals, hipMemcpyDeviceToHost, st), "totals") && ok(hipStreamSynchronize(st), "sync stage");
  if (!good) return -1;
  if (totals[kTsTotOverflow] || totals[kTsTotSlotOverflow] || totals[kTsTotUnits] > unit_cap) {
    set_error("ts_push: a lane gave more than its buffers hold; the handle's state is lost");
    return -1;
  }
  const int64_t nu = totals[kTsTotUnits];
  d->n_units = nu;
  d->fetched = false;
  const size_t cu = static_cast<size_t>(nu ? nu : 1);
  good = d->words.reserve(static_cast<size_t>(ts_word_buffer_bytes(static_cast<int64_t>(cu)))) && d->data.reserve(cu * kTsData) && d->recs.reserve(cu) &&
         d->cw_status.reserve(cu) && d->syn.reserve(cu * 4) &&
         ok(launch_ts_gather(fr, d->units.get(), d->totals.get(), nu, d->loc.get(), maxv, nsub, carry, d->lanes.get(), d->words.get(), st), "gather") &&
         f.mark(5) && ok(launch_ts_syndrome(d->totals.get(), nu, d->gf.get(), d->words.get(), d->cw_status.get(), d->syn.get(), st), "syndrome") &&
         f.mark(6) && ok(launch_ts_decode(d->totals.get(), nu, d->gf.get(), d->words.get(), d->cw_status.get(), d->syn.get(), st), "decode") &&
         f.mark(7) &&
         ok(launch_ts_parse(d->units.get(), d->totals.get(), nu, d->words.get(), d->cw_status.get(), d->recs.get(), d->data.get(), d->counters.get(), st), "parse") &&
         f.mark(8) && ok(launch_ts_carry(fr, nl, d->loc.get(), maxv, nsub, carry, d->lanes.get(), d->totals.get(), d->carry[d->cur ^ 1].get(), st), "carry") &&
         f.mark(9) && f.finish();
  if (!good) return -1;
  d->cur ^= 1;
  return nu;
}

extern "C" int64_t dabhip_ts_records(const dabhip_ts* d, int stream, int sub, dabhip_ts_rec* out, int64_t cap)
{
  int64_t a = 0, n = 0;
  if (!d || !d->lane_range(stream, sub, a, n)) return -1;
  const int64_t take = out ? std::min(n, std::max<int64_t>(cap, 0)) : 0;
  if (take > 0 && !d->f.ok(blocking_copy(out, d->recs.get() + a, sizeof(dabhip_ts_rec) * static_cast<size_t>(take), hipMemcpyDeviceToHost), "records")) return -1;
  return n;
}

extern "C" int64_t dabhip_ts_data(const dabhip_ts* d, int stream, int sub, uint8_t* dst, int64_t cap)
{
  int64_t a = 0, n = 0;
  if (!d || !d->lane_range(stream, sub, a, n)) return -1;
  const int64_t take = dst ? std::min(n, std::max<int64_t>(cap, 0) / kTsData) : 0;
  if (take > 0 && !d->f.ok(blocking_copy(dst, d->data.get() + a * kTsData, static_cast<size_t>(take) * kTsData, hipMemcpyDeviceToHost), "data")) return -1;
  return n * kTsData;
}

extern "C" int dabhip_ts_stats(const dabhip_ts* d, int stream, int sub, int64_t* counters8)
{
  if (!d || !counters8) { set_error("ts_stats: null argument"); return -1; }
  if (!d->lane_ok(stream, sub)) return -1;
  if (!d->f.use_device()) return -1;
  return d->f.ok(blocking_copy(counters8, d->counters.get() + (static_cast<size_t>(stream) * d->nsub + sub) * kTsCntN, sizeof(int64_t) * kTsCntN, hipMemcpyDeviceToHost),
                 "counters") ? 0 : -1;
}

extern "C" int dabhip_ts_stage_ms(const dabhip_ts* d, const char** names, float* ms, int cap)
{
  if (!d) return -1;
  return d->f.stage_ms(names, ms, cap);
}
