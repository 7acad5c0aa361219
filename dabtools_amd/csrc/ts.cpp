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
#include "eti_lanes.hpp"
#include "kernels.hpp"
#include "ts.hpp"

using namespace dabhip;

namespace {
constexpr int kNStages = 9;
const char* const kStages[kNStages] = {"locate", "runs", "sync", "jobs", "gather", "syndrome", "decode", "parse", "carry"};
}

struct dabhip_ts {
  EtiLanes lanes{"ts"};                             // its host copy: the lanes' first units (lane_unit_base)
  DeviceBuffer<TsSync> sync;
  DeviceBuffer<TsLane> lane_state;
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
  StageFrame<kNStages> f{"ts", kStages};

  // the units of one lane of the last push: [a, a + n) of the push's list
  bool lane_range(int stream, int sub, int64_t& a, int64_t& n) const
  {
    if (!lanes.lane_ok(stream, sub) || !lanes.fetch(f, lane_unit_base.get(), n_units > 0)) return false;
    lanes.range(stream, sub, a, n);
    return true;
  }
};

extern "C" dabhip_ts* dabhip_ts_create(int device, int nstreams, const int32_t* subch_ids, int nsub)
{
  std::unique_ptr<dabhip_ts> d(new dabhip_ts);
  StageFrame<kNStages>& f = d->f;
  if (!f.open(device, "no HIP device: the MPEG-2 TS stage runs on the GPU only", "ts_create: device index out of range")) return nullptr;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!d->lanes.create(f, nstreams, subch_ids, nsub, true, 1 << 18)) return nullptr;
  const size_t nlanes = d->lanes.count();
  const size_t carry_bytes = nlanes * kTsCarryStride;
  bool good = d->sync.reserve(nlanes) && d->lane_state.reserve(nlanes) && d->counters.reserve(nlanes * kTsCntN) && d->carry[0].reserve(carry_bytes) &&
              d->carry[1].reserve(carry_bytes) && d->totals.reserve(kTsTotN) && d->nunits.reserve(nlanes) && d->lane_unit_base.reserve(nlanes + 1);
  good = good && ok(hipMemset(d->sync.get(), 0, sizeof(TsSync) * nlanes), "clear") && ok(hipMemset(d->counters.get(), 0, sizeof(int64_t) * nlanes * kTsCntN), "clear") &&
         upload_rs_tables<kPkRoots>(f, d->gf);
  return good ? d.release() : nullptr;
}

extern "C" void dabhip_ts_destroy(dabhip_ts* d) { delete d; }

extern "C" int64_t dabhip_ts_push(dabhip_ts* d, const uint8_t* frames, const int64_t* counts, int on_device)
{
  if (!d || !counts) { set_error("ts_push: null argument"); return -1; }
  StageFrame<kNStages>& f = d->f;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!f.use_device()) return -1;
  const int ns = d->lanes.nstreams, nsub = d->lanes.nsub;
  const EtiPush p = plan_eti_push("ts_push", counts, ns, !frames, 1 << 16, kEtiNoTotalBound);
  if (!p.refusal.empty()) { set_error(p.refusal); return -1; }
  EtiFrames fr;
  if (!f.place(p, frames, on_device, d->staging, d->meta, fr)) return -1;
  const int64_t nlanes = static_cast<int64_t>(d->lanes.count()), total = p.total;
  const int maxv = p.maxv;
  // What the push can hold at most.  The sub-channels of one frame do not overlap, so the lanes of a stream share its frames' 6144 bytes: all
  // lanes together have their carried bytes and the frames' bytes.  A flag word covers 64 positions of one lane (one more for its ragged end); a
  // unit needs 204 bytes of its own lane.  One lane alone can give ts_unit_bound of its carried bytes and maxv frames at the largest STL.
  const int64_t all_bytes = nlanes * kTsCarry + total * DABHIP_ETI_BYTES;
  const int64_t flag_cap = all_bytes / 64 + nlanes;
  const int64_t unit_cap = all_bytes / kTsSlot + 1;
  const int cap = static_cast<int>(ts_unit_bound(kTsCarry, maxv, kTsStlMax)) + 1;
  if (all_bytes >= (int64_t{1} << 31) || flag_cap >= (int64_t{1} << 31) || nlanes * cap >= (int64_t{1} << 31)) { set_error("ts_push: too many frames for one push"); return -1; }
  if (!d->loc.reserve(static_cast<size_t>(ns) * std::max(maxv, 1) * nsub) || !d->flags.reserve(static_cast<size_t>(flag_cap)) ||
      !d->slots.reserve(static_cast<size_t>(nlanes) * cap) || !d->units.reserve(static_cast<size_t>(unit_cap)))
    return -1;
  hipStream_t st = f.stream;
  const uint8_t* carry = d->carry[d->cur].get();
  // the runs kernel's workgroups per lane: about 8 words of flags per wave for a lane at the largest rate, 64 at most
  const int per_lane = static_cast<int>(std::min<int64_t>(64, std::max<int64_t>(1, (kTsCarry + static_cast<int64_t>(maxv) * kTsFrameBytesMax) / (64 * 4 * 8))));
  int totals[kTsTotN] = {0, 0, 0, 0};
  const int nl = static_cast<int>(nlanes);
  bool good = ok(hipMemsetAsync(d->totals.get(), 0, sizeof totals, st), "clear") && f.mark(0) &&
              ok(launch_ts_locate(fr, d->lanes.subch.get(), nsub, ns, maxv, d->loc.get(), d->sync.get(), d->lane_state.get(), static_cast<int>(flag_cap), d->totals.get(), st), "locate") &&
              f.mark(1) && ok(launch_ts_runs(fr, nl, nsub, maxv, per_lane, d->loc.get(), d->lane_state.get(), carry, d->totals.get(), d->flags.get(), st), "runs") &&
              f.mark(2) &&
              ok(launch_ts_sync(fr, nl, nsub, maxv, d->loc.get(), d->sync.get(), d->lane_state.get(), carry, d->flags.get(), d->slots.get(), cap, d->nunits.get(),
                                d->counters.get(), d->totals.get(), st), "sync") &&
              f.mark(3) &&
              ok(launch_ts_jobs(nl, d->slots.get(), cap, d->nunits.get(), d->lane_unit_base.get(), d->sync.get(), d->lane_state.get(), d->units.get(), unit_cap,
                                d->totals.get(), st), "jobs") &&
              f.mark(4) && ok(hipMemcpyAsync(totals, d->totals.get(), sizeof totals, hipMemcpyDeviceToHost, st), "totals") && ok(hipStreamSynchronize(st), "sync stage");
  if (!good) return -1;
  if (totals[kTsTotOverflow] || totals[kTsTotSlotOverflow] || totals[kTsTotUnits] > unit_cap) {
    set_error("ts_push: a lane gave more than its buffers hold; the handle's state is lost");
    return -1;
  }
  const int64_t nu = totals[kTsTotUnits];
  d->n_units = nu;
  d->lanes.fetched = false;
  const size_t cu = static_cast<size_t>(nu ? nu : 1);
  good = d->words.reserve(static_cast<size_t>(ts_word_buffer_bytes(static_cast<int64_t>(cu)))) && d->data.reserve(cu * kTsData) && d->recs.reserve(cu) &&
         d->cw_status.reserve(cu) && d->syn.reserve(cu * 4) &&
         ok(launch_ts_gather(fr, d->units.get(), d->totals.get(), nu, d->loc.get(), maxv, nsub, carry, d->lane_state.get(), d->words.get(), st), "gather") &&
         f.mark(5) && ok(launch_ts_syndrome(d->totals.get(), nu, d->gf.get(), d->words.get(), d->cw_status.get(), d->syn.get(), st), "syndrome") &&
         f.mark(6) && ok(launch_ts_decode(d->totals.get(), nu, d->gf.get(), d->words.get(), d->cw_status.get(), d->syn.get(), st), "decode") &&
         f.mark(7) &&
         ok(launch_ts_parse(d->units.get(), d->totals.get(), nu, d->words.get(), d->cw_status.get(), d->recs.get(), d->data.get(), d->counters.get(), st), "parse") &&
         f.mark(8) && ok(launch_ts_carry(fr, nl, d->loc.get(), maxv, nsub, carry, d->lane_state.get(), d->totals.get(), d->carry[d->cur ^ 1].get(), st), "carry") &&
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
  return d->lanes.lane_counters(d->f, stream, sub, d->counters.get(), kTsCntN, counters8, kTsCntN);
}

extern "C" int dabhip_ts_stage_ms(const dabhip_ts* d, const char** names, float* ms, int cap)
{
  if (!d) return -1;
  return d->f.stage_ms(names, ms, cap);
}
