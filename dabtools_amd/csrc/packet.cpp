// packet.cpp — dabhip_packet: the stateful packet-mode consumer of ETI frames (dabhip.h), and dabhip_packet_groups, the host rule above it
// (packet_groups.hpp).  Each push runs the kernels of k_packet.hip on its own HIP stream over the frames where they lie (device) or after one
// upload (host); between pushes it keeps the unconsumed cells of every (stream, sub-channel), 102 at most, in one of two carry buffers and the
// sync state on the device.  The per-cell records, the cell buffer and the counters stay on the device until asked for.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "dab_bits.hpp"
#include "eti_lanes.hpp"
#include "kernels.hpp"
#include "packet.hpp"
#include "packet_groups.hpp"

using namespace dabhip;

namespace {
const char* const kStages[7] = {"locate", "sync", "gather", "rs", "cand", "walk", "carry"};
}

struct dabhip_packet {
  EtiLanes lanes{"packet"};                         // its host copy: the lanes' first cells in the cell buffer (lane_buf_base)
  DeviceBuffer<uint8_t> fec;
  DeviceBuffer<PacketSync> sync;
  DeviceBuffer<int64_t> counters;
  DeviceBuffer<uint8_t> carry[2];
  int cur = 0;
  DeviceBuffer<uint8_t> staging;
  DeviceBuffer<uint8_t> meta;                       // base (int64) | nnew (int), per stream
  DeviceBuffer<PacketLoc> loc;
  DeviceBuffer<PacketSlot> slots;
  DeviceBuffer<PacketUnit> units;
  DeviceBuffer<int> nunits, lane_buf, ncar_in, ncar_out, lo, lane_unit_base, lane_buf_base, totals;
  DeviceBuffer<uint8_t> cells, cand, cw_status, gf;
  DeviceBuffer<uint32_t> syn;
  DeviceBuffer<uint16_t> crc_tab;
  DeviceBuffer<dabhip_packet_rec> recs;
  int64_t n_units = 0, n_cells = 0;
  StageFrame<7> f{"packet", kStages};

  // the per-cell records of one lane of the last push, and its cells when asked for
  bool lane_cells(int stream, int sub, std::vector<dabhip_packet_rec>& r, std::vector<uint8_t>* bytes) const
  {
    if (!lanes.lane_ok(stream, sub) || !lanes.fetch(f, lane_buf_base.get(), n_cells > 0)) return false;
    int64_t a = 0, n = 0;
    lanes.range(stream, sub, a, n);
    r.resize(static_cast<size_t>(n));
    if (bytes) bytes->resize(static_cast<size_t>(n) * kPkCell);
    if (n == 0) return true;
    if (!f.ok(blocking_copy(r.data(), recs.get() + a, sizeof(dabhip_packet_rec) * static_cast<size_t>(n), hipMemcpyDeviceToHost), "records")) return false;
    return !bytes || f.ok(blocking_copy(bytes->data(), cells.get() + a * kPkCell, bytes->size(), hipMemcpyDeviceToHost), "data");
  }
};

extern "C" dabhip_packet* dabhip_packet_create(int device, int nstreams, const int32_t* subch_ids, const uint8_t* fec_flags, int nsub)
{
  std::unique_ptr<dabhip_packet> d(new dabhip_packet);
  StageFrame<7>& f = d->f;
  if (!f.open(device, "no HIP device: the packet-mode stage runs on the GPU only", "packet_create: device index out of range")) return nullptr;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!d->lanes.create(f, nstreams, subch_ids, nsub, fec_flags != nullptr, 1 << 24)) return nullptr;
  const size_t nlanes = d->lanes.count();
  std::vector<uint16_t> crc(256);
  for (int v = 0; v < 256; ++v) {
    const uint8_t b = static_cast<uint8_t>(v);
    crc[v] = crc16_ccitt(&b, 1, 0);   // the CRC register after byte v from 0: the kernel's table-driven step
  }
  const size_t carry_bytes = nlanes * kPkCarry * kPkCell;
  bool good = d->fec.reserve(nsub) && d->sync.reserve(nlanes) && d->counters.reserve(nlanes * kPkCntN) && d->crc_tab.reserve(crc.size()) &&
              d->carry[0].reserve(carry_bytes) && d->carry[1].reserve(carry_bytes) && d->totals.reserve(4) &&
              d->nunits.reserve(nlanes) && d->lane_buf.reserve(nlanes) && d->ncar_in.reserve(nlanes) && d->ncar_out.reserve(nlanes) && d->lo.reserve(nlanes) &&
              d->lane_unit_base.reserve(nlanes + 1) && d->lane_buf_base.reserve(nlanes + 1);
  good = good && ok(hipMemcpy(d->fec.get(), fec_flags, static_cast<size_t>(nsub), hipMemcpyHostToDevice), "upload") &&
         ok(hipMemset(d->sync.get(), 0, sizeof(PacketSync) * nlanes), "clear") && ok(hipMemset(d->counters.get(), 0, sizeof(int64_t) * nlanes * kPkCntN), "clear") &&
         upload_rs_tables<kPkRoots>(f, d->gf) && ok(hipMemcpy(d->crc_tab.get(), crc.data(), crc.size() * 2, hipMemcpyHostToDevice), "upload");
  return good ? d.release() : nullptr;
}

extern "C" void dabhip_packet_destroy(dabhip_packet* d) { delete d; }

extern "C" int64_t dabhip_packet_push(dabhip_packet* d, const uint8_t* frames, const int64_t* counts, int on_device)
{
  if (!d || !counts) { set_error("packet_push: null argument"); return -1; }
  StageFrame<7>& f = d->f;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!f.use_device()) return -1;
  const int ns = d->lanes.nstreams, nsub = d->lanes.nsub;
  const EtiPush p = plan_eti_push("packet_push", counts, ns, !frames, 1 << 16, kEtiNoTotalBound);
  if (!p.refusal.empty()) { set_error(p.refusal); return -1; }
  EtiFrames fr;
  if (!f.place(p, frames, on_device, d->staging, d->meta, fr)) return -1;
  const size_t nlanes = d->lanes.count();
  const int maxv = p.maxv;
  // the units a lane can give in one push: its frames without FEC; with it, a frame per 103 of its carried and new cells (256 per ETI frame at
  // most) and one more for the frame a first run completes.  (Units never share a cell, so a lane gives floor((102 + 255 maxv) / 103) at most:
  // cap - 2 or less.  tests/host_sanitize/packet_units.cpp reaches exactly that over every rate, carried count and maxv of 1, 2, 3 and 64: at
  // worst 159 units in 162 slots, 0.981.)  The sync kernel flags a lane that passes cap all the same.
  const int cap = std::max(maxv, (kPkCarry + maxv * 256) / kPkFrameCells + 1) + 1;
  if (!d->loc.reserve(static_cast<size_t>(ns) * std::max(maxv, 1) * nsub) || !d->slots.reserve(nlanes * cap) || !d->units.reserve(nlanes * cap)) return -1;
  hipStream_t st = f.stream;
  const uint8_t* carry = d->carry[d->cur].get();
  int totals[4] = {0, 0, 0, 0};
  bool good = f.mark(0) && ok(launch_packet_locate(fr, d->lanes.subch.get(), nsub, ns, maxv, d->loc.get(), st), "locate") &&
              f.mark(1) && ok(hipMemsetAsync(d->totals.get(), 0, sizeof totals, st), "clear") &&
              ok(launch_packet_sync(fr, ns, nsub, maxv, d->fec.get(), d->loc.get(), d->sync.get(), carry, d->slots.get(), cap, d->nunits.get(), d->lane_buf.get(),
                                    d->ncar_in.get(), d->ncar_out.get(), d->lo.get(), d->counters.get(), d->units.get(), d->lane_unit_base.get(),
                                    d->lane_buf_base.get(), d->totals.get(), st), "sync") &&
              f.mark(2) && ok(hipMemcpyAsync(totals, d->totals.get(), sizeof totals, hipMemcpyDeviceToHost, st), "totals") &&
              ok(hipStreamSynchronize(st), "sync stage");
  if (!good) return -1;
  if (totals[3]) { set_error("packet_push: a lane gave more units than its slots hold; the handle's state is lost"); return -1; }
  d->n_units = totals[0];
  d->n_cells = totals[1];
  d->lanes.fetched = false;
  const int nu = totals[0], nc = totals[1];
  const size_t cu = static_cast<size_t>(nu ? nu : 1), cc = static_cast<size_t>(nc ? nc : 1);
  good = d->cells.reserve(cc * kPkCell) && d->cand.reserve(cc) && d->recs.reserve(cc) && d->cw_status.reserve(cu * kPkRows) && d->syn.reserve(cu * kPkRows * 4) &&
         ok(launch_packet_gather(fr, d->units.get(), d->totals.get(), nc, d->loc.get(), maxv, nsub, carry, d->ncar_in.get(), d->cells.get(), st), "gather") &&
         f.mark(3) && ok(launch_packet_rs(d->units.get(), d->totals.get(), nu, d->gf.get(), d->cells.get(), d->cw_status.get(), d->syn.get(), st), "rs") &&
         f.mark(4) && ok(launch_packet_cand(d->units.get(), d->totals.get(), nc, d->crc_tab.get(), d->cells.get(), d->cand.get(), st), "cand") &&
         f.mark(5) &&
         ok(launch_packet_walk(d->units.get(), d->totals.get(), nu, d->cells.get(), d->cand.get(), d->cw_status.get(), d->recs.get(), d->counters.get(),
                               d->totals.get() + 2, st), "walk") &&
         f.mark(6) &&
         ok(launch_packet_carry(fr, static_cast<int>(nlanes), d->loc.get(), maxv, nsub, carry, d->ncar_in.get(), d->ncar_out.get(), d->lo.get(),
                                d->carry[d->cur ^ 1].get(), st), "carry") &&
         f.mark(7) && ok(hipMemcpyAsync(totals, d->totals.get(), sizeof totals, hipMemcpyDeviceToHost, st), "totals") && f.finish();
  if (!good) return -1;
  d->cur ^= 1;
  return totals[2];
}

extern "C" int64_t dabhip_packet_records(const dabhip_packet* d, int stream, int sub, dabhip_packet_rec* out, int64_t cap)
{
  std::vector<dabhip_packet_rec> r;
  if (!d || !d->lane_cells(stream, sub, r, nullptr)) return -1;
  int64_t n = 0;
  for (const dabhip_packet_rec& x : r) {
    if (!x.length) continue;
    if (out && n < cap) out[n] = x;
    ++n;
  }
  return n;
}

extern "C" int64_t dabhip_packet_data(const dabhip_packet* d, int stream, int sub, uint8_t* dst, int64_t cap)
{
  std::vector<dabhip_packet_rec> r;
  std::vector<uint8_t> bytes;
  if (!d || !d->lane_cells(stream, sub, r, &bytes)) return -1;
  int64_t w = 0;
  for (size_t c = 0; c < r.size(); ++c) {
    if (!r[c].length) continue;
    const int64_t len = r[c].useful_length;
    if (dst && w + len <= cap) std::memcpy(dst + w, bytes.data() + c * kPkCell + 3, static_cast<size_t>(len));
    w += len;
  }
  return w;
}

extern "C" int dabhip_packet_stats(const dabhip_packet* d, int stream, int sub, int64_t* counters8)
{
  if (!d || !counters8) { set_error("packet_stats: null argument"); return -1; }
  return d->lanes.lane_counters(d->f, stream, sub, d->counters.get(), kPkCntN, counters8, kPkCntN);
}

extern "C" int dabhip_packet_stage_ms(const dabhip_packet* d, const char** names, float* ms, int cap)
{
  if (!d) return -1;
  return d->f.stage_ms(names, ms, cap);
}

// ---- data groups (host only) ----------------------------------------------------------------------------------------------------------------
struct dabhip_packet_groups {
  PacketGroups g;
};

extern "C" dabhip_packet_groups* dabhip_packet_groups_create(void) { return new dabhip_packet_groups; }
extern "C" void dabhip_packet_groups_destroy(dabhip_packet_groups* g) { delete g; }

extern "C" int64_t dabhip_packet_groups_push(dabhip_packet_groups* g, const dabhip_packet_rec* recs, int64_t nrecs, const uint8_t* data, int64_t ndata)
{
  if (!g || nrecs < 0 || ndata < 0 || (nrecs > 0 && !recs) || (ndata > 0 && !data)) { set_error("packet_groups_push: bad arguments"); return -1; }
  if (!g->g.push(recs, nrecs, data, ndata)) { set_error("packet_groups_push: fewer bytes than the records' useful lengths"); return -1; }
  return static_cast<int64_t>(g->g.done.size());
}

extern "C" int64_t dabhip_packet_groups_get(const dabhip_packet_groups* g, int64_t i, dabhip_packet_group* rec, uint8_t* dst, int64_t cap)
{
  if (!g || i < 0 || i >= static_cast<int64_t>(g->g.done.size())) { set_error("packet_groups_get: no such group"); return -1; }
  const std::vector<uint8_t>& b = g->g.done_bytes[static_cast<size_t>(i)];
  if (rec) *rec = g->g.done[static_cast<size_t>(i)];
  if (dst && cap > 0) std::memcpy(dst, b.data(), static_cast<size_t>(std::min<int64_t>(cap, static_cast<int64_t>(b.size()))));
  return static_cast<int64_t>(b.size());
}

extern "C" int dabhip_packet_groups_stats(const dabhip_packet_groups* g, int64_t* counters4)
{
  if (!g || !counters4) { set_error("packet_groups_stats: null argument"); return -1; }
  std::memcpy(counters4, g->g.counters, sizeof g->g.counters);
  return 0;
}
