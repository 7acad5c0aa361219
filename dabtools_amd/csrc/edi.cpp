// edi.cpp — dabhip_edi: the stateful consumer of ETI frames that repackages them as EDI packets (dabhip.h).  Each push runs the kernels of
// k_edi.hip on its own HIP stream over the frames where they lie (device) or after one upload (host); between pushes it keeps 24 bytes of
// state per stream on the device.  The packets, their records and the counters stay on the device until asked for.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "edi.hpp"
#include "stage_frame.hpp"

using namespace dabhip;

namespace {
constexpr int kNStages = 5;
const char* const kStages[kNStages] = {"plan", "scan", "assemble", "rs", "fragment"};
constexpr int64_t kMaxPushFrames = 1 << 17;              // 6656 bytes of work buffer per frame: 872 MB at this bound

const char* const kRefusal[5] = {"", "l out of range (13 .. 2^20)", "mode out of range (0 .. 2)", "recover out of range (0 .. 5)", "max_frag out of range (64 .. 1472)"};
}  // namespace

struct dabhip_edi {
  int nstreams = 0;
  EdiConfig cfg = {};
  DeviceBuffer<EdiState> state;
  DeviceBuffer<int64_t> counters, sums, bases;
  DeviceBuffer<uint8_t> table;
  DeviceBuffer<uint8_t> staging;
  DeviceBuffer<uint8_t> meta;                            // base (int64) | nnew (int), per stream
  DeviceBuffer<EdiFrame> frames;
  DeviceBuffer<uint8_t> work, parity, out;
  DeviceBuffer<dabhip_edi_rec> recs;
  std::vector<int64_t> h_bases;                          // of the last push: packets and bytes in front of every stream, the totals last
  StageFrame<kNStages> f{"edi", kStages};

  bool stream_ok(int s) const
  {
    if (s < 0 || s >= nstreams) { set_error("edi: no such stream"); return false; }
    return true;
  }
  EdiState initial() const { return EdiState{0, 0, 0, 0, cfg.seq0}; }
};

extern "C" int dabhip_edi_plan(int64_t l, int mode, int recover, int max_frag, dabhip_edi_sizes* out)
{
  if (!out) { set_error("edi_plan: null argument"); return -1; }
  const int bad = edi_plan_check(l, mode, recover, max_frag);
  if (bad) { set_error(std::string("edi_plan: ") + kRefusal[bad]); return -bad; }
  const EdiPlan p = edi_plan(static_cast<int32_t>(l), mode, recover, max_frag);
  *out = dabhip_edi_sizes{p.c, p.k, p.z, p.B, p.f, p.s};
  return 0;
}

extern "C" dabhip_edi* dabhip_edi_create(int device, int nstreams, int mode, int recover, int max_frag, int seq0)
{
  std::unique_ptr<dabhip_edi> d(new dabhip_edi);
  StageFrame<kNStages>& f = d->f;
  if (!f.open(device, "no HIP device: the EDI stage runs on the GPU only", "edi_create: device index out of range")) return nullptr;
  if (nstreams <= 0 || nstreams > (1 << 16) || seq0 < 0 || seq0 > 0xFFFF) { set_error("edi_create: bad arguments"); return nullptr; }
  const int bad = edi_plan_check(kEdiMinL, mode, recover, max_frag);
  if (bad) { set_error(std::string("edi_create: ") + kRefusal[bad]); return nullptr; }
  d->nstreams = nstreams;
  d->cfg = EdiConfig{mode, mode == 2 ? recover : 0, mode ? max_frag : 0, seq0};
  const size_t ns = static_cast<size_t>(nstreams);
  std::vector<EdiState> st(ns, d->initial());
  std::vector<uint8_t> table(256 * kEdiRsP);
  edi_rs_table_fill(table.data());
  d->h_bases.assign(2 * ns + 2, 0);
  const bool good = d->state.reserve(ns) && d->counters.reserve(ns * kEdiCntN) && d->sums.reserve(2 * ns) && d->bases.reserve(2 * ns + 2) &&
                    d->table.reserve(table.size()) && f.ok(hipMemcpy(d->state.get(), st.data(), sizeof(EdiState) * ns, hipMemcpyHostToDevice), "upload") &&
                    f.ok(hipMemset(d->counters.get(), 0, sizeof(int64_t) * ns * kEdiCntN), "clear") &&
                    f.ok(hipMemcpy(d->table.get(), table.data(), table.size(), hipMemcpyHostToDevice), "upload");
  return good ? d.release() : nullptr;
}

extern "C" void dabhip_edi_destroy(dabhip_edi* d) { delete d; }

extern "C" int64_t dabhip_edi_push(dabhip_edi* d, const uint8_t* frames, const int64_t* counts, int on_device)
{
  if (!d || !counts) { set_error("edi_push: null argument"); return -1; }
  StageFrame<kNStages>& f = d->f;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!f.use_device()) return -1;
  const int ns = d->nstreams;
  const EtiPush p = plan_eti_push("edi_push", counts, ns, !frames, kMaxPushFrames, kMaxPushFrames);
  if (!p.refusal.empty()) { set_error(p.refusal); return -1; }
  EtiFrames fr;
  if (!f.place(p, frames, on_device, d->staging, d->meta, fr)) return -1;
  const int64_t total = p.total;
  const int maxv = p.maxv;
  const size_t nf = static_cast<size_t>(std::max<int64_t>(total, 1));
  if (!d->frames.reserve(nf) || !d->work.reserve(nf * kEdiWorkStride) || (d->cfg.mode == 2 && !d->parity.reserve(nf * kEdiMaxChunks * kEdiRsP))) return -1;
  hipStream_t st = f.stream;
  std::vector<int64_t>& hb = d->h_bases;
  bool good = f.mark(0) && ok(launch_edi_plan(fr, d->cfg, ns, maxv, d->frames.get(), st), "plan") && f.mark(1) &&
              ok(launch_edi_scan(fr, d->cfg, ns, d->frames.get(), d->state.get(), d->counters.get(), d->sums.get(), d->bases.get(), st), "scan") && f.mark(2) &&
              ok(hipMemcpyAsync(hb.data(), d->bases.get(), sizeof(int64_t) * hb.size(), hipMemcpyDeviceToHost, st), "totals") && ok(hipStreamSynchronize(st), "scan stage");
  if (!good) return -1;
  const int64_t npackets = hb[2 * static_cast<size_t>(ns)], nbytes = hb[2 * static_cast<size_t>(ns) + 1];
  good = d->out.reserve(static_cast<size_t>(std::max<int64_t>(nbytes, 1))) && d->recs.reserve(static_cast<size_t>(std::max<int64_t>(npackets, 1))) &&
         ok(launch_edi_assemble(fr, total, d->frames.get(), d->work.get(), st), "assemble") && f.mark(3) &&
         (d->cfg.mode != 2 || ok(launch_edi_rs(total, d->frames.get(), d->table.get(), d->work.get(), d->parity.get(), st), "rs")) && f.mark(4) &&
         ok(launch_edi_fragment(d->cfg, total, d->frames.get(), d->bases.get(), d->work.get(), d->parity.get(), d->out.get(), d->recs.get(), st), "fragment") &&
         f.mark(5) && f.finish();
  if (!good) {
    std::fill(hb.begin(), hb.end(), 0);
    return -1;
  }
  return npackets;
}

extern "C" int64_t dabhip_edi_records(const dabhip_edi* d, int stream, dabhip_edi_rec* out, int64_t cap)
{
  if (!d) { set_error("edi_records: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  const int64_t a = d->h_bases[2 * static_cast<size_t>(stream)], n = d->h_bases[2 * static_cast<size_t>(stream) + 2] - a;
  const int64_t take = out ? std::min(n, std::max<int64_t>(cap, 0)) : 0;
  if (take > 0 && !d->f.ok(blocking_copy(out, d->recs.get() + a, sizeof(dabhip_edi_rec) * static_cast<size_t>(take), hipMemcpyDeviceToHost), "records")) return -1;
  return n;
}

extern "C" int64_t dabhip_edi_data(const dabhip_edi* d, int stream, uint8_t* dst, int64_t cap)
{
  if (!d) { set_error("edi_data: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  const int64_t a = d->h_bases[2 * static_cast<size_t>(stream) + 1], n = d->h_bases[2 * static_cast<size_t>(stream) + 3] - a;
  const int64_t take = dst ? std::min(n, std::max<int64_t>(cap, 0)) : 0;
  if (take > 0 && !d->f.ok(blocking_copy(dst, d->out.get() + a, static_cast<size_t>(take), hipMemcpyDeviceToHost), "data")) return -1;
  return n;
}

extern "C" int dabhip_edi_reset(dabhip_edi* d, int stream)
{
  if (!d) { set_error("edi_reset: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  // the frame numbers go on: everything behind EdiState::frames returns to its first value
  const EdiState init = d->initial();
  const size_t skip = sizeof(int64_t);
  return d->f.ok(blocking_copy(reinterpret_cast<uint8_t*>(d->state.get() + stream) + skip, reinterpret_cast<const uint8_t*>(&init) + skip, sizeof(EdiState) - skip,
                               hipMemcpyHostToDevice), "reset") ? 0 : -1;
}

extern "C" int dabhip_edi_stats(const dabhip_edi* d, int stream, int64_t* counters6)
{
  if (!d || !counters6) { set_error("edi_stats: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  return d->f.ok(blocking_copy(counters6, d->counters.get() + static_cast<size_t>(stream) * kEdiCntN, sizeof(int64_t) * kEdiCntN, hipMemcpyDeviceToHost), "counters") ? 0 : -1;
}

extern "C" int dabhip_edi_stage_ms(const dabhip_edi* d, const char** names, float* ms, int cap)
{
  if (!d) return -1;
  return d->f.stage_ms(names, ms, cap);
}
