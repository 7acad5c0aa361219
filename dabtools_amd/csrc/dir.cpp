// dir.cpp — dabhip_dir: the stateful consumer of ETI frames that keeps the ensemble directory (dabhip.h).  Each push runs the two kernels of
// k_dir.hip on its own HIP stream over the frames where they lie (device) or after one upload (host).  The tables and the counters stay on the
// device; a query fetches the one stream it asks about (17 KB) and turns the kept facts into the public records with dir_figs.hpp.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "dir.hpp"
#include "kernels.hpp"
#include "stage_frame.hpp"

using namespace dabhip;

namespace {
constexpr int kNStages = 2;
const char* const kStages[kNStages] = {"fibs", "merge"};
constexpr int64_t kMaxPushFrames = 1 << 16;              // 3840 bytes of fact slots per frame: 252 MB at this bound
}

struct dabhip_dir {
  int nstreams = 0;
  DeviceBuffer<DirStream> state;
  DeviceBuffer<uint8_t> staging;
  DeviceBuffer<uint8_t> meta;                            // base (int64) | nnew (int), per stream
  DeviceBuffer<DirFib> fibs;
  DeviceBuffer<DirFact> facts;
  DeviceBuffer<int> ok_fibs;
  std::vector<int> h_ok;
  // the one stream last asked about, as the public records
  mutable int cached = -1;
  mutable std::unique_ptr<DirStream> h;
  mutable dabhip_dir_ensemble_rec ens;
  mutable std::vector<dabhip_dir_subch> sub;
  mutable std::vector<dabhip_dir_service> svc;
  mutable std::vector<dabhip_dir_pktcomp> pkt;
  StageFrame<kNStages> f{"dir", kStages};

  bool stream_ok(int s) const
  {
    if (s < 0 || s >= nstreams) { set_error("dir: no such stream"); return false; }
    return true;
  }

  bool fetch(int s) const
  {
    if (!stream_ok(s)) return false;
    if (cached == s) return true;
    if (!f.use_device()) return false;
    if (!h) h.reset(new DirStream);
    cached = -1;
    if (!f.ok(blocking_copy(h.get(), state.get() + s, sizeof(DirStream), hipMemcpyDeviceToHost), "tables")) return false;
    const DirEntry* e = h->e;
    std::memset(&ens, 0, sizeof ens);
    int have = 0;
    for (int k = 0; k < kDirEnsEntries; ++k) have |= (e[k].have & 1) << k;
    dir_ensemble_from(e[0].part0, e[1].part0, e[2].part0, e[3].part0, have, &ens);
    ens.time_frame = (have & DABHIP_DIR_HAVE_10) ? e[2].last : -1;
    bool any = false;
    for (int k = 0; k < kDirEnsEntries; ++k) {
      if (!e[k].have) continue;
      ens.first_frame = any ? std::min(ens.first_frame, e[k].first) : e[k].first;
      ens.last_frame = any ? std::max(ens.last_frame, e[k].last) : e[k].last;
      ens.changes += e[k].changes;
      any = true;
    }
    sub.clear();
    svc.clear();
    pkt.clear();
    for (int id = 0; id < kDirTable; ++id) {
      const DirEntry& x = e[kDirSubBase + id];
      if (!x.have) continue;
      dabhip_dir_subch o;
      std::memset(&o, 0, sizeof o);
      dir_subch_from(x.part0, x.part1, x.have, id, &o);
      o.first_frame = x.first; o.last_frame = x.last; o.changes = x.changes;
      sub.push_back(o);
    }
    for (int i = 0; i < std::min(h->nsvc, kDirTable); ++i) {
      const DirEntry& x = e[kDirSvcBase + i];
      dabhip_dir_service o;
      std::memset(&o, 0, sizeof o);
      dir_service_from(x.part0, x.part1, x.have, x.pd, x.key, &o);
      o.first_frame = x.first; o.last_frame = x.last; o.changes = x.changes;
      svc.push_back(o);
    }
    for (int i = 0; i < std::min(h->npkt, kDirTable); ++i) {
      const DirEntry& x = e[kDirPktBase + i];
      dabhip_dir_pktcomp o;
      std::memset(&o, 0, sizeof o);
      dir_pktcomp_from(x.part0, x.key, &o);
      o.first_frame = x.first; o.last_frame = x.last; o.changes = x.changes;
      pkt.push_back(o);
    }
    cached = s;
    return true;
  }

  DirView view() const { return DirView{&ens, sub.data(), static_cast<int>(sub.size()), svc.data(), static_cast<int>(svc.size()), pkt.data(), static_cast<int>(pkt.size())}; }
};

extern "C" dabhip_dir* dabhip_dir_create(int device, int nstreams)
{
  std::unique_ptr<dabhip_dir> d(new dabhip_dir);
  StageFrame<kNStages>& f = d->f;
  if (!f.open(device, "no HIP device: the ensemble directory is built on the GPU only", "dir_create: device index out of range")) return nullptr;
  if (nstreams <= 0 || nstreams > (1 << 16)) { set_error("dir_create: bad arguments"); return nullptr; }
  d->nstreams = nstreams;
  d->h_ok.assign(static_cast<size_t>(nstreams), 0);
  const bool good = d->state.reserve(static_cast<size_t>(nstreams)) && d->ok_fibs.reserve(static_cast<size_t>(nstreams)) &&
                    f.ok(hipMemset(d->state.get(), 0, sizeof(DirStream) * static_cast<size_t>(nstreams)), "clear");
  return good ? d.release() : nullptr;
}

extern "C" void dabhip_dir_destroy(dabhip_dir* d) { delete d; }

extern "C" int64_t dabhip_dir_push(dabhip_dir* d, const uint8_t* frames, const int64_t* counts, int on_device)
{
  if (!d || !counts) { set_error("dir_push: null argument"); return -1; }
  StageFrame<kNStages>& f = d->f;
  const auto ok = [&f](hipError_t e, const char* what) { return f.ok(e, what); };
  if (!f.use_device()) return -1;
  const int ns = d->nstreams;
  const EtiPush p = plan_eti_push("dir_push", counts, ns, !frames, kMaxPushFrames, kMaxPushFrames);
  if (!p.refusal.empty()) { set_error(p.refusal); return -1; }
  EtiFrames fr;
  if (!f.place(p, frames, on_device, d->staging, d->meta, fr)) return -1;
  const size_t nfib = static_cast<size_t>(std::max<int64_t>(p.total, 1)) * 3;
  if (!d->fibs.reserve(nfib) || !d->facts.reserve(nfib * kDirFactSlots)) return -1;
  d->cached = -1;
  const bool good = f.mark(0) && ok(launch_dir_fibs(fr, ns, p.maxv, d->fibs.get(), d->facts.get(), f.stream), "fibs") && f.mark(1) &&
                    ok(launch_dir_merge(fr, ns, d->fibs.get(), d->facts.get(), d->state.get(), d->ok_fibs.get(), f.stream), "merge") && f.mark(2) &&
                    ok(hipMemcpyAsync(d->h_ok.data(), d->ok_fibs.get(), sizeof(int) * ns, hipMemcpyDeviceToHost, f.stream), "counts") && f.finish();
  if (!good) return -1;
  int64_t n = 0;
  for (int s = 0; s < ns; ++s) n += d->h_ok[s];
  return n;
}

extern "C" int dabhip_dir_ensemble(const dabhip_dir* d, int stream, dabhip_dir_ensemble_rec* out)
{
  if (!d || !out) { set_error("dir_ensemble: null argument"); return -1; }
  if (!d->fetch(stream)) return -1;
  *out = d->ens;
  return 0;
}

namespace {
template <class T>
int copy_out(const std::vector<T>& v, T* out, int cap)
{
  const int n = static_cast<int>(v.size());
  if (out && cap > 0) std::copy_n(v.begin(), std::min(n, cap), out);
  return n;
}
}  // namespace

extern "C" int dabhip_dir_subchannels(const dabhip_dir* d, int stream, dabhip_dir_subch* out, int cap)
{
  if (!d) { set_error("dir_subchannels: null argument"); return -1; }
  return d->fetch(stream) ? copy_out(d->sub, out, cap) : -1;
}

extern "C" int dabhip_dir_services(const dabhip_dir* d, int stream, dabhip_dir_service* out, int cap)
{
  if (!d) { set_error("dir_services: null argument"); return -1; }
  return d->fetch(stream) ? copy_out(d->svc, out, cap) : -1;
}

extern "C" int dabhip_dir_packet_components(const dabhip_dir* d, int stream, dabhip_dir_pktcomp* out, int cap)
{
  if (!d) { set_error("dir_packet_components: null argument"); return -1; }
  return d->fetch(stream) ? copy_out(d->pkt, out, cap) : -1;
}

extern "C" int dabhip_dir_complete(const dabhip_dir* d, int stream)
{
  if (!d) { set_error("dir_complete: null argument"); return -1; }
  if (!d->fetch(stream)) return -1;
  return dir_complete(d->view()) ? 1 : 0;
}

extern "C" int dabhip_dir_resolve(const dabhip_dir* d, int stream, int pd, uint32_t sid, int component, dabhip_dir_target* out)
{
  if (!d || !out) { set_error("dir_resolve: null argument"); return -1; }
  if (!d->fetch(stream)) return -1;
  const int r = dir_resolve(d->view(), pd, sid, component, out);
  if (r != 0)
    set_error(r == DABHIP_DIR_NO_SERVICE ? "dir_resolve: no such service" : r == DABHIP_DIR_NO_COMPONENT ? "dir_resolve: the service has no such component" :
              r == DABHIP_DIR_NO_PKTCOMP ? "dir_resolve: no FIG 0/3 for the component's SCId" : "dir_resolve: no FIG 0/1 for the component's sub-channel");
  return r;
}

extern "C" int dabhip_dir_reset(dabhip_dir* d, int stream)
{
  if (!d) { set_error("dir_reset: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  d->cached = -1;
  return d->f.ok(hipMemsetAsync(d->state.get() + stream, 0, kDirTablesBytes, d->f.stream), "reset") && d->f.ok(hipStreamSynchronize(d->f.stream), "reset") ? 0 : -1;
}

extern "C" int dabhip_dir_stats(const dabhip_dir* d, int stream, int64_t* counters11)
{
  if (!d || !counters11) { set_error("dir_stats: null argument"); return -1; }
  if (!d->stream_ok(stream) || !d->f.use_device()) return -1;
  return d->f.ok(blocking_copy(counters11, d->state.get()[stream].counters, sizeof(int64_t) * kDirCntN, hipMemcpyDeviceToHost), "counters") ? 0 : -1;
}

extern "C" int dabhip_dir_stage_ms(const dabhip_dir* d, const char** names, float* ms, int cap)
{
  if (!d) return -1;
  return d->f.stage_ms(names, ms, cap);
}
