// session.cpp — streaming sessions of the C ABI (include/dabhip.h: dabhip_stream_*).
// B parallel unbounded streams decoded segment by segment.  Per stream the session keeps device windows: segment k lives in
// window k % 3 behind a reserve of kWindowReserve bytes, and the bytes of earlier segments the front end may still read (FIFO
// backlog and stale-tail sources, Engine::stream_need_from) are copied in front of it from window (k - 1) % 3 when segment k is
// fed (session_windows.hpp has the arithmetic).  Three windows so that the NEXT segment (k + 1) can be uploading into its window -- which holds
// segment k - 2, dead since feed(k - 1) -- on a stream of its own while segment k decodes (dabhip_stream_prefetch).
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "capi_detail.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "session_windows.hpp"

using namespace dabhip;

namespace {
// room in front of every segment for the bytes of earlier segments K1 may still read: > FIFO capacity (1.5 MiB) + 12 nested stale tails of
// one TF each.  (DABHIP_WINDOW_RESERVE=bytes: test knob -- a small reserve sends every feed through the "more history than the reserve
// holds" path.)
const size_t kWindowReserve = [] {
  const char* env = std::getenv("DABHIP_WINDOW_RESERVE");
  const size_t v = env ? static_cast<size_t>(std::strtoull(env, nullptr, 10)) & ~size_t(255) : 0;
  return v ? v : size_t(8) << 20;
}();
}
struct dabhip_stream {
  Engine eng;
  int n = 0;
  bool first = true;
  std::vector<std::unique_ptr<DeviceBuffer<uint8_t>>> win[3];
  std::vector<WindowBook> book;                // per stream (session_windows.hpp)
  uint64_t fed = 0, queued = 0;                // segments fed / handed over (fed <= queued <= fed + 2)
  bool queued_ever = false;                    // dabhip_stream_prefetch has been used: its stream has work to forget (reap_stream)
  uint32_t up_uses = 0;
  // device-gather launches and the gathers they belong to: counted since the last feed returned, reported for the segment fed last (launch_limits.hpp)
  int64_t gather_launches = 0, gather_calls = 0, fed_gather_launches = 0, fed_gather_calls = 0;
  bool device_gather(const CopyDesc* descs, int count, uint32_t longest, hipStream_t st)
  {
    ++gather_calls;
    return launch_device_gather(descs, count, longest, st, eng.launch_limits().gather_descs, &gather_launches) == hipSuccess;
  }
  // A feed that fails after it has started to move the session on (windows, offsets, the engine's carried state) leaves a session nobody can
  // re-feed correctly: it is marked and refuses everything but its destruction -- an honest error instead of frames decoded at the wrong offsets.
  bool failed = false;
  bool resident = false;                       // fed through dabhip_stream_feed_resident: the caller's buffers are read in place, no windows
  // prefetch uploads run on ONE stream of their own.  Measured on the 256-stream workload, 8-TF segments (805 MB each): one gather kernel
  // per segment 56.5 GB/s, 256 copy commands on one stream 54.0, dealt to two / four streams 25 / 36 (they get in each other's way)
  hipStream_t up_stream = nullptr;
  hipEvent_t up_done[3] = {};                  // per window: its prefetch is through
  // upload by a gather kernel that reads the page-locked host segments over PCIe (one launch per segment instead of one copy command
  // per stream): descriptor lists, one per window, page-locked so that they go up asynchronously
  HostList<CopyDesc> gather_descs[3];
  DeviceBuffer<CopyDesc> d_gather_descs[3];
  struct Pending { std::vector<const uint8_t*> iq; std::vector<size_t> nbytes; };
  Pending pending[3];                          // what was prefetched into window i (checked against the feed that consumes it)
  dabhip_stream(int device, int nstreams, int host_threads = 0, std::vector<int> cpus = {})
      : eng(device, host_threads, std::move(cpus)), n(nstreams), book(nstreams)
  {
    for (int s = 0; s < 3; ++s)
      for (int b = 0; b < nstreams; ++b) win[s].emplace_back(new DeviceBuffer<uint8_t>());
    if (eng.ok()) {
      (void)hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking);
      for (auto& e : up_done) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
    }
  }
  ~dabhip_stream()
  {
    if (up_stream) (void)hipStreamSynchronize(up_stream);
    for (auto& e : up_done)
      if (e) (void)hipEventDestroy(e);
    if (up_stream) (void)hipStreamDestroy(up_stream);
  }
  bool ok() const { return eng.ok() && up_stream; }
  // window w of stream b, reserved for a segment of nbytes: where the segment goes (null: no memory)
  uint8_t* segment_room(int w, int b, size_t nbytes)
  {
    DeviceBuffer<uint8_t>& to = *win[w][b];
    return to.reserve(window_bytes(kWindowReserve, nbytes)) ? to.get() + kWindowReserve : nullptr;
  }
  // the same by ONE kernel launch on the upload stream, when every non-empty host segment is page-locked (device-visible): a small
  // persistent grid reads the host memory over PCIe (64 workgroups: 56.5 GB/s; 16: 54.5; 256: 43.8 -- and they would take CUs from the
  // decode running beside it).  DABHIP_PREFETCH_KERNEL=0 selects the copy engine instead, = N > 1 another grid size.
  bool upload_by_kernel(int w, const uint8_t* const* iq, const size_t* nbytes)
  {
    static const int mode = std::getenv("DABHIP_PREFETCH_KERNEL") ? std::atoi(std::getenv("DABHIP_PREFETCH_KERNEL")) : 1;
    if (mode <= 0) return false;
    HostList<CopyDesc>& descs = gather_descs[w];
    descs.clear();
    for (int b = 0; b < n; ++b) {
      if (nbytes[b] == 0) continue;
      if (!gather_fits(nbytes[b])) return false;
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, iq[b]) != hipSuccess || attr.type != hipMemoryTypeHost || !attr.devicePointer) { (void)hipGetLastError(); return false; }
      uint8_t* to = segment_room(w, b, nbytes[b]);
      if (!to) return false;
      const uint8_t* dev_view = static_cast<const uint8_t*>(attr.devicePointer) + (iq[b] - static_cast<const uint8_t*>(attr.hostPointer));
      descs.push_back(CopyDesc{dev_view, to, static_cast<uint32_t>(nbytes[b]), 0});
    }
    if (descs.empty()) return true;
    const int wgs = mode > 1 ? mode : 64;
    return d_gather_descs[w].upload(descs, up_stream) && launch_host_gather(d_gather_descs[w].get(), static_cast<int>(descs.size()), wgs, up_stream) == hipSuccess;
  }
  // segments that already are in device memory: one launch copies them all (256 copy commands cost 2.9 ms back to back and as much on the host)
  bool copy_by_kernel(int w, const uint8_t* const* iq, const size_t* nbytes, hipStream_t st)
  {
    HostList<CopyDesc>& descs = gather_descs[w];
    descs.clear();
    uint32_t longest = 0;
    for (int b = 0; b < n; ++b) {
      if (!gather_fits(nbytes[b])) return false;
      uint8_t* to = segment_room(w, b, nbytes[b]);
      if (!to) return false;
      if (nbytes[b] == 0) continue;
      descs.push_back(CopyDesc{iq[b], to, static_cast<uint32_t>(nbytes[b]), 0});
      longest = std::max(longest, static_cast<uint32_t>(nbytes[b]));
    }
    if (descs.empty()) return true;
    return d_gather_descs[w].upload(descs, st) && device_gather(d_gather_descs[w].get(), static_cast<int>(descs.size()), longest, st);
  }
  HostList<CopyDesc> history_descs;            // the bytes of earlier segments moved in front of the segment being fed (dabhip_stream_feed)
  DeviceBuffer<CopyDesc> d_history_descs;
  // segment -> window w of every stream, behind the reserve; on stream `one`, or (prefetch) on the upload stream
  bool upload(int w, const uint8_t* const* iq, const size_t* nbytes, bool on_device, hipStream_t one)
  {
    if (!one && !on_device && upload_by_kernel(w, iq, nbytes)) return true;
    hipStream_t st = one ? one : up_stream;
    if (on_device && copy_by_kernel(w, iq, nbytes, st)) return true;
    for (int b = 0; b < n; ++b) {
      uint8_t* to = segment_room(w, b, nbytes[b]);
      if (!to) return false;
      if (nbytes[b] && hipMemcpyAsync(to, iq[b], nbytes[b], on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("stream_feed: segment upload failed");
        return false;
      }
    }
    return true;
  }
};

namespace {
// what prefetch, feed and feed_resident refuse alike (`what`: the entry's name; for_resident: the entry that owns no windows; half_way: feed's longer text)
bool may_feed(const dabhip_stream* s, const char* what, const void* ptrs, const void* sizes, bool for_resident, const char* half_way = "")
{
  const std::string name(what);
  if (!s || !ptrs || !sizes) { set_error(name + ": null argument"); return false; }
  if (s->failed) { set_error(name + ": an earlier feed of this session failed half-way" + half_way + " -- destroy the session"); return false; }
  if (!for_resident && s->resident) { set_error(name + ": this session is fed through dabhip_stream_feed_resident"); return false; }
  if (for_resident && s->queued > 0) { set_error(name + ": this session is fed through dabhip_stream_feed (windows)"); return false; }
  return true;
}
}  // namespace

extern "C" {

dabhip_stream* dabhip_stream_create(int device, int nstreams) { return dabhip_stream_create_on_cpus(device, nstreams, 0, nullptr, 0); }
// the same with the host side chosen by the caller (dabhip_multi_stream_create: one session per device, each on the CPUs of its device's NUMA node)
dabhip_stream* dabhip_stream_create_on_cpus(int device, int nstreams, int host_threads, const int32_t* cpus, int ncpus)
{
  if (nstreams <= 0) { set_error("stream_create: no streams"); return nullptr; }
  std::vector<int> list;
  for (int i = 0; cpus && i < ncpus; ++i) list.push_back(cpus[i]);
  dabhip_stream* s = new dabhip_stream(device, nstreams, host_threads, list);
  if (!s->ok()) { delete s; return nullptr; }
  return s;
}
void dabhip_stream_destroy(dabhip_stream* s) { delete s; }
int dabhip_stream_set_subchannels(dabhip_stream* s, const int32_t* ids, int n)
{
  if (!s) return -1;
  if (!s->first) { set_error("stream_set_subchannels: only before the first segment"); return -1; }
  s->eng.set_subchannel_filter(subchannel_mask(ids, n));
  return 0;
}
int dabhip_stream_set_tii(dabhip_stream* s, int on) { if (!s) return -1; s->eng.set_tii(on != 0); return 0; }
int dabhip_stream_tii_sums(dabhip_stream* s, int stream, uint64_t* T, int* frames)
{
  if (!s || stream < 0 || stream >= s->n) { set_error("stream_tii_sums: bad argument"); return -1; }
  return s->eng.tii_sums(stream, T, frames) ? 0 : -1;
}
int dabhip_stream_tii(dabhip_stream* s, int stream, dabhip_tii_id* out, int cap)
{
  uint64_t T[DABHIP_TII_SUMS];
  if (cap < 0 || (!out && cap > 0)) { set_error("stream_tii: bad argument"); return -1; }
  if (dabhip_stream_tii_sums(s, stream, T, nullptr) != 0) return -1;
  return dabhip_tii_detect(T, out, cap);
}
int dabhip_stream_tii_reset(dabhip_stream* s)
{
  if (!s) { set_error("stream_tii_reset: null handle"); return -1; }
  return s->eng.tii_reset() ? 0 : -1;
}
int dabhip_stream_set_afc(dabhip_stream* s, int on) { if (!s) return -1; s->eng.set_afc(on != 0); return 0; }
int dabhip_stream_set_parity_guard(dabhip_stream* s, int on) { if (!s) return -1; s->eng.set_parity_guard(on); return 0; }
int dabhip_stream_set_sync_speculation(dabhip_stream* s, int mode) { if (!s) return -1; s->eng.set_sync_speculation(mode); return 0; }
int dabhip_stream_set_demod_all(dabhip_stream* s, int on) { if (!s) return -1; s->eng.set_demod_all(on != 0); return 0; }
int dabhip_stream_msc_deferred(const dabhip_stream* s) { return s ? s->eng.msc_deferred() : -1; }
int dabhip_stream_set_launch_limits(dabhip_stream* s, const int64_t* limits, int n)
{
  if (!s || !limits || n != kLaunchLimitCount) { set_error("stream_set_launch_limits: bad argument"); return -1; }
  return s->eng.set_launch_limits(limits) ? 0 : -1;
}
int dabhip_stream_launch_report(const dabhip_stream* s, int64_t* out, int cap)
{
  if (!s || !out || cap < 0) { set_error("stream_launch_report: bad argument"); return -1; }
  LaunchReport r = s->eng.launch_report();
  r.gather = s->fed_gather_launches;
  r.gather_calls = s->fed_gather_calls;
  return report_to_words(r, out, cap);
}
int dabhip_stream_set_soft(dabhip_stream* s, int on)
{
  if (!s) return -1;
  if (!s->first) { set_error("stream_set_soft: only before the first segment"); return -1; }
  s->eng.set_soft(on != 0);
  return 0;
}
int dabhip_stream_set_soft_lanes(dabhip_stream* s, int on)
{
  if (!s) { set_error("stream_set_soft_lanes: null handle"); return -1; }
  s->eng.set_soft_lanes(on != 0);
  return 0;
}

// Start uploading a segment that a LATER dabhip_stream_feed will consume, and return at once.  Host segments must live in
// page-locked memory (dabhip_host_alloc) for the copy to be a true asynchronous DMA; they must stay untouched until the feed
// that consumes them has returned.
int dabhip_stream_prefetch(dabhip_stream* s, const uint8_t* const* iq, const size_t* nbytes, int on_device)
{
  if (!may_feed(s, "stream_prefetch", iq, nbytes, false)) return -1;
  if (s->queued - s->fed >= 2) { set_error("stream_prefetch: two segments are already waiting to be fed"); return -1; }
  if (hipSetDevice(s->eng.device()) != hipSuccess) { set_error("stream_prefetch: hipSetDevice failed"); return -1; }
  const int w = static_cast<int>(s->queued % 3);
  if (!s->upload(w, iq, nbytes, on_device != 0, nullptr)) return -1;
  if (hipEventRecord(s->up_done[w], s->up_stream) != hipSuccess) { set_error("stream_prefetch: event record failed"); return -1; }
  s->pending[w].iq.assign(iq, iq + s->n);
  s->pending[w].nbytes.assign(nbytes, nbytes + s->n);
  ++s->queued;
  s->queued_ever = true;
  return 0;
}

// upload (or the wait for the prefetched upload), the windows' plan, its application -- reserve or grow, one gather launch for all streams' history --, Engine::feed
int64_t dabhip_stream_feed(dabhip_stream* s, const uint8_t* const* iq, const size_t* nbytes, int on_device)
{
  if (!may_feed(s, "stream_feed", iq, nbytes, false, "; its state is not trustworthy any more")) return -1;
  if (hipSetDevice(s->eng.device()) != hipSuccess) { set_error("stream_feed: hipSetDevice failed"); return -1; }
  auto broken = [s](const char* msg) -> int64_t {          // from here on an error leaves the session's books half-updated
    s->failed = true;
    if (msg) set_error(msg);
    return -1;
  };
  const int w = static_cast<int>(s->fed % 3), wprev = static_cast<int>((s->fed + 2) % 3);
  hipStream_t st = s->eng.stream();
  if (s->queued > s->fed) {                    // this segment was prefetched: it must be the one handed over first
    const dabhip_stream::Pending& p = s->pending[w];
    for (int b = 0; b < s->n; ++b)
      if (p.iq[b] != iq[b] || p.nbytes[b] != nbytes[b]) { set_error("stream_feed: not the segment that was prefetched first"); return -1; }
    if (hipStreamWaitEvent(st, s->up_done[w], 0) != hipSuccess) { set_error("stream_feed: event wait failed"); return -1; }
  } else {
    if (!s->upload(w, iq, nbytes, on_device != 0, st)) return broken(nullptr);
    ++s->queued;
  }
  std::vector<const uint8_t*> virt(s->n);
  std::vector<size_t> avail(s->n);
  HostList<CopyDesc>& moves = s->history_descs;
  moves.clear();
  uint32_t longest_move = 0;
  for (int b = 0; b < s->n; ++b) {
    const WindowPlan p = plan_window(s->book[b], s->first, s->eng.stream_need_from(b), nbytes[b], kWindowReserve);
    if (p.refused) return broken(p.refused);
    if (p.grow) {                               // the segment, uploaded behind the reserve, moves into a larger window
      std::unique_ptr<DeviceBuffer<uint8_t>> big(new DeviceBuffer<uint8_t>());
      if (!big->reserve(p.grow_bytes)) return broken(nullptr);
      if (nbytes[b] && hipMemcpyAsync(big->get() + p.at, s->win[w][b]->get() + kWindowReserve, nbytes[b], hipMemcpyDeviceToDevice, st) != hipSuccess) return broken("stream_feed: window move failed");
      if (hipStreamSynchronize(st) != hipSuccess) return broken("stream_feed: window move failed");      // (the old window goes: nothing may still read it)
      s->win[w][b] = std::move(big);
    }
    uint8_t* to = s->win[w][b]->get();
    if (p.kept) {                               // all streams' moves go in one launch behind the loop
      moves.push_back(CopyDesc{s->win[wprev][b]->get() + p.move_from, to + p.move_to, static_cast<uint32_t>(p.kept), 0});
      longest_move = std::max(longest_move, static_cast<uint32_t>(p.kept));
    }
    s->book[b] = p.book;
    virt[b] = to + p.virtual_base;              // byte x of the stream lives at virt[b][x]
    avail[b] = static_cast<size_t>(p.book.avail);
  }
  if (!moves.empty() && !(s->d_history_descs.upload(moves, st) &&
                          s->device_gather(s->d_history_descs.get(), static_cast<int>(moves.size()), longest_move, st)))
    return broken("stream_feed: window move failed");
  ++s->fed;
  s->fed_gather_launches = s->gather_launches;
  s->fed_gather_calls = s->gather_calls;
  s->gather_launches = s->gather_calls = 0;
  const int64_t frames = s->eng.feed(virt.data(), avail.data(), s->n, s->first);
  if (frames < 0) return broken(nullptr);        // (the engine's error text stands)
  // the prefetch stream is only ever waited for through events (hip_util.hpp: blocking_copy): every 32nd segment, wait for the stream itself -- at
  // most the upload of the next segment, which the next feed needs anyway
  if (s->queued_ever && ++s->up_uses % kReapEvery == 0 && reap_enabled()) (void)hipStreamSynchronize(s->up_stream);
  s->first = false;
  return frames;
}
// A session over streams that LIVE in device memory, without any copy: base[b][x] is byte x of stream b counted from the session's start, of which
// the first avail[b] are there now (avail never shrinks).  The caller keeps the bytes from dabhip_stream_need_from(s, b) on in place -- a linear
// buffer that is appended to -- and may recycle what lies below.  base may change between calls as long as those bytes stay addressable through it.
// Not to be mixed with dabhip_stream_feed / _prefetch on the same session (those own their windows).
int64_t dabhip_stream_feed_resident(dabhip_stream* s, const uint8_t* const* base, const size_t* avail)
{
  if (!may_feed(s, "stream_feed_resident", base, avail, true)) return -1;
  if (hipSetDevice(s->eng.device()) != hipSuccess) { set_error("stream_feed_resident: hipSetDevice failed"); return -1; }
  for (int b = 0; b < s->n; ++b)
    if (static_cast<int64_t>(avail[b]) < s->book[b].avail) { set_error("stream_feed_resident: a stream's byte count went down"); return -1; }
  if (s->first)                                // the kernels dereference these addresses: a host pointer here would be a fault on the device, not an error code
    for (int b = 0; b < s->n; ++b) {
      if (avail[b] == 0) continue;
      hipPointerAttribute_t attr;
      if (hipPointerGetAttributes(&attr, base[b]) != hipSuccess || (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)) {
        (void)hipGetLastError();
        set_error("stream_feed_resident: base[" + std::to_string(b) + "] is not device memory");
        return -1;
      }
    }
  const int64_t frames = s->eng.feed(base, avail, s->n, s->first);
  if (frames < 0) { s->failed = true; return -1; }     // (the engine's error text stands)
  for (int b = 0; b < s->n; ++b) s->book[b].avail = static_cast<int64_t>(avail[b]);
  s->resident = true;
  s->first = false;
  return frames;
}
// oldest byte of stream b a later segment may still read (FIFO backlog and stale-tail sources of the front end): everything below may go
int64_t dabhip_stream_need_from(const dabhip_stream* s, int stream)
{
  if (!s || stream < 0 || stream >= s->n) return -1;
  return window_need_from(s->first, s->eng.stream_need_from(stream), s->book[stream].avail);
}
int64_t dabhip_stream_eti_count(const dabhip_stream* s, int stream) { return s ? s->eng.eti_count(stream) : -1; }
// stage times of the segment fed last (the names of dabhip_engine_stage_ms; "wall" = the engine's part of the feed, without the window moves)
int dabhip_stream_stage_ms(const dabhip_stream* s, const char** names, float* ms, int cap)
{
  if (!s) return -1;
  static const char* kNames[13] = {"sync", "fft", "demap", "fic", "control", "gather", "viterbi", "eti", "host_setup", "host_frames", "host_worklist", "wall",
                                   "sync_spec_calls"};
  const StageTimes& t = s->eng.stage_times();
  const float v[13] = {t.sync, t.fft, t.demap, t.fic, t.control, t.gather, t.viterbi, t.eti, t.setup, t.frames, t.worklist, t.wall, t.sync_spec_calls};
  int n = 0;
  for (; n < 13 && n < cap; ++n) {
    if (names) names[n] = kNames[n];
    if (ms) ms[n] = v[n];
  }
  return n;
}
uint32_t dabhip_stream_status(const dabhip_stream* s, int stream) { return s ? s->eng.stream_status(stream) : 0xffffffffu; }
int64_t dabhip_stream_log(dabhip_stream* s, int stream, char* buf, int64_t cap)
{
  if (!s || stream < 0 || stream >= s->n) return -1;
  return hand_over_text(s->eng.take_stream_log(stream), buf, cap);
}
int64_t dabhip_stream_eti_read(dabhip_stream* s, int stream, uint8_t* dst, int64_t cap_frames)
{
  if (!s || !dst) { set_error("stream_eti_read: null argument"); return -1; }
  return s->eng.eti_read(stream, dst, cap_frames);
}
int64_t dabhip_stream_eti_fetch(dabhip_stream* s, uint8_t* dst, int64_t cap_frames)
{
  if (!s) { set_error("stream_eti_fetch: null handle"); return -1; }
  return s->eng.eti_fetch_async(dst, cap_frames);
}
int dabhip_stream_eti_fetch_wait(dabhip_stream* s)
{
  if (!s) { set_error("stream_eti_fetch_wait: null handle"); return -1; }
  return s->eng.eti_fetch_wait() ? 0 : -1;
}
int64_t dabhip_stream_eti_drain(dabhip_stream* s, dabhip_eti_sink sink, void* user)
{
  if (!s || !sink) { set_error("stream_eti_drain: null argument"); return -1; }
  return drain_eti(s->n, sink, user, false, [s](int b) { return s->eng.eti_count(b); },
                   [s](int b, uint8_t* dst, int64_t n) { return s->eng.eti_read(b, dst, n); });
}

}  // extern "C"
