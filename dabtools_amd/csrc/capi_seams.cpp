// capi_seams.cpp — the reference's streaming seams of the C ABI (include/dabhip.h): S2 sdr_demod (dabhip_sdr) and S3 dab_process_frame (dabhip_dab)
// as single-stream shims over the same HIP kernels the batch engine uses.  S1 (viterbi) and the batch handle: capi_engine.cpp.
#include <cstring>
#include <new>
#include <vector>

#include "capi_detail.hpp"
#include "engine.hpp"
#include "fifo_view.hpp"

using namespace dabhip;

// ---- S2: front-end seam ---------------------------------------------------------------------------
struct dabhip_sdr {
  Engine eng;
  DeviceBuffer<uint8_t> window;      // the most recent IQ bytes, device resident
  DeviceBuffer<StreamState> state;
  DeviceBuffer<uint8_t> tail;        // the last kTailBytes of sdr->buffer (device_types.hpp)
  int64_t base = 0;                  // stream offset of window[0]
  int64_t fed = 0;                   // bytes received so far
  int call = 0;
  CallDesc last{};
  explicit dabhip_sdr(int device) : eng(device) {}
};

namespace {
constexpr int64_t kWindowBytes = int64_t(48) << 20;
constexpr int64_t kKeepBytes = int64_t(16) << 20;
}  // namespace

extern "C" {

dabhip_sdr* dabhip_sdr_init(int device)
{
  dabhip_sdr* s = new (std::nothrow) dabhip_sdr(device);
  if (!s) return nullptr;
  if (!s->eng.ok() || !s->window.reserve(kWindowBytes) || !s->state.reserve(1) || !s->tail.reserve(kTailBytes)) { delete s; return nullptr; }
  StreamState st;
  std::memset(&st, 0, sizeof st);
  fifo_reset(st);
  if (blocking_copy(s->state.get(), &st, sizeof st, hipMemcpyHostToDevice) != hipSuccess || hipMemset(s->tail.get(), 0, kTailBytes) != hipSuccess) {
    set_error("sdr_init: state upload failed");
    delete s;
    return nullptr;
  }
  std::memset(&s->last, 0, sizeof s->last);
  return s;
}
void dabhip_sdr_free(dabhip_sdr* s) { delete s; }

int dabhip_sdr_demod(dabhip_sdr* s, const uint8_t* input_buffer, int input_buffer_len, uint8_t* fic, uint8_t* msc)
{
  if (!s || (!input_buffer && input_buffer_len != 0) || !fic || !msc) { set_error("sdr_demod: null argument"); return -1; }
  // sdr_demod appends whatever the callback left, input_buffer_len bytes (input_sdr.c:36-38; librtlsdr delivers DEFAULT_BUF_LENGTH = 262144,
  // dab2eti.c:125-126,238, a file's last buffer is shorter).  Whole I/Q pairs only: the kernels read the stream two bytes at a time.
  if (input_buffer_len < 0 || input_buffer_len > kChunkBytes || (input_buffer_len & 1)) {
    set_error("sdr_demod: input_buffer_len must be an even number of bytes, 0 .. 262144 (sizeof sdr->input_buffer, input_sdr.h:14)");
    return -1;
  }
  if (s->fed - s->base + input_buffer_len > kWindowBytes) {   // slide the device window
    const int64_t keep_from = s->fed - kKeepBytes;
    DeviceBuffer<uint8_t> tmp;
    if (!tmp.reserve(kKeepBytes)) return -1;
    if (blocking_copy(tmp.get(), s->window.get() + (keep_from - s->base), kKeepBytes, hipMemcpyDeviceToDevice) != hipSuccess ||
        blocking_copy(s->window.get(), tmp.get(), kKeepBytes, hipMemcpyDeviceToDevice) != hipSuccess) {
      set_error("sdr_demod: window slide failed");
      return -1;
    }
    s->base = keep_from;
  }
  if (input_buffer_len && blocking_copy(s->window.get() + (s->fed - s->base), input_buffer, input_buffer_len, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("sdr_demod: IQ upload failed");
    return -1;
  }
  s->fed += input_buffer_len;
  const uint8_t* virtual_base = s->window.get() - s->base;    // stream offset x lives at virtual_base + x
  if (!s->eng.scan_one_call(virtual_base, s->state.get(), s->tail.get(), s->call, input_buffer_len, &s->last)) return -1;
  ++s->call;
  if (s->last.status != 2) return 0;
  for (int i = 0; i < s->last.view.nseg; ++i)
    if (s->last.view.seg_src[i] >= 0 && s->last.view.seg_src[i] < s->base) { set_error("sdr_demod: stale frame tail older than the device window"); return -1; }
  return s->eng.demod_one_frame(virtual_base, s->last, fic, msc) ? 1 : -1;
}

int32_t dabhip_sdr_coarse_timeshift(const dabhip_sdr* s) { return s ? s->last.coarse_timeshift : 0; }
int32_t dabhip_sdr_fine_timeshift(const dabhip_sdr* s) { return s ? s->last.fine_timeshift : 0; }
int32_t dabhip_sdr_coarse_freq_shift(const dabhip_sdr* s) { return s ? s->last.coarse_freq_shift : 0; }
double dabhip_sdr_fine_freq_shift(const dabhip_sdr* s) { return s ? s->last.fine_freq_shift : 0.0; }

}  // extern "C"

// ---- S3: back-end seam ----------------------------------------------------------------------------
struct dabhip_dab {
  Engine eng;
  ControlPlane plane;
  dabhip_eti_callback cb = nullptr;
  std::vector<uint8_t> fic, msc, fibs, ok, eti;
  int slot = 0;                      // TF slot the next frame goes to
  int ordinal = 0;                   // == slot + dropped
  int dropped = 0;                   // TF slots discarded from the front so far
  explicit dabhip_dab(int device) : eng(device), fic(kFicBits), msc(kMscBits), fibs(384), ok(12), eti(4 * kEtiBytes) {}
};

namespace {
constexpr int kDabSlots = 64;
}

extern "C" {

dabhip_dab* dabhip_dab_init(int device, dabhip_eti_callback cb)
{
  dabhip_dab* d = new (std::nothrow) dabhip_dab(device);
  if (!d) return nullptr;
  if (!d->eng.ok() || !d->eng.reserve_tf_slots(kDabSlots)) { delete d; return nullptr; }
  d->cb = cb;
  return d;
}
void dabhip_dab_free(dabhip_dab* d) { delete d; }
uint8_t* dabhip_dab_tf_fic(dabhip_dab* d) { return d ? d->fic.data() : nullptr; }
uint8_t* dabhip_dab_tf_msc(dabhip_dab* d) { return d ? d->msc.data() : nullptr; }
int dabhip_dab_locked(const dabhip_dab* d) { return d && d->plane.locked(); }
int64_t dabhip_dab_take_log(dabhip_dab* d, char* buf, int64_t cap) { return d ? hand_over_text(d->plane.take_log(), buf, cap) : -1; }
uint32_t dabhip_dab_status(const dabhip_dab* d) { return d ? d->plane.fault() : 0xffffffffu; }
int dabhip_dab_set_soft(dabhip_dab* d, int enable)
{
  if (!d) { set_error("dab_set_soft: null handle"); return -1; }
  if (d->slot != 0 || d->dropped != 0) { set_error("dab_set_soft: only before the first frame"); return -1; }
  d->eng.set_soft(enable != 0);
  return d->eng.reserve_tf_slots(kDabSlots) ? 0 : -1;
}
int dabhip_dab_set_decoder_forms(dabhip_dab* d, int msc_form, int fic_form)
{
  if (!d) { set_error("dab_set_decoder_forms: null handle"); return -1; }
  return d->eng.set_decoder_forms(msc_form, fic_form) ? 0 : -1;
}
int dabhip_dab_set_soft_lanes(dabhip_dab* d, int enable)
{
  if (!d) { set_error("dab_set_soft_lanes: null handle"); return -1; }
  d->eng.set_soft_lanes(enable != 0);
  return 0;
}
int dabhip_dab_decoder_forms(const dabhip_dab* d, uint32_t* msc_mask, uint32_t* fic_mask)
{
  if (!d) { set_error("dab_decoder_forms: null handle"); return -1; }
  if (msc_mask) *msc_mask = d->eng.msc_forms_ran();
  if (fic_mask) *fic_mask = d->eng.fic_forms_ran();
  return 0;
}
int dabhip_dab_set_launch_limits(dabhip_dab* d, const int64_t* limits, int n)
{
  if (!d || !limits || n != kLaunchLimitCount) { set_error("dab_set_launch_limits: bad argument"); return -1; }
  return d->eng.set_launch_limits(limits) ? 0 : -1;
}
int dabhip_dab_launch_report(const dabhip_dab* d, int64_t* out, int cap)
{
  if (!d || !out || cap < 0) { set_error("dab_launch_report: bad argument"); return -1; }
  return report_to_words(d->eng.launch_report(), out, cap);
}
int dabhip_dab_last_fibs(const dabhip_dab* d, uint8_t* fibs, uint8_t* crc_ok)
{
  if (!d || !fibs || !crc_ok) return -1;
  std::memcpy(fibs, d->fibs.data(), 384);
  std::memcpy(crc_ok, d->ok.data(), 12);
  return 0;
}

int dabhip_dab_process_frame(dabhip_dab* d)
{
  if (!d) { set_error("dab_process_frame: null handle"); return -1; }
  d->eng.clear_forms_ran();
  d->eng.clear_launch_report();
  if (d->slot == kDabSlots) {        // keep the 4 most recent TFs (16 CIFs of interleaver history)
    if (!d->eng.recycle_tf_slots(kDabSlots, 4)) return -1;
    d->plane.rebase(4 * (kDabSlots - 4));
    d->dropped += kDabSlots - 4;
    d->slot = 4;
  }
  if (!d->eng.store_tf_bytes(d->slot, d->fic.data(), d->msc.data())) return -1;
  if (!d->eng.fic_decode_slots(d->slot, 1, d->fibs.data(), d->ok.data())) return -1;
  JobList jobs;
  d->plane.on_tf(d->slot, d->fibs.data(), d->ok.data(), jobs);
  ++d->slot;
  if (jobs.empty()) return 0;
  std::vector<int> row_base = {15}, fib_base = {0};   // single stream: CIF 0 at logical row 15 (Engine::store_tf_bytes)
  std::vector<const ControlPlane*> planes = {&d->plane};
  std::vector<const JobList*> job_lists = {&jobs};
  if (!d->eng.msc_decode(job_lists, planes, row_base, fib_base)) return -1;
  if (!d->eng.read_eti(0, static_cast<int64_t>(jobs.size()), d->eti.data())) return -1;
  if (d->cb)
    for (size_t f = 0; f < jobs.size(); ++f) d->cb(d->eti.data() + f * kEtiBytes);
  return static_cast<int>(jobs.size());
}

}  // extern "C"
