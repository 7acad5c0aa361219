// tii.cpp — transmitter identification on the host side (include/dabhip.h, "TII"): the engine's hook -- the sums' rows, the one launch of
// k_tii.hip per decode over the scan's descriptors -- the stage entry on explicit frames, and the C ABI of both handles and of the host rule
// (tii_detect.hpp).
#include <string>
#include <vector>

#include "capi_detail.hpp"
#include "engine_detail.hpp"
#include "ingest_plan.hpp"
#include "tii.hpp"

namespace dabhip {

bool Engine::tii_tables()
{
  if (d_tii_nco_.get()) return true;
  for (Event& e : ev_tii_)
    if (!e && !check(e.create(), "hipEventCreate")) return false;
  const std::vector<uint32_t> nco = ingest_tune_nco_words();
  if (!d_tii_nco_.reserve(nco.size())) return false;
  if (!check(blocking_copy(d_tii_nco_.get(), nco.data(), nco.size() * 4, hipMemcpyHostToDevice), "NCO table upload")) { d_tii_nco_.release(); return false; }
  return true;
}

bool Engine::tii_begin(int nstreams, bool cont)
{
  if (!tii_tables()) return false;
  const bool keep = cont && tii_rows_ == nstreams && d_tii_sums_.get();      // (a session that switched TII on between two segments starts from zero)
  if (keep) return true;
  if (!d_tii_sums_.reserve(static_cast<size_t>(nstreams) * kTiiRow)) return false;
  tii_rows_ = nstreams;
  return check(hipMemsetAsync(d_tii_sums_.get(), 0, static_cast<size_t>(nstreams) * kTiiRow * sizeof(unsigned long long), stream_), "TII sums");
}

bool Engine::tii_launch()
{
  const TiiArgs a{d_iq_ptrs_.get(), d_descs_.get(), scan_.max_calls, nullptr, nullptr, d_tii_sums_.get()};
  tii_ran_ = record(ev_tii_[0], stream_) && check(launch_tii(a, scan_.ndesc, d_tii_nco_.get(), stream_), "TII launch") && record(ev_tii_[1], stream_);
  return tii_ran_;
}

bool Engine::tii_reset()
{
  if (!d_tii_sums_.get() || tii_rows_ == 0) return true;
  return check(hipSetDevice(device_), "hipSetDevice") &&
         check(hipMemsetAsync(d_tii_sums_.get(), 0, static_cast<size_t>(tii_rows_) * kTiiRow * sizeof(unsigned long long), stream_), "TII sums") &&
         check(hipStreamSynchronize(stream_), "TII sums");
}

bool Engine::tii_sums(int stream, uint64_t* T, int* frames)
{
  if (stream < 0 || stream >= tii_rows_ || !d_tii_sums_.get()) { set_error("tii_sums: no sums for this stream (dabhip_engine_set_tii before the decode)"); return false; }
  unsigned long long row[kTiiRow];
  if (!check(hipSetDevice(device_), "hipSetDevice") ||
      !check(blocking_copy(row, d_tii_sums_.get() + static_cast<size_t>(stream) * kTiiRow, sizeof row, hipMemcpyDeviceToHost), "TII sums download"))
    return false;
  for (int i = 0; T && i < kTiiSums; ++i) T[i] = row[i];
  if (frames) *frames = static_cast<int>(row[kTiiSums]);
  return true;
}

int Engine::stage_tii(const uint8_t* frames, int nframes, const int32_t* w0, const uint32_t* step, bool on_device, uint64_t* T)
{
  if (!ok_) { set_error("engine not initialised (no GPU?)"); return -1; }
  if (nframes <= 0) return 0;
  for (int j = 0; j < nframes; ++j)
    if (w0[j] < 0 || w0[j] > kTiiW0 + kTiiMaxShift) { set_error("stage_tii: frame " + std::to_string(j) + ": w0 must be 0 .. 608"); return -1; }
  if (!check(hipSetDevice(device_), "hipSetDevice") || !tii_tables()) return -1;
  if (!on_device) last_.pending = false;       // the last decode's samples in the engine's upload buffer are gone
  const uint8_t* const d_in = frames_on_device(frames, nframes, on_device);
  if (!d_in) return -1;
  const StreamState st0 = initial_state();
  std::vector<CallDesc> descs(static_cast<size_t>(nframes));
  for (int j = 0; j < nframes; ++j) {          // frame j of one stream, read where it lies
    std::memset(&descs[static_cast<size_t>(j)], 0, sizeof(CallDesc));
    descs[static_cast<size_t>(j)].status = 2;
    descs[static_cast<size_t>(j)].view = st0.view;
    descs[static_cast<size_t>(j)].view.seg_src[0] = static_cast<int64_t>(j) * kTfBytes;
  }
  const size_t words = static_cast<size_t>(nframes) * kTiiRow;
  std::vector<unsigned long long> rows(words);
  const bool done = d_tii_descs_.upload(descs, stream_) && d_tii_ptr_.upload(&d_in, 1, stream_) && d_tii_w0_.upload(w0, static_cast<size_t>(nframes), stream_) &&
                    d_tii_step_.upload(step, static_cast<size_t>(nframes), stream_) && d_tii_stage_sums_.reserve(words) &&
                    check(hipMemsetAsync(d_tii_stage_sums_.get(), 0, words * sizeof(unsigned long long), stream_), "TII sums") &&
                    check(launch_tii(TiiArgs{d_tii_ptr_.get(), d_tii_descs_.get(), nframes, d_tii_w0_.get(), d_tii_step_.get(), d_tii_stage_sums_.get()}, static_cast<size_t>(nframes),
                                     d_tii_nco_.get(), stream_),
                          "TII launch") &&
                    check(hipMemcpyAsync(rows.data(), d_tii_stage_sums_.get(), words * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_), "TII sums download");
  if (!check(hipStreamSynchronize(stream_), "stage_tii") || !done) return -1;      // (the uploads read this call's vectors: awaited on every path)
  for (int j = 0; j < nframes; ++j)
    for (int i = 0; i < kTiiSums; ++i) T[static_cast<size_t>(j) * kTiiSums + i] = rows[static_cast<size_t>(j) * kTiiRow + i];
  return nframes;
}

}  // namespace dabhip

using namespace dabhip;

extern "C" int dabhip_tii_detect(const uint64_t* T, dabhip_tii_id* out, int cap)
{
  if (!T || cap < 0 || (!out && cap > 0)) { set_error("tii_detect: bad argument"); return -1; }
  return tii_detect(T, out, cap);
}

extern "C" int dabhip_tii_carriers(int main_id, int sub_id, int16_t* k, int cap)
{
  if (!k || cap < kTiiCarriers) { set_error("tii_carriers: room for 32 carriers is needed"); return -1; }
  if (!tii_carriers(main_id, sub_id, k)) { set_error("tii_carriers: main_id must be 0 .. 69 and sub_id 0 .. 23"); return -1; }
  return kTiiCarriers;
}
