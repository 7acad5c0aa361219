// eti_lanes.hpp — what the three lane stages (dabhip_dabplus, dabhip_packet, dabhip_ts) keep about their lanes, a lane being one (stream,
// sub-channel): the create-time checks, the SubChIds on the device, the bounds check of the queries, the host copy of the last push's lane
// bases and the copy behind the *_stats entries.  f is the handle's StageFrame (stage_frame.hpp).
#pragma once

#include <string>
#include <vector>

#include "rs_code.hpp"
#include "stage_frame.hpp"

namespace dabhip {

struct EtiLanes {
  const char* const who;                           // "dabplus", "packet", "ts": in front of every refusal
  int nstreams = 0, nsub = 0;
  DeviceBuffer<int32_t> subch;
  mutable bool fetched = false;                    // a push clears it
  mutable std::vector<int> h_base;                 // lane l's items of the last push are [h_base[l], h_base[l + 1]) of the push's list

  size_t count() const { return static_cast<size_t>(nstreams) * nsub; }

  // the checks of *_create and the SubChIds' upload.  others_ok: the entry's further pointers are there; max_lanes: 0 = no ceiling
  template <class Frame>
  bool create(const Frame& f, int nstreams_, const int32_t* subch_ids, int nsub_, bool others_ok, int64_t max_lanes)
  {
    const std::string at = std::string(who) + "_create: ";
    if (nstreams_ <= 0 || nsub_ <= 0 || nsub_ > 64 || !subch_ids || !others_ok) { set_error(at + "bad arguments"); return false; }
    for (int q = 0; q < nsub_; ++q)
      if (subch_ids[q] < 0 || subch_ids[q] > 63) { set_error(at + "SubChId out of range"); return false; }
    if (max_lanes && static_cast<int64_t>(nstreams_) * nsub_ > max_lanes) { set_error(at + "too many (stream, sub-channel) pairs"); return false; }
    nstreams = nstreams_;
    nsub = nsub_;
    return subch.reserve(nsub) && f.ok(hipMemcpy(subch.get(), subch_ids, sizeof(int32_t) * nsub, hipMemcpyHostToDevice), "upload");
  }

  bool lane_ok(int s, int q) const
  {
    if (s < 0 || s >= nstreams || q < 0 || q >= nsub) { set_error(std::string(who) + ": no such stream / sub-channel"); return false; }
    return true;
  }
  int lane(int stream, int sub) const { return stream * nsub + sub; }

  // h_base from the device's count() + 1 lane bases, once per push; any: the push gave something (else all are 0 and nothing is copied)
  template <class Frame>
  bool fetch(const Frame& f, const int* dev_base, bool any) const
  {
    if (fetched) return true;
    if (!f.use_device()) return false;
    h_base.assign(count() + 1, 0);
    if (any && !f.ok(blocking_copy(h_base.data(), dev_base, sizeof(int) * (count() + 1), hipMemcpyDeviceToHost), "records")) return false;
    fetched = true;
    return true;
  }
  void range(int stream, int sub, int64_t& a, int64_t& n) const
  {
    a = h_base[lane(stream, sub)];
    n = h_base[lane(stream, sub) + 1] - a;
  }

  // the *_stats entries: the first n of a lane's `stride` counters
  template <class Frame>
  int lane_counters(const Frame& f, int stream, int sub, const int64_t* counters, int stride, int64_t* out, int n) const
  {
    if (!lane_ok(stream, sub) || !f.use_device()) return -1;
    return f.ok(blocking_copy(out, counters + static_cast<size_t>(lane(stream, sub)) * stride, sizeof(int64_t) * n, hipMemcpyDeviceToHost), "counters") ? 0 : -1;
  }
};

// the tables of a Reed-Solomon code (rs_code.hpp) as its kernels load them
template <int kRoots, class Frame>
bool upload_rs_tables(const Frame& f, DeviceBuffer<uint8_t>& gf)
{
  GfRs<kRoots> t;
  rs_tables_fill(t);
  return gf.reserve(sizeof t) && f.ok(hipMemcpy(gf.get(), &t, sizeof t, hipMemcpyHostToDevice), "upload");
}

}  // namespace dabhip
