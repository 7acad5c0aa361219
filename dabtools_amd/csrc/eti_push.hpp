// eti_push.hpp — the front of the five pushes of ETI frames (dabhip_dabplus_push, _packet_push, _ts_push, _dir_push, _edi_push): what such a
// push is refused for, how many frames it brings, and the block of per-stream numbers its kernels read.  Host-only, no GPU call
// (tests/host_sanitize/eti_push_units.cpp runs it); StageFrame::place (stage_frame.hpp) carries the plan out.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace dabhip {

// the frames of one push as the kernels see them: stream s's new frames are frames + (base[s] + v) 6144, v < nnew[s]
struct EtiFrames {
  const uint8_t* frames;
  const int64_t* base;
  const int* nnew;
};

constexpr int64_t kEtiNoTotalBound = std::numeric_limits<int64_t>::max();

struct EtiPush {
  std::string refusal;                             // "" = taken
  int64_t total = 0;                               // frames of all streams
  int maxv = 0;                                    // the most frames of one stream, its carried ones included
  int nstreams = 0;
  bool carries = false;                            // the block has its third column
  std::vector<uint8_t> meta;                       // base (int64) | nnew (int) [| ncarry (int)], each per stream: what goes to the device
};

// who: the entry's name, in front of a refusal.  carried: frames every stream still holds from the push before (DAB+), the block's third column.
inline EtiPush plan_eti_push(const char* who, const int64_t* counts, int nstreams, bool frames_is_null, int64_t max_per_stream, int64_t max_total,
                             const int* carried = nullptr)
{
  EtiPush p;
  const size_t ns = static_cast<size_t>(nstreams);
  p.nstreams = nstreams;
  p.carries = carried != nullptr;
  p.meta.resize(ns * (carried ? 16 : 12));
  for (size_t s = 0; s < ns; ++s) {
    if (counts[s] < 0 || counts[s] > max_per_stream) { p.refusal = std::string(who) + ": bad frame count"; return p; }
    const int n = static_cast<int>(counts[s]);
    std::memcpy(p.meta.data() + 8 * s, &p.total, 8);
    std::memcpy(p.meta.data() + 8 * ns + 4 * s, &n, 4);
    if (carried) std::memcpy(p.meta.data() + 12 * ns + 4 * s, &carried[s], 4);
    p.total += counts[s];
    p.maxv = std::max(p.maxv, (carried ? carried[s] : 0) + n);
  }
  if (p.total > max_total) p.refusal = std::string(who) + ": too many frames for one push";
  else if (p.total > 0 && frames_is_null) p.refusal = std::string(who) + ": null frames";
  return p;
}

}  // namespace dabhip
