// capi_detail.hpp — what the files of the C ABI layer (capi_*.cpp, session.cpp, multi.cpp) share.  Host-only, no GPU call.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "launch_limits.hpp"

namespace dabhip {

void set_error(const std::string& msg);

// copy `text` into buf (NUL-terminated, cut at cap - 1 bytes); returns the length of the whole text
inline int64_t hand_over_text(const std::string& text, char* buf, int64_t cap)
{
  if (buf && cap > 0) {
    const size_t n = std::min(text.size(), static_cast<size_t>(cap - 1));
    std::memcpy(buf, text.data(), n);
    buf[n] = 0;
  }
  return static_cast<int64_t>(text.size());
}

// SubChIds -> Engine::set_subchannel_filter's mask; no list = all of them
inline uint64_t subchannel_mask(const int32_t* ids, int n)
{
  if (!ids || n <= 0) return ~0ull;
  uint64_t m = 0;
  for (int i = 0; i < n; ++i)
    if (ids[i] >= 0 && ids[i] < 64) m |= 1ull << ids[i];
  return m;
}

// a launch report as the *_launch_report entries hand it over: at most cap words; returns how many
inline int report_to_words(const LaunchReport& r, int64_t* out, int cap)
{
  const int64_t v[kLaunchReportCount] = {r.decoder, r.regroup, r.fic_group, r.gather, r.ofdm_chunks, r.fic_prepass, r.fetch_form, r.fetches, r.gather_calls, r.decoder_planned};
  for (int i = 0; i < cap && i < kLaunchReportCount; ++i) out[i] = v[i];
  return std::min(cap, kLaunchReportCount);
}

// the *_eti_drain entries: every frame of streams [0, nstreams) to the sink, stream by stream in emission order.  count(b): frames of stream b;
// read(b, dst, n): n of them to dst, returns n.  read_empty: a stream without frames is read all the same (dabhip_engine_eti_drain: its read refuses
// the still unallocated buffer, so that a batch whose first stream gave nothing fails -- kept as it is; the other forms skip such a stream)
template <class Count, class Read>
int64_t drain_eti(int nstreams, dabhip_eti_sink sink, void* user, bool read_empty, Count count, Read read)
{
  int64_t total = 0;
  std::vector<uint8_t> buf;
  for (int b = 0; b < nstreams; ++b) {
    const int64_t n = count(b);
    if (n < 0) return -1;
    buf.resize(static_cast<size_t>(n) * DABHIP_ETI_BYTES);
    if ((n || read_empty) && read(b, buf.data(), n) != n) return -1;
    for (int64_t f = 0; f < n; ++f) sink(buf.data() + f * DABHIP_ETI_BYTES, b, user);
    total += n;
  }
  return total;
}

}  // namespace dabhip
