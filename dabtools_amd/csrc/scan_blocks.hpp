// scan_blocks.hpp — the host rule of the block scan (scan.cpp runs it, k_scan.hip is its kernel): what dabhip_scan_create refuses, the bookkeeping
// of one push (which segments it completes, which samples are carried), and the rule that turns a power spectrum into a list of DAB blocks
// (dabhip_scan_detect).  Host-only, integers only, no GPU call (tests/host_sanitize/scan_units.cpp runs it on arrays of exactly the stated sizes).
// The arithmetic and the rule are stated in include/dabhip.h, "block scan"; tests/scan_model.py restates both.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dabhip.h"

namespace dabhip {

constexpr int kScanSize = 4096;                    // S: samples of a segment, bins of the spectrum
constexpr int kScanMaxSegments = 65536;
constexpr int kScanMaxBlocks = 16;
constexpr int64_t kScanMinRate = 2048000, kScanMaxRate = 10240000;
constexpr int64_t kScanMinWidth = 1436000, kScanMaxWidth = 1636000, kScanSnap = 32000;
constexpr int64_t kScanMaxCenter = 1000000000000;  // 1 THz: beyond it center_hz + offset_hz is no frequency anybody tunes to

// everything dabhip_scan_create refuses before it looks for a device ("" = taken)
inline std::string scan_check(int nstreams, int format, int64_t rate_hz, int nsegments)
{
  if (nstreams <= 0 || nstreams > 65535) return "nstreams must be 1 .. 65535";
  if (format < 0 || format >= 4) return "unknown format " + std::to_string(format) + " (0 = cu8, 1 = cs8, 2 = cs16, 3 = cf32)";
  if (rate_hz < kScanMinRate || rate_hz > kScanMaxRate) return "sample rate " + std::to_string(rate_hz) + " Hz is outside 2048000 .. 10240000";
  if (nsegments < 1 || nsegments > kScanMaxSegments) return "nsegments must be 1 .. 65536";
  return "";
}

// ---- bookkeeping of one stream: positions are absolute and 64-bit, the first sample ever pushed is 0 ------------------------------------------
struct ScanStreamState {
  int64_t pushed = 0, kept_from = 0;               // input samples so far; samples [kept_from, pushed) are carried
  int64_t done = 0;                                // segments accumulated
};
struct ScanPush {
  int64_t carry_from = 0, new_from = 0, end = 0;   // before the push [carry_from, new_from) was kept; the push brings [new_from, end)
  int64_t first_seg = 0, nseg = 0;                 // segments [first_seg, first_seg + nseg) are completed by this push: samples [4096 seg, 4096 seg + 4096)
  int64_t keep_from = 0, keep = 0;                 // to carry afterwards: the unfinished segment's samples, at most 4095; nothing once the window is full
};
inline ScanPush scan_plan_push(int nsegments, ScanStreamState& s, int64_t nsamples)
{
  ScanPush p;
  p.carry_from = s.kept_from;
  p.new_from = s.pushed;
  s.pushed += nsamples;
  p.end = s.pushed;
  p.first_seg = s.done;
  const int64_t total = std::min<int64_t>(nsegments, s.pushed / kScanSize);
  p.nseg = total - s.done;
  s.done = total;
  p.keep_from = s.done == nsegments ? s.pushed : s.done * kScanSize;
  p.keep = s.pushed - p.keep_from;
  s.kept_from = p.keep_from;
  return p;
}
// of a push of nsamples, the samples the host path uploads: only what the window can still use -- the unfinished segment and the segments missing
inline int64_t scan_upload_samples(int nsegments, const ScanStreamState& s, int64_t nsamples)
{
  const int64_t wanted = s.done == nsegments ? 0 : static_cast<int64_t>(nsegments) * kScanSize - s.pushed;
  return std::min<int64_t>(nsamples, std::max<int64_t>(wanted, 0));
}

// ---- from spectrum to blocks -------------------------------------------------------------------------------------------------------------------
// the 38 Band III block centres in Hz, ascending, and their names
struct ScanRaster {
  int64_t hz[38];
  char name[38][4];
};
inline ScanRaster scan_raster()
{
  ScanRaster r;
  static const int64_t kFirst[8] = {174928, 181936, 188928, 195936, 202928, 209936, 216928, 223936};      // 5A .. 12A in kHz; B, C, D each + 1712
  static const int64_t k13[6] = {230784, 232496, 234208, 235776, 237488, 239200};
  int n = 0;
  for (int ch = 0; ch < 8; ++ch)
    for (int l = 0; l < 4; ++l, ++n) {
      r.hz[n] = (kFirst[ch] + 1712 * l) * 1000;
      std::snprintf(r.name[n], sizeof r.name[n], "%d%c", 5 + ch, 'A' + l);
    }
  for (int l = 0; l < 6; ++l, ++n) {
    r.hz[n] = k13[l] * 1000;
    std::snprintf(r.name[n], sizeof r.name[n], "13%c", 'A' + l);
  }
  return r;
}

inline int64_t scan_floor_div(__int128 num, int64_t den)      // den > 0; towards minus infinity
{
  __int128 q = num / den;
  if (num % den < 0) --q;
  return static_cast<int64_t>(q);
}

// P: 4096 bins in transform order.  out: room for cap records (16 suffice).  Returns the number of blocks, in ascending offset; -1 with *why set
// when the rate is refused or more than 16 blocks pass the width gate.
inline int scan_detect(const uint64_t* P, int64_t rate_hz, int64_t center_hz, dabhip_scan_block* out, int cap, std::string* why)
{
  typedef unsigned __int128 u128;
  if (rate_hz < kScanMinRate || rate_hz > kScanMaxRate) { *why = "sample rate " + std::to_string(rate_hz) + " Hz is outside 2048000 .. 10240000"; return -1; }
  if (center_hz < 0 || center_hz > kScanMaxCenter) { *why = "center_hz must be 0 (not known) .. 1000000000000"; return -1; }
  const int N = kScanSize;
  const int64_t Fin = rate_hz;
  const int ni = static_cast<int>(700000LL * N / Fin), a0 = static_cast<int>((800000LL * N + Fin - 1) / Fin), a1 = static_cast<int>(900000LL * N / Fin);
  const int w = std::max(1, static_cast<int>(16000LL * N / Fin));
  const int nin = 2 * ni + 1, ng = a1 - a0 + 1;
  std::vector<u128> pre(static_cast<size_t>(N) + 1, 0);          // of P in shifted order: bin b has frequency (b - 2048) Fin / 4096
  for (int b = 0; b < N; ++b) pre[static_cast<size_t>(b) + 1] = pre[static_cast<size_t>(b)] + P[(b + N / 2) % N];
  auto sum = [&](int from, int to) { return pre[static_cast<size_t>(to) + 1] - pre[static_cast<size_t>(from)]; };      // bins [from, to]
  auto in_of = [&](int c) { return sum(c - ni, c + ni); };
  auto candidate = [&](int c) {
    const u128 in = in_of(c) * static_cast<u128>(ng);
    return in > 4 * sum(c - a1, c - a0) * static_cast<u128>(nin) && in > 4 * sum(c + a0, c + a1) * static_cast<u128>(nin);
  };
  auto sat = [](u128 v) { return v > static_cast<u128>(UINT64_MAX) ? UINT64_MAX : static_cast<uint64_t>(v); };
  const ScanRaster raster = scan_raster();
  std::vector<dabhip_scan_block> found;
  for (int c = a1; c < N - a1;) {
    if (!candidate(c)) { ++c; continue; }
    const int a = c;
    while (c + 1 < N - a1 && candidate(c + 1)) ++c;
    const int b = c++;                                           // the run [a, b]
    const int mid = (a + b) / 2;
    const u128 in = in_of(mid);
    int edge[2];
    for (int side = 0; side < 2; ++side) {
      const int d = side ? 1 : -1;
      int j = mid + d * ni;
      for (;; j += d) {
        const int from = std::max(0, j - w), to = std::min(N, j + w + 1);      // the box [from, to)
        if (sum(from, to - 1) * static_cast<u128>(nin) * 4 < in * static_cast<u128>(to - from) || j == 0 || j == N - 1) break;
      }
      edge[side] = j;
    }
    dabhip_scan_block r;
    std::memset(&r, 0, sizeof r);
    r.raw_center_hz = scan_floor_div(static_cast<__int128>(a + b - N) * Fin + N, 2 * N);
    r.offset_hz = scan_floor_div(static_cast<__int128>(edge[0] + edge[1] - N) * Fin + N, 2 * N);
    r.width_hz = static_cast<int64_t>(edge[1] - edge[0]) * Fin / N;
    if (r.width_hz < kScanMinWidth || r.width_hz > kScanMaxWidth) continue;
    r.in = sat(in);
    r.lo = sat(sum(mid - a1, mid - a0));
    r.hi = sat(sum(mid + a0, mid + a1));
    r.nin = nin;
    r.ng = ng;
    if (center_hz > 0) {
      const int64_t f = center_hz + r.offset_hz;
      int best = 0;
      for (int k = 1; k < 38; ++k)
        if (std::llabs(raster.hz[k] - f) < std::llabs(raster.hz[best] - f)) best = k;
      if (std::llabs(raster.hz[best] - f) <= kScanSnap) {
        r.offset_hz = raster.hz[best] - center_hz;
        std::memcpy(r.name, raster.name[best], sizeof raster.name[best]);
      }
    }
    found.push_back(r);
  }
  if (found.size() > static_cast<size_t>(kScanMaxBlocks)) { *why = std::to_string(found.size()) + " blocks found: more than 16"; return -1; }
  std::stable_sort(found.begin(), found.end(), [](const dabhip_scan_block& x, const dabhip_scan_block& y) { return x.offset_hz < y.offset_hz; });
  for (size_t k = 0; k < found.size() && static_cast<int>(k) < cap; ++k) out[k] = found[k];
  return static_cast<int>(found.size());
}

}  // namespace dabhip
