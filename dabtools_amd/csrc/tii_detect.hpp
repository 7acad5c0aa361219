// tii_detect.hpp — the host side of transmitter identification (include/dabhip.h, "TII"): the 70 patterns, the carriers of a transmitter, the bin
// -> (sub identifier, pattern bit) map that k_tii.hip folds by, and the rule that turns the folded sums T[24][8] into identifiers
// (dabhip_tii_detect).  Host-only, integers only, no GPU call (tests/host_sanitize/tii_units.cpp runs it on arrays of exactly the stated sizes);
// tests/tii_model.py restates all of it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/dabhip.h"

#ifdef __HIPCC__
#define DABHIP_TII_HD __host__ __device__
#else
#define DABHIP_TII_HD
#endif

namespace dabhip {

constexpr int kTiiSubs = 24, kTiiBits = 8, kTiiSums = kTiiSubs * kTiiBits, kTiiPatterns = 70, kTiiCarriers = 32;
constexpr int kTiiWindow = 2048;                    // samples of the window, bins of the transform
constexpr int kTiiW0 = 304, kTiiMaxShift = 304;     // the window starts at sample 304 + fine_timeshift of the frame buffer

// the 8-bit words with exactly four ones in ascending order: pattern p, or -1 past the 70th
inline int tii_pattern(int p)
{
  for (int w = 0, n = 0; w < 256; ++w)
    if (__builtin_popcount(static_cast<unsigned>(w)) == 4 && n++ == p) return w;
  return -1;
}
// the index of a word with exactly four ones
inline int tii_pattern_index(int word)
{
  int n = 0;
  for (int w = 0; w < word; ++w) n += __builtin_popcount(static_cast<unsigned>(w)) == 4;
  return n;
}

constexpr int kTiiQuarterBase[4] = {-768, -384, 1, 385};

// the 32 carriers of transmitter (main, sub), ascending within a quarter, quarter after quarter; false: no such transmitter
inline bool tii_carriers(int main_id, int sub_id, int16_t* k)
{
  if (main_id < 0 || main_id >= kTiiPatterns || sub_id < 0 || sub_id >= kTiiSubs) return false;
  const int word = tii_pattern(main_id);
  int n = 0;
  for (int q = 0; q < 4; ++q)
    for (int b = 0; b < kTiiBits; ++b) {
      if (!(word >> (7 - b) & 1)) continue;
      const int lower = kTiiQuarterBase[q] + 2 * sub_id + 48 * b;
      k[n++] = static_cast<int16_t>(lower);
      k[n++] = static_cast<int16_t>(lower + 1);
    }
  return true;
}

// bin of the 2048-point transform -> c * 8 + b of the pair it belongs to, -1 for the bins that carry nothing (0 and 769 .. 1279)
DABHIP_TII_HD inline int tii_slot_of_bin(int bin)
{
  int kk;                                           // position within the half: 0 .. 767
  if (bin >= 1 && bin <= 768) kk = bin - 1;
  else if (bin >= 1280 && bin < 2048) kk = bin - 1280;
  else return -1;
  if (kk >= 384) kk -= 384;
  return (kk % 48) / 2 * 8 + kk / 48;
}

// T: 192 sums, T[c * 8 + b].  out: room for cap records (24 suffice).  Returns the number of combs present, in ascending sub identifier.
inline int tii_detect(const uint64_t* T, dabhip_tii_id* out, int cap)
{
  typedef unsigned __int128 u128;
  dabhip_tii_id found[kTiiSubs];
  u128 strength[kTiiSubs];
  int nfound = 0;
  for (int c = 0; c < kTiiSubs; ++c) {
    int order[kTiiBits];
    for (int b = 0; b < kTiiBits; ++b) order[b] = b;
    const uint64_t* v = T + c * kTiiBits;
    std::stable_sort(order, order + kTiiBits, [&](int x, int y) { return v[x] > v[y]; });      // descending, ties to the lower b
    u128 s = 0, n = 0;
    for (int i = 0; i < 4; ++i) { s += v[order[i]]; n += v[order[4 + i]]; }
    if (!(s > 2 * n) || !(static_cast<u128>(v[order[3]]) > 2 * static_cast<u128>(v[order[4]]))) continue;
    int word = 0;
    for (int i = 0; i < 4; ++i) word |= 1 << (7 - order[i]);
    dabhip_tii_id r;
    std::memset(&r, 0, sizeof r);
    r.main_id = tii_pattern_index(word);
    r.sub_id = c;
    r.strong = s > static_cast<u128>(UINT64_MAX) ? UINT64_MAX : static_cast<uint64_t>(s);      // (saturating: no sum of an engine's gets there)
    r.weak = n > static_cast<u128>(UINT64_MAX) ? UINT64_MAX : static_cast<uint64_t>(n);
    strength[nfound] = s;
    found[nfound++] = r;
  }
  for (int i = 0; i < nfound; ++i)
    for (int j = 0; j < nfound; ++j)
      if (j != i && found[j].main_id == found[i].main_id && strength[j] > 64 * strength[i]) found[i].flags |= DABHIP_TII_SHADOW;
  for (int i = 0; i < nfound && i < cap; ++i) out[i] = found[i];
  return nfound;
}

}  // namespace dabhip
