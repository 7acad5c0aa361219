// tii_units.cpp — transmitter identification's host rule and carrier list (csrc/tii_detect.hpp) as a stand-alone program under
// -fsanitize=address,undefined (tests/test_tii_model.py builds and runs it).  Sums of exactly 192 values and records of exactly `cap` entries, carrier
// lists of exactly 32: an index outside what the header promised is an overrun the sanitizer reports.  The pattern table, the tiling of the 1536
// carriers, the bin map against the carrier lists; the rule on zeros, on the exact ties, on equal values, on sums near 2^64 (the 128-bit products)
// and on random sums against a restatement with sorting by hand; the SHADOW flag at exactly 64 x and just above.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "../../dabtools_amd/csrc/tii_detect.hpp"

using namespace dabhip;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace {

struct Sums {
  std::unique_ptr<uint64_t[]> t{new uint64_t[kTiiSums]};      // exactly 192
  Sums() { for (int i = 0; i < kTiiSums; ++i) t[i] = 0; }
  uint64_t& at(int c, int b) { CHECK(c >= 0 && c < kTiiSubs && b >= 0 && b < kTiiBits); return t[c * kTiiBits + b]; }
};

// the rule run with room for exactly `cap` records
std::vector<dabhip_tii_id> run(Sums& s, int cap, int* total = nullptr)
{
  std::unique_ptr<dabhip_tii_id[]> out(new dabhip_tii_id[cap > 0 ? cap : 1]);
  const int n = tii_detect(s.t.get(), cap > 0 ? out.get() : nullptr, cap);
  CHECK(n >= 0 && n <= kTiiSubs);
  if (total) *total = n;
  return std::vector<dabhip_tii_id>(out.get(), out.get() + (n < cap ? n : cap));
}

void patterns_and_carriers()
{
  CHECK(tii_pattern(0) == 0x0f && tii_pattern(69) == 0xf0 && tii_pattern(70) == -1);
  for (int p = 0; p < kTiiPatterns; ++p) {
    CHECK(__builtin_popcount(static_cast<unsigned>(tii_pattern(p))) == 4 && tii_pattern_index(tii_pattern(p)) == p);
    if (p) CHECK(tii_pattern(p) > tii_pattern(p - 1));
  }
  std::vector<int> seen(1537, 0);                              // carriers -768 .. 768
  for (int c = 0; c < kTiiSubs; ++c) {
    for (int p = 0; p < kTiiPatterns; ++p) {
      std::unique_ptr<int16_t[]> k(new int16_t[kTiiCarriers]);   // exactly 32
      CHECK(tii_carriers(p, c, k.get()));
      for (int i = 0; i < kTiiCarriers; ++i) {
        CHECK(k[i] >= -768 && k[i] <= 768 && k[i] != 0);
        if (i & 1) CHECK(k[i] == k[i - 1] + 1);
        const int slot = tii_slot_of_bin((k[i] + 2048) % 2048);
        CHECK(slot >= 0 && slot / kTiiBits == c && (tii_pattern(p) >> (7 - slot % kTiiBits) & 1));
      }
    }
    // the union over b of one sub identifier: patterns 0x0f and 0xf0 together hold every b once
    std::unique_ptr<int16_t[]> lo(new int16_t[kTiiCarriers]), hi(new int16_t[kTiiCarriers]);
    CHECK(tii_carriers(0, c, lo.get()) && tii_carriers(69, c, hi.get()));
    for (int i = 0; i < kTiiCarriers; ++i) { ++seen[static_cast<size_t>(lo[i] + 768)]; ++seen[static_cast<size_t>(hi[i] + 768)]; }
  }
  for (int k = -768; k <= 768; ++k) CHECK(seen[static_cast<size_t>(k + 768)] == (k != 0));      // tiled exactly once
  int mapped = 0;
  for (int bin = 0; bin < kTiiWindow; ++bin) mapped += tii_slot_of_bin(bin) >= 0;
  CHECK(mapped == 1536 && tii_slot_of_bin(0) == -1 && tii_slot_of_bin(769) == -1 && tii_slot_of_bin(1279) == -1);
  std::unique_ptr<int16_t[]> k(new int16_t[kTiiCarriers]);
  CHECK(!tii_carriers(-1, 0, k.get()) && !tii_carriers(70, 0, k.get()) && !tii_carriers(0, -1, k.get()) && !tii_carriers(0, 24, k.get()));
}

void rule()
{
  {
    Sums z;
    CHECK(run(z, 24).empty() && run(z, 0).empty());
  }
  {                                                            // one clear comb; cap smaller than the count
    Sums s;
    for (int c : {2, 7, 23})
      for (int b : {1, 2, 5, 6}) s.at(c, b) = 1000;
    int total = 0;
    const auto one = run(s, 1, &total);
    CHECK(total == 3 && one.size() == 1 && one[0].sub_id == 2 && one[0].main_id == tii_pattern_index(0x66));
    const auto all = run(s, 24);
    CHECK(all.size() == 3 && all[1].sub_id == 7 && all[2].sub_id == 23 && all[0].strong == 4000 && all[0].weak == 0 && all[0].flags == 0);
    int t0 = 0;
    CHECK(run(s, 0, &t0).empty() && t0 == 3);
  }
  {                                                            // the exact ties are absent, one more is present
    Sums s;
    for (int b = 0; b < 4; ++b) s.at(4, b) = 10;
    for (int b = 4; b < 8; ++b) s.at(4, b) = 5;                // s = 40 = 2 n, v3 = 10 = 2 v4
    CHECK(run(s, 24).empty());
    s.at(4, 3) = 11;                                           // s = 41 > 40, but v3 is still 10 = 2 v4: absent
    CHECK(run(s, 24).empty());
    for (int b = 0; b < 4; ++b) s.at(4, b) = 11;               // s = 44 > 40, v3 = 11 > 10
    CHECK(run(s, 24).size() == 1);
    s.at(4, 4) = 6;                                            // v3 = 11 <= 12
    CHECK(run(s, 24).empty());
    Sums e;                                                    // equal values: order goes to the lower b, and nothing is present
    for (int b = 0; b < 8; ++b) e.at(0, b) = 7;
    CHECK(run(e, 24).empty());
    Sums f;                                                    // four equal strong values among zeros, and a fifth equal to them: the lower four win, absent (v3 = v4)
    for (int b : {0, 3, 4, 6, 7}) f.at(9, b) = 50;
    CHECK(run(f, 24).empty());
    f.at(9, 7) = 0;
    const auto r = run(f, 24);
    CHECK(r.size() == 1 && r[0].main_id == tii_pattern_index(0x9a));      // b = 0, 3, 4, 6
  }
  {                                                            // values up to 2^64 - 1: sums beyond 2^64, saturating records, no wrap in the comparisons
    Sums s;
    for (int b = 0; b < 4; ++b) s.at(1, b) = UINT64_MAX;
    for (int b = 4; b < 8; ++b) s.at(1, b) = UINT64_MAX / 2;   // v3 = 2 v4 + 1: present by the second test; s = 4 M, 2 n = 4 (M / 2) < s
    const auto r = run(s, 24);
    CHECK(r.size() == 1 && r[0].strong == UINT64_MAX && r[0].weak == UINT64_MAX && r[0].main_id == 69);
    for (int b = 4; b < 8; ++b) s.at(1, b) = UINT64_MAX / 2 + 1;      // 2 v4 = 2^64 > v3: a 64-bit product would wrap to 0 and pass
    CHECK(run(s, 24).empty());
  }
  {                                                            // SHADOW: at exactly 64 x not flagged, just above flagged; another main identifier never
    Sums s;
    for (int b = 0; b < 4; ++b) { s.at(3, b) = 6400; s.at(10, b) = 100; s.at(11, b + 4) = 1; }
    auto r = run(s, 24);
    CHECK(r.size() == 3 && r[0].flags == 0 && r[1].flags == 0 && r[2].flags == 0);
    s.at(3, 0) = 6401;
    r = run(s, 24);
    CHECK(r.size() == 3 && r[0].flags == 0 && r[1].flags == DABHIP_TII_SHADOW && r[2].flags == 0);
  }
  std::mt19937_64 rng(5);
  int present = 0;
  for (int trial = 0; trial < 400; ++trial) {                  // random sums against a restatement by hand
    Sums s;
    const int bits = 1 + static_cast<int>(rng() % 64);
    for (int i = 0; i < kTiiSums; ++i) s.t[i] = (rng() >> (64 - bits)) >> (rng() % 4 ? 0 : rng() % 8);
    const auto r = run(s, 24);
    size_t at = 0;
    for (int c = 0; c < kTiiSubs; ++c) {
      int order[8] = {0, 1, 2, 3, 4, 5, 6, 7};
      for (int i = 1; i < 8; ++i)                              // insertion sort: descending, equal values keep their order
        for (int j = i; j > 0 && s.at(c, order[j]) > s.at(c, order[j - 1]); --j) std::swap(order[j], order[j - 1]);
      unsigned __int128 strong = 0, weak = 0;
      int word = 0;
      for (int i = 0; i < 4; ++i) { strong += s.at(c, order[i]); weak += s.at(c, order[4 + i]); word |= 1 << (7 - order[i]); }
      const bool here = strong > 2 * weak && static_cast<unsigned __int128>(s.at(c, order[3])) > 2 * static_cast<unsigned __int128>(s.at(c, order[4]));
      if (!here) continue;
      CHECK(at < r.size() && r[at].sub_id == c && r[at].main_id == tii_pattern_index(word));
      ++at;
    }
    CHECK(at == r.size());
    present += static_cast<int>(at);
  }
  CHECK(present > 20);
}

}  // namespace

int main()
{
  patterns_and_carriers();
  rule();
  std::printf("ok tii-units\n");
  return 0;
}
