// eti_push_units.cpp — the front of the five pushes of ETI frames (csrc/eti_push.hpp) and the STC walk of the three locate kernels
// (csrc/eti_locate.hpp) as a stand-alone program under -fsanitize=address,undefined (tests/test_scan_model.py builds and runs it).  counts[] and
// carried[] are arrays of EXACTLY the stream count and a frame is EXACTLY 6144 bytes on the heap, so a read beyond either is an overrun the
// sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../dabtools_amd/csrc/eti_locate.hpp"
#include "../../dabtools_amd/csrc/eti_push.hpp"

using namespace dabhip;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace {
// ---- plan_eti_push ---------------------------------------------------------------------------------------------------------------------------
struct Who {
  const char* name;
  int64_t per_stream, total;                                       // the bounds; total < 0: none
  bool carries;
};
const Who kWho[5] = {{"dabplus_push", 1 << 24, -1, true}, {"packet_push", 1 << 16, -1, false}, {"ts_push", 1 << 16, -1, false},
                     {"dir_push", 1 << 16, 1 << 16, false}, {"edi_push", 1 << 17, 1 << 17, false}};

EtiPush plan(const Who& w, const std::vector<int64_t>& counts, bool frames_is_null, const std::vector<int>* carried = nullptr)
{
  const size_t ns = counts.size();
  std::unique_ptr<int64_t[]> c(new int64_t[ns]);                   // exactly ns entries
  std::unique_ptr<int[]> k(carried ? new int[ns] : nullptr);
  for (size_t s = 0; s < ns; ++s) c[s] = counts[s];
  for (size_t s = 0; carried && s < ns; ++s) k[s] = (*carried)[s];
  return plan_eti_push(w.name, c.get(), static_cast<int>(ns), frames_is_null, w.per_stream, w.total < 0 ? kEtiNoTotalBound : w.total, k.get());
}

#define B8(x) x, 0, 0, 0, 0, 0, 0, 0                               /* an int64 below 256, as its bytes */
#define N4(x) x, 0, 0, 0                                           /* an int below 256 */
struct Ragged {
  int64_t counts[3];
  uint8_t meta[36];                                                // base | nnew
  int maxv_carried;                                                // maxv with {4, 0, 2} frames carried
};
const Ragged kRagged[6] = {
    {{0, 1, 5}, {B8(0), B8(0), B8(1), N4(0), N4(1), N4(5)}, 7}, {{0, 5, 1}, {B8(0), B8(0), B8(5), N4(0), N4(5), N4(1)}, 5},
    {{1, 0, 5}, {B8(0), B8(1), B8(1), N4(1), N4(0), N4(5)}, 7}, {{1, 5, 0}, {B8(0), B8(1), B8(6), N4(1), N4(5), N4(0)}, 5},
    {{5, 0, 1}, {B8(0), B8(5), B8(5), N4(5), N4(0), N4(1)}, 9}, {{5, 1, 0}, {B8(0), B8(5), B8(6), N4(5), N4(1), N4(0)}, 9},
};
const uint8_t kCarriedColumn[12] = {N4(4), N4(0), N4(2)};

void ragged_streams()
{
  const std::vector<int> carried = {4, 0, 2};
  for (const Who& w : kWho)
    for (const Ragged& r : kRagged) {
      const std::vector<int64_t> counts(r.counts, r.counts + 3);
      const EtiPush p = plan(w, counts, false);
      CHECK(p.refusal.empty() && p.total == 6 && p.maxv == 5 && p.nstreams == 3 && !p.carries);
      CHECK(p.meta.size() == 36 && !std::memcmp(p.meta.data(), r.meta, 36));
      if (!w.carries) continue;
      const EtiPush c = plan(w, counts, false, &carried);
      CHECK(c.refusal.empty() && c.total == 6 && c.maxv == r.maxv_carried && c.nstreams == 3 && c.carries);
      CHECK(c.meta.size() == 48 && !std::memcmp(c.meta.data(), r.meta, 36) && !std::memcmp(c.meta.data() + 36, kCarriedColumn, 12));
    }
}

void refusals()
{
  for (const Who& w : kWho) {
    const std::string who = w.name;
    const int64_t m = w.per_stream;
    // one stream, at the bound: taken, and the block is base 0 | nnew m
    const EtiPush at = plan(w, {m}, false);
    const int mi = static_cast<int>(m);
    const int64_t zero = 0;
    CHECK(at.refusal.empty() && at.total == m && at.maxv == mi && at.meta.size() == 12);
    CHECK(!std::memcmp(at.meta.data(), &zero, 8) && !std::memcmp(at.meta.data() + 8, &mi, 4));
    CHECK(plan(w, {m + 1}, false).refusal == who + ": bad frame count");
    CHECK(plan(w, {-1}, false).refusal == who + ": bad frame count");
    CHECK(plan(w, {1, m + 1}, false).refusal == who + ": bad frame count");
    CHECK(plan(w, {0, -1, 0}, true).refusal == who + ": bad frame count");       // before the null frames are looked at
    // every count legal, the total one over
    const EtiPush over = plan(w, {m, 1}, false), over_null = plan(w, {m, 1}, true);
    if (w.total < 0) {
      CHECK(over.refusal.empty() && over.total == m + 1 && over.maxv == mi);
      CHECK(over_null.refusal == who + ": null frames");
    } else {
      CHECK(over.refusal == who + ": too many frames for one push");
      CHECK(over_null.refusal == who + ": too many frames for one push");        // the total is checked first
      CHECK(plan(w, {m - 1, 1}, false).refusal.empty());
    }
    CHECK(plan(w, {1}, true).refusal == who + ": null frames");
    CHECK(plan(w, {0, 1, 0}, true).refusal == who + ": null frames");
    const EtiPush none = plan(w, {0, 0}, true);                                  // nothing to read: no pointer is needed
    CHECK(none.refusal.empty() && none.total == 0 && none.maxv == 0 && none.meta == std::vector<uint8_t>(24, 0));
    if (w.carries) {                                                             // carried frames count towards maxv, not towards the bound or the total
      const std::vector<int> four = {4};
      const EtiPush c = plan(w, {m}, false, &four);
      CHECK(c.refusal.empty() && c.total == m && c.maxv == mi + 4 && c.meta.size() == 16);
      const EtiPush idle = plan(w, {0}, true, &four);
      CHECK(idle.refusal.empty() && idle.total == 0 && idle.maxv == 4);
    }
  }
}

// ---- eti_stc_walk ----------------------------------------------------------------------------------------------------------------------------
struct Entry {
  int scid, stl;
};
struct Hit {
  int q, stl;
  bool fits;
  int off;
  bool operator==(const Hit& o) const { return q == o.q && stl == o.stl && fits == o.fits && off == o.off; }
};

// a frame of exactly 6144 bytes with this FC / STC; the bits around ficf, SCID and STL (FCT, SAD, TPL) are set, so a wrong mask shows
std::unique_ptr<uint8_t[]> frame(int ficf, const std::vector<Entry>& stc)
{
  std::unique_ptr<uint8_t[]> f(new uint8_t[DABHIP_ETI_BYTES]);
  std::memset(f.get(), 0xA5, DABHIP_ETI_BYTES);
  f[5] = static_cast<uint8_t>((ficf << 7) | static_cast<int>(stc.size()));
  for (size_t i = 0; i < stc.size(); ++i) {
    uint8_t* e = f.get() + 8 + 4 * i;
    e[0] = static_cast<uint8_t>((stc[i].scid << 2) | 3);
    e[1] = 0xff;
    e[2] = static_cast<uint8_t>(0xfc | (stc[i].stl >> 8));
    e[3] = static_cast<uint8_t>(stc[i].stl & 0xff);
  }
  return f;
}

// the rule, restated: the sub-channels' payloads follow the header (4 bytes of FC + 4 per entry + 4 of EOH, behind 4 of SYNC) and the FIC's 96
// bytes if it is there, in the order of their entries, 8 bytes per STL; an id's first entry is the one that counts
std::vector<Hit> restated(const uint8_t* f, const std::vector<int32_t>& subch)
{
  std::vector<Hit> hits;
  std::vector<bool> taken(subch.size(), false);
  const int nst = f[5] % 128;
  int at = 4 + 4 + 4 * nst + 4 + (f[5] >= 128 ? 96 : 0);
  for (int i = 0; i < nst; ++i) {
    const uint8_t* e = f + 8 + 4 * i;
    const int id = e[0] / 4, words = (e[2] % 4) * 256 + e[3];
    for (size_t q = 0; q < subch.size(); ++q)
      if (subch[q] == id && !taken[q]) {
        taken[q] = true;
        hits.push_back(Hit{static_cast<int>(q), words, at + 8 * words <= 6144, at});
      }
    at += 8 * words;
    if (at > 6144) break;
  }
  return hits;
}

std::vector<Hit> walked(int ficf, const std::vector<Entry>& stc, const std::vector<int32_t>& subch)
{
  const std::unique_ptr<uint8_t[]> f = frame(ficf, stc);
  std::unique_ptr<int32_t[]> ids(new int32_t[subch.size()]);       // exactly nsub entries
  for (size_t q = 0; q < subch.size(); ++q) ids[q] = subch[q];
  std::vector<Hit> hits;
  const uint8_t* f0 = f.get();
  eti_stc_walk(f0, ids.get(), static_cast<int>(subch.size()), [&](int q, int stl, bool fits, const uint8_t* p) { hits.push_back(Hit{q, stl, fits, static_cast<int>(p - f0)}); });
  CHECK(hits == restated(f0, subch));
  return hits;
}

void stc_walk()
{
  using Hits = std::vector<Hit>;
  std::vector<int32_t> all(64), all_reversed(64);
  for (int q = 0; q < 64; ++q) { all[q] = q; all_reversed[q] = 63 - q; }
  for (int ficf = 0; ficf < 2; ++ficf) {
    const int fic = 96 * ficf;
    // no entry; one entry, asked for or not, by one id and by 64
    CHECK(walked(ficf, {}, {5}).empty() && walked(ficf, {}, all).empty());
    CHECK(walked(ficf, {{5, 6}}, {5}) == Hits({{0, 6, true, 16 + fic}}));
    CHECK(walked(ficf, {{5, 6}}, {6}).empty());
    CHECK(walked(ficf, {{5, 6}}, all) == Hits({{5, 6, true, 16 + fic}}));
    // 64 entries of every id, 8 bytes each, asked for in the other order
    std::vector<Entry> full;
    for (int i = 0; i < 64; ++i) full.push_back({i, 1});
    const Hits h = walked(ficf, full, all_reversed);
    CHECK(h.size() == 64);
    for (int i = 0; i < 64; ++i) CHECK((h[i] == Hit{63 - i, 1, true, 12 + 256 + fic + 8 * i}));
    CHECK(walked(ficf, full, {63}) == Hits({{0, 1, true, 12 + 256 + fic + 8 * 63}}));
    // an id listed twice: the first entry counts, the second still takes its room
    CHECK(walked(ficf, {{7, 3}, {7, 6}, {9, 3}}, {9, 7}) == Hits({{1, 3, true, 24 + fic}, {0, 3, true, 24 + fic + 24 + 48}}));
    // an id asked for twice is found twice
    CHECK(walked(ficf, {{7, 3}}, {7, 7}) == Hits({{0, 3, true, 16 + fic}, {1, 3, true, 16 + fic}}));
  }
  // a payload that ends exactly at byte 6144 (16 + 8 * 766), and the least one past it: STLs count 8 bytes and the header 4, so that is 4 bytes
  CHECK(walked(0, {{1, 766}}, {1}) == Hits({{0, 766, true, 16}}));
  CHECK(walked(0, {{1, 767}}, {1}) == Hits({{0, 767, false, 16}}));
  CHECK(walked(0, {{1, 766}, {2, 0}}, {1, 2}) == Hits({{0, 766, false, 20}}));           // 20 + 6128 = 6148; the entry behind it is not reached
  CHECK(walked(1, {{1, 754}}, {1}) == Hits({{0, 754, true, 112}}));                      // 112 + 6032 = 6144
  CHECK(walked(1, {{1, 755}}, {1}) == Hits({{0, 755, false, 112}}));
  CHECK(walked(1, {{1, 753}, {2, 1}}, {2, 1}) == Hits({{1, 753, true, 116}, {0, 1, false, 6140}}));
  // the walk goes on behind a payload that ends exactly at the frame's end (32 + 8 * 764): an empty entry there fits, the next does not and ends it
  CHECK(walked(0, {{1, 764}, {2, 0}, {3, 1}, {4, 0}, {5, 0}}, {5, 4, 3, 2, 1}) == Hits({{4, 764, true, 32}, {3, 0, true, 6144}, {2, 1, false, 6144}}));
  // an STL that runs past the frame: the entries behind it are not reached
  CHECK(walked(0, {{1, 1023}, {2, 5}, {3, 5}}, {1, 2, 3}) == Hits({{0, 1023, false, 24}}));
  CHECK(walked(0, {{1, 5}, {2, 1023}, {3, 5}}, {3, 2, 1}) == Hits({{2, 5, true, 24}, {1, 1023, false, 64}}));
}
}  // namespace

int main()
{
  ragged_streams();
  refusals();
  stc_walk();
  std::printf("ok eti_push-units\n");
  return 0;
}
