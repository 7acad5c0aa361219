// ts_units.cpp — the host-and-device header of the MPEG-2 TS stage (csrc/ts_sync.hpp) under ASan + UBSan, as a stand-alone program:
// ts_chunk_step against the rule slot by slot, the position map against a linear search, and a lane driven the way the sync kernel's wave drives
// it (run flags, the search over them, 64 slots per step) over arrays of exactly the planned sizes -- a carry of 2447 bytes, unit slots of
// ts_unit_bound -- against the rule byte by byte.  Any cutting of a stream into pushes must give the same units.  Prints "ok ts-units", the
// fullest slot array and the largest carry it saw.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../dabtools_amd/csrc/ts_sync.hpp"

using namespace dabhip;

namespace {
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// ---- ts_chunk_step against the rule, one slot at a time ---------------------------------------------------------------------------------------
TsChunkStep serial_step(uint64_t hits, int nvalid, int misses)
{
  TsChunkStep r{0, 0, 0, 0};
  for (int i = 0; i < nvalid; ++i) {
    const bool hit = hits >> i & 1;
    if (hit) {
      misses = 0;
    } else if (++misses == kTsMissLimit) {
      r.lost = 1;
      r.misses = 0;
      return r;
    } else {
      r.from_miss |= uint64_t{1} << i;
    }
    ++r.npackets;
  }
  r.misses = misses;
  return r;
}

long check_step(uint64_t hits, int nvalid, int misses_in)
{
  const TsChunkStep a = ts_chunk_step(hits, nvalid, misses_in), b = serial_step(hits, nvalid, misses_in);
  CHECK(a.npackets == b.npackets && a.lost == b.lost && a.from_miss == b.from_miss && a.misses == b.misses);
  return 1;
}

long chunk_steps(std::mt19937_64& rng)
{
  long n = 0;
  for (int mi = 0; mi < kTsMissLimit; ++mi)
    for (int nvalid = 1; nvalid <= kTsChunk; ++nvalid) {
      const uint64_t valid = nvalid == 64 ? ~uint64_t{0} : (uint64_t{1} << nvalid) - 1;
      // every mask of the low 12 slots (all masks of a chunk of 12 or fewer), the rest hits; the same above garbage in the invalid bits
      for (uint64_t m = 0; m < 4096; ++m) {
        n += check_step(~m, nvalid, mi);
        n += check_step(~m & valid, nvalid, mi);
      }
      // misses at the chunk's two borders only: every pattern of the lowest 4 and the highest 4 valid slots
      for (uint64_t lo = 0; lo < 16; ++lo)
        for (uint64_t hi = 0; hi < 16; ++hi) {
          const uint64_t miss = (lo | (nvalid >= 4 ? hi << (nvalid - 4) : hi >> (4 - nvalid))) & valid;
          n += check_step(~miss, nvalid, mi);
        }
      // random masks at several miss densities
      for (int i = 0; i < 1600; ++i) {
        uint64_t miss = rng();
        for (int d = i % 5; d > 0; --d) miss &= rng();
        n += check_step(~miss, nvalid, mi);
      }
    }
  return n;
}

// ---- the position map ----------------------------------------------------------------------------------------------------------------------------
void position_map(std::mt19937_64& rng)
{
  for (int round = 0; round < 2000; ++round) {
    const int nnew = 1 + static_cast<int>(rng() % 70), ncar = static_cast<int>(rng() % (kTsCarry + 1));
    std::vector<int32_t> byte0(static_cast<size_t>(nnew)), bytes(static_cast<size_t>(nnew));
    int32_t nv = ncar;
    for (int v = 0; v < nnew; ++v) {
      bytes[v] = rng() % 3 == 0 ? 0 : 8 * static_cast<int32_t>(1 + rng() % kTsStlMax);   // frames that give no bytes among them
      byte0[v] = nv;
      nv += bytes[v];
    }
    for (int i = 0; i < 200 && nv > ncar; ++i) {
      const int32_t u = i == 0 ? ncar : (i == 1 ? nv - 1 : ncar + static_cast<int32_t>(rng() % static_cast<uint64_t>(nv - ncar)));
      const int f = ts_frame_of(nnew, u, [&](int v) { return byte0[static_cast<size_t>(v)]; });
      CHECK(f >= 0 && f < nnew && bytes[f] > 0 && byte0[f] <= u && u < byte0[f] + bytes[f]);
    }
  }
  for (int k = 0; k < kTsSlot; ++k) CHECK(ts_byte_pos(1000, k) >= 1000 && ts_byte_pos(1000, k) < 1000 + kTsLook);
  CHECK(ts_byte_pos(0, 0) == 0 && ts_byte_pos(0, kTsSlot - 1) == kTsLook - 1);
}

// ---- a lane ----------------------------------------------------------------------------------------------------------------------------------------
struct Unit {
  int64_t pos;
  int flags;
  bool operator==(const Unit& o) const { return pos == o.pos && flags == o.flags; }
};

struct Counters {
  int64_t skipped = 0, losses = 0;
  bool operator==(const Counters& o) const { return skipped == o.skipped && losses == o.losses; }
};

// the rule byte by byte, as dabhip.h words it, over the bytes on hand
struct SerialLane {
  std::vector<uint8_t> buf;
  int64_t base = 0;
  bool synced = false;
  int misses = 0;
  std::vector<Unit> units;
  Counters c;

  void rule()
  {
    const int64_t end = static_cast<int64_t>(buf.size());
    int64_t q = 0;
    for (;;) {
      if (!synced) {
        int64_t p = q;
        for (; p + kTsRunSpan < end; ++p) {
          bool run = true;
          for (int i = 0; i < kTsRun && run; ++i) run = buf[static_cast<size_t>(p + kTsSlot * i)] == kTsSyncByte;
          if (run) break;
        }
        if (p + kTsRunSpan < end) {
          c.skipped += p - q;
          q = p;
          synced = true;
          misses = 0;
        } else {
          const int64_t wait = std::max(q, end - kTsRunSpan);
          c.skipped += wait - q;
          q = wait;
          break;
        }
      } else {
        if (q + kTsLook > end) break;
        const bool hit = buf[static_cast<size_t>(q)] == kTsSyncByte;
        misses = hit ? 0 : misses + 1;
        if (misses == kTsMissLimit) {
          ++c.losses;
          ++c.skipped;
          synced = false;
          misses = 0;
          ++q;
          continue;
        }
        units.push_back(Unit{base + q, hit ? 0 : DABHIP_TS_FROM_MISS});
        q += kTsSlot;
      }
    }
    base += q;
    buf.erase(buf.begin(), buf.begin() + q);
  }
  void push(const uint8_t* b, int64_t n)
  {
    buf.insert(buf.end(), b, b + n);
    rule();
  }
  void brk()
  {
    c.skipped += static_cast<int64_t>(buf.size());
    if (synced) ++c.losses;
    base += static_cast<int64_t>(buf.size());
    buf.clear();
    synced = false;
    misses = 0;
  }
};

int g_fullest_n = 0, g_fullest_cap = 1, g_max_carry = 0;

// the loops of ts_runs_kernel and ts_sync_kernel with the wave's 64 lanes as a loop
struct WaveLane {
  TsSync st{};
  std::vector<uint8_t> carry = std::vector<uint8_t>(kTsCarry);   // exactly the bytes a lane may carry
  std::vector<Unit> units;
  Counters c;

  // nframes frames of 8 stl bytes; break_at >= 0: the stream breaks in front of that new frame
  void push(const uint8_t* b, int nframes, int stl, int break_at = -1)
  {
    const int ncar = st.ncar;
    CHECK(ncar >= 0 && ncar <= kTsCarry);
    const int64_t cap = ts_unit_bound(ncar, nframes, stl);
    std::vector<Unit> slots(static_cast<size_t>(cap));            // exactly the slots the bound gives
    const int nv = ncar + nframes * 8 * stl;
    std::vector<uint8_t> all(static_cast<size_t>(nv));             // virtual positions: the carried bytes, then the new
    std::copy(carry.begin(), carry.begin() + ncar, all.begin());
    std::copy(b, b + nframes * 8 * stl, all.begin() + ncar);
    const int brk_pos = break_at >= 0 ? ncar + break_at * 8 * stl : -1;
    const auto seg = [&](int u) { return brk_pos >= 0 && u >= brk_pos ? 1 : 0; };
    // runs: a bit per position, 64 to a word
    std::vector<uint64_t> flags(static_cast<size_t>((nv + 63) / 64), 0);
    for (int p = 0; p + kTsRunSpan < nv; ++p) {
      bool run = seg(p) == seg(p + kTsRunSpan);
      for (int i = 0; i < kTsRun && run; ++i) run = all[static_cast<size_t>(p + kTsSlot * i)] == kTsSyncByte;
      if (run) flags[static_cast<size_t>(p >> 6)] |= uint64_t{1} << (p & 63);
    }
    const auto find_run = [&](int from, int end) {
      const int w0 = from >> 6, wend = (end + 63) >> 6;
      for (int wb = w0; wb < wend; wb += 64)
        for (int l = 0; l < 64; ++l) {
          const int w = wb + l;
          uint64_t x = w < wend ? flags[static_cast<size_t>(w)] : 0;
          if (w == w0) x &= ~uint64_t{0} << (from & 63);
          if (!x) continue;
          const int p = w * 64 + __builtin_ctzll(x);
          return p < end ? p : -1;
        }
      return -1;
    };
    int lo = 0, n = 0;
    const int64_t base = st.next_pos - ncar;
    const auto segment = [&](int end) {
      for (;;) {
        if (!st.synced) {
          const int p = find_run(lo, end);
          if (p < 0) {
            const int wait = static_cast<int>(ts_search_wait(lo, end));
            c.skipped += wait - lo;
            lo = wait;
            return;
          }
          c.skipped += p - lo;
          lo = p;
          st.synced = 1;
          st.misses = 0;
        }
        const int64_t ready = ts_slots_ready(end - lo);
        if (ready <= 0) return;
        const int m = static_cast<int>(std::min<int64_t>(ready, kTsChunk));
        uint64_t hits = 0;
        for (int l = 0; l < m; ++l)
          if (all[static_cast<size_t>(lo + kTsSlot * l)] == kTsSyncByte) hits |= uint64_t{1} << l;
        const TsChunkStep r = ts_chunk_step(hits, m, st.misses);
        for (int l = 0; l < r.npackets; ++l) {
          CHECK(n + l < cap);
          CHECK(lo + kTsSlot * l + kTsLook <= end);
          slots[static_cast<size_t>(n + l)] = Unit{base + lo + kTsSlot * l, (r.from_miss >> l & 1) ? DABHIP_TS_FROM_MISS : 0};
        }
        n += r.npackets;
        lo += kTsSlot * r.npackets;
        if (r.lost) {
          ++c.losses;
          ++c.skipped;
          ++lo;
          st.synced = 0;
          st.misses = 0;
        } else {
          st.misses = r.misses;
        }
      }
    };
    if (brk_pos >= 0) {
      segment(brk_pos);
      c.skipped += brk_pos - lo;
      if (st.synced) ++c.losses;
      st.synced = st.misses = 0;
      lo = brk_pos;
    }
    segment(nv);
    CHECK(nv - lo <= kTsCarry);
    g_max_carry = std::max(g_max_carry, nv - lo);
    std::vector<uint8_t> next(kTsCarry);
    std::copy(all.begin() + lo, all.end(), next.begin());
    carry.swap(next);
    st.ncar = nv - lo;
    st.next_pos = base + nv;
    units.insert(units.end(), slots.begin(), slots.begin() + n);
    const int64_t mine = static_cast<int64_t>(n) * g_fullest_cap, best = static_cast<int64_t>(g_fullest_n) * cap;
    if (cap > 0 && (mine > best || (mine == best && cap > g_fullest_cap))) {      // as full, and larger
      g_fullest_n = n;
      g_fullest_cap = static_cast<int>(cap);
    }
  }
};

// an interleaver-shaped stream: 0x47 every 204 bytes from `phase`, noise elsewhere, then sync bytes knocked out and bytes cut out
std::vector<uint8_t> make_stream(std::mt19937_64& rng, int64_t n, int kind)
{
  std::vector<uint8_t> s(static_cast<size_t>(n));
  for (auto& b : s) b = kind == 3 ? kTsSyncByte : static_cast<uint8_t>(rng());
  if (kind == 3) return s;                                         // 0x47 everywhere: synced at once, every slot a hit
  const int phase = static_cast<int>(rng() % kTsSlot);
  for (int64_t p = phase; p < n; p += kTsSlot) s[static_cast<size_t>(p)] = kTsSyncByte;
  if (kind >= 1)
    for (int64_t p = phase; p < n; p += kTsSlot)
      if (rng() % (kind == 1 ? 9 : 3) == 0) s[static_cast<size_t>(p)] = 0;      // misses: now and then, or so often that sync is lost again and again
  if (kind == 2 && n > 4000) s.erase(s.begin() + 3000 + static_cast<int64_t>(rng() % 500), s.begin() + 3507);   // a slip
  return s;
}

void lanes(std::mt19937_64& rng)
{
  const int stls[] = {1, 3, 24, 26, 51, 204, 205, 306, kTsStlMax};
  const int pushes[] = {1, 2, 3, 64};
  for (int stl : stls)
    for (int kind = 0; kind < 4; ++kind) {
      const int per = 8 * stl;
      const int nframes = std::max(70, 3 * kTsLook / per + 140);
      std::vector<uint8_t> s = make_stream(rng, static_cast<int64_t>(nframes) * per + 600, kind);
      const int nf = static_cast<int>(s.size() / per);
      std::vector<Unit> first;
      Counters first_c;
      for (size_t pi = 0; pi <= 4; ++pi) {                         // pushes of 1, 2, 3 and 64 frames, then random cuts
        WaveLane w;
        SerialLane ref;
        for (int at = 0; at < nf;) {
          const int take = std::min(nf - at, pi < 4 ? pushes[pi] : static_cast<int>(rng() % 9));
          const int brk = (pi == 4 && take > 0 && rng() % 11 == 0) ? static_cast<int>(rng() % take) : -1;
          w.push(s.data() + static_cast<size_t>(at) * per, take, stl, brk);
          if (brk >= 0) {
            ref.push(s.data() + static_cast<size_t>(at) * per, static_cast<int64_t>(brk) * per);
            ref.brk();
            ref.push(s.data() + static_cast<size_t>(at + brk) * per, static_cast<int64_t>(take - brk) * per);
          } else {
            ref.push(s.data() + static_cast<size_t>(at) * per, static_cast<int64_t>(take) * per);
          }
          at += take;
        }
        CHECK(w.units == ref.units && w.c == ref.c);
        CHECK(w.st.next_pos == ref.base + static_cast<int64_t>(ref.buf.size()) && w.st.ncar == static_cast<int>(ref.buf.size()));
        if (pi == 0) {
          first = w.units;
          first_c = w.c;
          CHECK(!first.empty());
        } else if (pi < 4) {
          CHECK(w.units == first && w.c == first_c);              // any cutting without breaks: the same units
        }
      }
    }
}

// the bound as a property: STL 1 .. 766, carried bytes 0 .. 2447, pushes of 1, 2, 3 and 64 frames.  A lane that comes in synced with its next
// slot at its first carried byte and meets nothing but hits gives a unit for every slot that has its look-ahead: the bound exactly, never more.
void unit_bound()
{
  const int pushes[] = {1, 2, 3, 64};
  std::vector<uint8_t> hits(static_cast<size_t>(64) * kTsFrameBytesMax, kTsSyncByte);
  for (int stl = 1; stl <= kTsStlMax; ++stl)
    for (int ncar = 0; ncar <= kTsCarry; ++ncar)
      for (int nframes : pushes) {
        const int64_t have = ncar + static_cast<int64_t>(nframes) * 8 * stl, bound = ts_unit_bound(ncar, nframes, stl);
        CHECK(bound >= 0 && bound == ts_slots_ready(have));
        CHECK(bound == 0 ? have < kTsLook : (kTsSlot * (bound - 1) + kTsLook <= have && kTsSlot * bound + kTsLook > have));
        CHECK(bound * kTsSlot <= have);                            // ts.cpp's bound on all units of a push: 204 bytes of its own lane each
        // the lane itself, over exactly that many slots, where it is cheap: at the corners and on a sparse grid
        const bool corner = (stl <= 2 || stl == 51 || stl == kTsStlMax) && (ncar == 0 || ncar == kTsCarry || ncar % 611 == 0);
        if (!corner) continue;
        WaveLane w;
        w.st.synced = 1;
        w.st.ncar = ncar;
        w.st.next_pos = ncar;
        std::fill(w.carry.begin(), w.carry.end(), static_cast<uint8_t>(kTsSyncByte));
        w.push(hits.data(), nframes, stl);
        CHECK(static_cast<int64_t>(w.units.size()) == bound);
      }
}
}  // namespace

int main()
{
  std::mt19937_64 rng(20427);
  const long steps = chunk_steps(rng);
  position_map(rng);
  lanes(rng);
  unit_bound();
  std::printf("ok ts-units\n");
  std::printf("%ld chunk steps; fullest %d of %d slots; largest carry %d of %d\n", steps, g_fullest_n, g_fullest_cap, g_max_carry, kTsCarry);
  return 0;
}
