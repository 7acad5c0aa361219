// packet_units.cpp — the host-only parts of the packet-mode stage under ASan + UBSan, as a stand-alone program: the data-group rule
// (csrc/packet_groups.hpp) on every drop and on groups cut short, and the FEC sync rule (csrc/packet_sync.hpp) driven the way the sync kernel's
// lane drives it, over arrays of exactly the planned sizes: a carry of 102 cells, unit slots of the capacity packet.cpp plans for a push.  Any
// cutting of a stream into pushes must give the same units, at 1 .. 255 cells per ETI frame.  slot_bound() holds that capacity as a property: at
// every rate, carried count and push size, header streams built to give as many units as the rule allows, and random ones, never fill the slots.
// Prints "ok packet-units" and the fullest slot array it saw.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../dabtools_amd/csrc/packet_groups.hpp"
#include "../../dabtools_amd/csrc/packet_sync.hpp"

using namespace dabhip;

namespace {
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Unit {
  int64_t cell;
  int flags;
  bool operator==(const Unit& o) const { return cell == o.cell && flags == o.flags; }
};

// one lane over the FEC counters of its cells, s cells per frame, `chunk` frames per push: the loop of packet_sync_kernel with the cells'
// counters in place of the cells
struct LaneSim {
  PacketSync st{};
  std::vector<uint8_t> carry = std::vector<uint8_t>(kPkCarry);   // exactly the carry buffer's cells
  std::vector<Unit> units;
  int64_t skipped = 0, losses = 0, misses = 0;
  int last_n = 0, last_cap = 1;                                  // units and slots of the last push

  // break_every > 0: the stream breaks in front of new frames break_every, 2 break_every, ... of this push (packet_break, as at a frame whose STL
  // differs)
  void push(const uint8_t* h, int nframes, int s, int break_every = 0)
  {
    const int cap = std::max(nframes, (kPkCarry + nframes * 256) / kPkFrameCells + 1) + 1;   // packet.cpp
    std::vector<Unit> slots(static_cast<size_t>(cap));            // exactly the slots of this push
    int n = 0;
    PacketWalkState w{};
    w.st = st;
    const int ncar = st.ncar;
    CHECK(ncar >= 0 && ncar <= kPkCarry);
    const int64_t base = st.next_cell - ncar;
    const int total = ncar + nframes * s;
    std::vector<uint8_t> all(static_cast<size_t>(total));         // virtual cells: the carried, then the new
    std::copy(carry.begin(), carry.begin() + ncar, all.begin());
    std::copy(h, h + nframes * s, all.begin() + ncar);
    const auto emit = [&](int32_t u0, int flags) {
      CHECK(n < cap);
      CHECK(u0 >= 0 && u0 + kPkFrameCells <= total);
      slots[n++] = Unit{base + u0, flags};
    };
    const uint8_t* cells = all.data();
    int next_break = break_every > 0 ? ncar + break_every * s : total;
    for (int nv = ncar; nv < total; ++nv) {
      if (nv == next_break) {
        packet_break(w, nv);
        next_break += break_every * s;
      }
      if (packet_feed(w, nv, cells[nv], emit)) {
        CHECK(w.lo >= 0 && nv - w.lo == kPkFrameCells - 1);
        for (int u = w.lo + 1; u <= nv; ++u) CHECK(!packet_feed(w, u, all[u], emit));
      }
    }
    packet_push_end(w, total);
    CHECK(w.st.ncar >= 0 && w.st.ncar <= kPkCarry && w.lo + w.st.ncar == total);
    for (int i = 0; i < w.st.ncar; ++i) carry[i] = all[w.lo + i];
    w.st.next_cell = base + total;
    st = w.st;
    skipped += w.skipped;
    losses += w.losses;
    misses += w.misses;
    units.insert(units.end(), slots.begin(), slots.begin() + n);
    last_n = n;
    last_cap = cap;
  }
};

// cells of FEC frames with every header in place, from cell `phase` of a frame on
void perfect(std::vector<uint8_t>& h, int count, int phase = 0)
{
  const size_t at = h.size();
  h.resize(at + static_cast<size_t>(count));
  uint8_t* p = h.data() + at;
  for (int i = 0; i < count; ++i, phase = phase + 1 == kPkFrameCells ? 0 : phase + 1) p[i] = phase < kPkDataCells ? kPkNoCounter : static_cast<uint8_t>(phase - kPkDataCells);
}

struct Fullest {
  int n = 0, cap = 1, s = 0, car = 0, maxv = 0;
  void see(const LaneSim& l, int s_, int car_, int maxv_)
  {
    CHECK(l.last_n <= l.last_cap);
    if (static_cast<int64_t>(l.last_n) * cap > static_cast<int64_t>(n) * l.last_cap) *this = Fullest{l.last_n, l.last_cap, s_, car_, maxv_};
  }
};

// The units of one push against the slots packet.cpp plans for it (LaneSim::push CHECKs every unit against them).  A lane's units never share a
// cell, so floor((carried + new cells) / 103) is the most any stream can give; the built streams give exactly that, the others come close.
Fullest slot_bound()
{
  Fullest worst;
  const int sizes[] = {1, 2, 3, 64};
  const int longest = 64 * 255 + 5 * kPkFrameCells;
  // whole frames; and a whole frame, two frames without headers, a third with headers 0 .. 8 on its cells 1 .. 9, whole frames from its cell 10 on
  std::vector<uint8_t> whole, lost;
  perfect(whole, longest);
  perfect(lost, kPkFrameCells);
  lost.insert(lost.end(), 2 * kPkFrameCells + 1, kPkNoCounter);
  for (int i = 0; i < kPkFecCells; ++i) lost.push_back(static_cast<uint8_t>(i));
  perfect(lost, longest);
  // a: an unsynced lane that carries the first cells of a frame: the run of nine completes at the first possible cell, then hits back to back
  // b: a synced lane that carries the first cells of a frame: hits back to back
  // c: as b, the stream breaking every few frames and starting anew with a whole frame (as often as still lets a unit through)
  // d: a synced lane with two misses that carries the first cells of a third frame without headers; a run of nine inside the 103 cells searched
  //    again, frames with every header behind it
  // e: as d, cut in the first of the three frames: two units from misses, the loss and the new run in one push
  // the lanes as the push before left them, by kind and carried count
  const int heads[5] = {0, kPkFrameCells, kPkFrameCells, 3 * kPkFrameCells, kPkFrameCells};
  std::vector<LaneSim> before(5 * (kPkCarry + 1));
  for (int kind = 0; kind < 5; ++kind)
    for (int car = 0; car <= kPkCarry; ++car) {
      LaneSim& lane = before[kind * (kPkCarry + 1) + car];
      lane.push((kind < 3 ? whole : lost).data(), heads[kind] + car, 1);
      CHECK(lane.st.ncar == car && lane.st.synced == (kind != 0));
      if (kind >= 3) CHECK(lane.st.misses == (kind == 3 ? 2 : 0) && lane.units.size() == (kind == 3 ? 3u : 1u));
    }
  std::vector<uint8_t> h;
  for (int s = 1; s <= 255; ++s)
    for (int car = 0; car <= kPkCarry; ++car)
      for (const int maxv : sizes) {
        const int fresh = maxv * s;
        for (int kind = 0; kind < 5; ++kind) {
          if (maxv == 64 && kind >= 1 && (s + car) % 8) continue;             // (the long pushes but a: every eighth (rate, carried count))
          LaneSim lane = before[kind * (kPkCarry + 1) + car];
          const int every = (kPkFrameCells + s - 1) / s;
          if (kind == 2) {
            h.clear();
            for (int f = 0; f < maxv; ++f) perfect(h, s, (f < every ? car + f * s : (f % every) * s) % kPkFrameCells);
            lane.push(h.data(), maxv, s, every);
          } else {
            lane.push((kind < 3 ? whole : lost).data() + heads[kind] + car, maxv, s);
          }
          worst.see(lane, s, car, maxv);
          if (kind <= 1) CHECK(lane.last_n == (car + fresh) / kPkFrameCells);   // the most there can be
          if (kind == 2 && s >= kPkFrameCells) CHECK(lane.last_n >= maxv * (s / kPkFrameCells) - 1);
          if (kind == 3 && car + fresh >= kPkFrameCells) CHECK(lane.losses == 1);
          if (kind == 3 && car + fresh >= 10 + 2 * kPkFrameCells) CHECK(lane.last_n == (car + fresh - 10) / kPkFrameCells);
          if (kind == 4 && car + fresh >= 10 + 4 * kPkFrameCells) CHECK(lane.losses == 1 && lane.misses == 2 && lane.last_n == 2 + (car + fresh - 10 - 2 * kPkFrameCells) / kPkFrameCells);
        }
      }
  // random streams, 2000 per rate: frames from a random phase on, headers lost, stray headers, frames without headers up to four in a row, cells
  // slipped; pushes of 1, 2, 3 and (one in 64) 64 frames, breaks in some; every push is held to its slots
  uint64_t x = 88172645463325252ull;
  const auto next = [&x]() {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int s = 1; s <= 255; ++s)
    for (int trial = 0; trial < 2000; ++trial) {
      LaneSim lane;
      int phase = static_cast<int>(next() % kPkFrameCells), dead = 0;
      const uint32_t loss = 2 + static_cast<uint32_t>(next() % 80), stray = 1 + static_cast<uint32_t>(next() % 40);     // of 256, of 1024
      for (int push = 0; push < 2; ++push) {
        const int maxv = next() % 64 == 0 ? 64 : sizes[next() % 3];
        h.resize(static_cast<size_t>(maxv * s));
        uint8_t* p = h.data();
        for (int i = 0; i < maxv * s; ++i) {
          const uint64_t r = next();
          if (phase == 0) dead = dead ? dead - 1 : ((r >> 50) % 9 == 0 ? 1 + static_cast<int>((r >> 56) & 3) : 0);
          if (phase < kPkDataCells) p[i] = (r & 1023) < stray ? static_cast<uint8_t>(((r >> 10 & 15) * kPkFecCells) >> 4) : kPkNoCounter;
          else p[i] = dead || (r >> 16 & 255) < loss ? kPkNoCounter : static_cast<uint8_t>(phase - kPkDataCells);
          phase += 1 + ((r >> 24 & 2047) == 0 ? static_cast<int>(r >> 40 & 31) : 0);
          if (phase >= kPkFrameCells) phase -= kPkFrameCells;
        }
        const int car = lane.st.ncar;
        lane.push(h.data(), maxv, s, next() % 4 == 0 ? 1 + static_cast<int>(next() % 3) : 0);
        worst.see(lane, s, car, maxv);
      }
    }
  return worst;
}

void sync_rule()
{
  std::mt19937 rng(12345);
  for (int trial = 0; trial < 40; ++trial) {
    // a stream of frames with a random start phase, headers lost at random, some frames with every header lost (three in a row at times), cells
    // slipped, and stray headers among the data cells
    std::vector<uint8_t> h;
    for (int i = static_cast<int>(rng() % kPkFrameCells); i > 0; --i) h.push_back(kPkNoCounter);
    int dead = 0;
    for (int f = 0; f < 120; ++f) {
      if (dead == 0 && rng() % 9 == 0) dead = 1 + static_cast<int>(rng() % 4);
      for (int c = 0; c < kPkDataCells; ++c) h.push_back(rng() % 50 == 0 ? static_cast<uint8_t>(rng() % kPkFecCells) : kPkNoCounter);
      for (int c = 0; c < kPkFecCells; ++c) h.push_back(dead || rng() % 12 == 0 ? kPkNoCounter : static_cast<uint8_t>(c));
      if (dead) --dead;
      if (rng() % 20 == 0) h.resize(h.size() - rng() % 40);
    }
    std::vector<Unit> first;
    int64_t first_skipped = 0, first_losses = 0;
    const int plans[][2] = {{1, 1 << 20}, {1, 1}, {1, 50}, {1, 103}, {4, 7}, {8, 3}, {255, 1}, {3, 40}, {9, 1}, {9, 5}, {16, 2}, {17, 1}, {17, 64}, {102, 1},
                            {102, 3}, {103, 1}, {103, 2}, {104, 1}, {104, 64}, {206, 1}, {206, 2}, {251, 1}, {251, 64}};
    for (const auto& plan : plans) {
      const int s = plan[0], chunk = plan[1];
      const int nframes = static_cast<int>(h.size()) / s;
      LaneSim lane;
      for (int a = 0; a < nframes; a += chunk) {
        const int n = std::min(chunk, nframes - a);
        lane.push(h.data() + static_cast<size_t>(a) * s, n, s);
      }
      const int64_t sent = static_cast<int64_t>(nframes) * s;
      CHECK(static_cast<int64_t>(lane.units.size()) * kPkFrameCells + lane.skipped + lane.st.ncar == sent);
      for (size_t i = 1; i < lane.units.size(); ++i) CHECK(lane.units[i].cell >= lane.units[i - 1].cell + kPkFrameCells);
      if (s == 1) {
        if (first.empty()) {
          first = lane.units;
          first_skipped = lane.skipped;
          first_losses = lane.losses;
          CHECK(first.size() > 20);
        }
        CHECK(lane.units == first && lane.skipped == first_skipped && lane.losses == first_losses);
      } else {
        // the same stream less the cells that fill no whole frame: the units that end inside it are the same
        size_t k = 0;
        while (k < first.size() && first[k].cell + kPkFrameCells <= sent - kPkFrameCells) ++k;
        CHECK(lane.units.size() >= k);
        for (size_t i = 0; i < k; ++i) CHECK(lane.units[i] == first[i]);
      }
    }
  }
  CHECK(fec_counter(0x03, 0xfe) == 0 && fec_counter(0x23, 0xfe) == 8 && fec_counter(0x27, 0xfe) == kPkNoCounter && fec_counter(0x43, 0xfe) == kPkNoCounter &&
        fec_counter(0x03, 0xff) == kPkNoCounter && fec_counter(0x02, 0xfe) == kPkNoCounter);
  for (int r = 0; r < kPkRows; ++r)
    for (int c = 0; c < kPkN; ++c) {
      const int o = fec_byte_offset(r, c);
      CHECK(o >= 0 && o < kPkFrameCells * kPkCell);
      if (c >= kPkK) CHECK(o >= kPkTable && o % kPkCell >= 2);
    }
  CHECK(fec_byte_offset(11, 203) == (kPkDataCells + 8) * kPkCell + 2 + 15);
}

dabhip_packet_rec rec(int64_t cell, int address, int ci, int fl, int ulen, int cmd = 0)
{
  dabhip_packet_rec r{};
  r.cell = cell;
  r.address = static_cast<uint16_t>(address);
  r.length = 1;
  r.continuity = static_cast<uint8_t>(ci);
  r.first_last = static_cast<uint8_t>(fl);
  r.command = static_cast<uint8_t>(cmd);
  r.useful_length = static_cast<uint8_t>(ulen);
  return r;
}

void group_rule()
{
  PacketGroups g;
  // exactly-sized useful bytes: a read past a packet's bytes is an ASan error
  const auto feed = [&g](const dabhip_packet_rec& r, uint8_t fill) {
    std::vector<uint8_t> u(r.useful_length, fill);
    g.packet(r, u.data());
  };
  feed(rec(0, 5, 0, 0, 10), 1);                                  // orphan
  feed(rec(1, 5, 0, 2, 19), 2);
  feed(rec(2, 5, 1, 0, 19), 3);
  feed(rec(3, 5, 2, 1, 7), 4);                                   // a group of 45 bytes
  CHECK(g.done.size() == 1 && g.done[0].length == 45 && g.done_bytes[0][18] == 2 && g.done_bytes[0][44] == 4);
  feed(rec(4, 5, 0, 2, 19), 5);
  feed(rec(5, 5, 2, 1, 19), 6);                                  // continuity skips: dropped
  feed(rec(6, 5, 3, 1, 19), 7);                                  // orphan
  feed(rec(7, 0, 0, 3, 19), 8);                                  // padding
  feed(rec(8, 5, 0, 3, 19, 1), 9);                               // command
  CHECK(g.done.size() == 1 && g.counters[kGrpDropped] == 1 && g.counters[kGrpOrphans] == 2);
  feed(rec(9, 6, 0, 2, 91), 0);
  int ci = 0;
  for (int i = 0; i < 89; ++i) feed(rec(10 + i, 6, ci = (ci + 1) & 3, 0, 91), 0);        // 90 x 91 = 8190
  feed(rec(100, 6, ci = (ci + 1) & 3, 0, 18), 0);                // 8208: the largest group
  feed(rec(101, 6, (ci + 1) & 3, 1, 0), 0);
  CHECK(g.done.size() == 2 && g.done[1].length == kPkMaxGroup && g.counters[kGrpDropped] == 1);
  feed(rec(102, 6, 0, 2, 91), 0);
  ci = 0;
  for (int i = 0; i < 89; ++i) feed(rec(103 + i, 6, ci = (ci + 1) & 3, 0, 91), 0);
  feed(rec(200, 6, (ci + 1) & 3, 1, 19), 0);                     // 8209: dropped
  CHECK(g.done.size() == 2 && g.counters[kGrpDropped] == 2 && g.open.empty());
  // groups cut short of the header their flags announce, and a CRC over a group of exactly 4 bytes
  const uint8_t full[] = {0xF1, 0x23, 0xAB, 0xCD, 0x80, 0x07, 0x12, 0x55, 0x66, 0x99, 0, 0};
  for (size_t n = 0; n <= sizeof full; ++n) {
    std::vector<uint8_t> b(full, full + n);
    const dabhip_packet_group r = parse_group(9, b);
    CHECK(r.length == static_cast<int32_t>(n));
    if (n < 11) CHECK(!r.header_ok && r.segment_number == -1 && r.transport_id == -1);
    if (n == 11) CHECK(r.header_ok && r.transport_id == 0x5566);
    if (n == 12) CHECK(r.header_ok && r.ext_field == 0xABCD && r.last_segment == 1 && r.segment_number == 7 && r.transport_id == 0x5566 && r.type == 1 && r.continuity == 2 &&
                       r.repetition == 3 && r.crc_flag && !r.crc_ok);
  }
  std::vector<uint8_t> four = {0x40, 0x00, 0, 0};
  const uint16_t c = static_cast<uint16_t>(~crc16_ccitt(four.data(), 2));
  four[2] = static_cast<uint8_t>(c >> 8);
  four[3] = static_cast<uint8_t>(c & 0xff);
  CHECK(parse_group(1, four).crc_ok && parse_group(1, four).header_ok);
  // push(): records whose useful lengths pass the bytes on hand are refused before any read
  std::vector<dabhip_packet_rec> recs = {rec(0, 7, 0, 3, 10), rec(1, 7, 1, 3, 10)};
  std::vector<uint8_t> data(19, 0);
  CHECK(!g.push(recs.data(), 2, data.data(), 19));
  data.push_back(0);
  CHECK(g.push(recs.data(), 2, data.data(), 20) && g.done.size() == 2);
}
}  // namespace

int main()
{
  sync_rule();
  group_rule();
  const Fullest w = slot_bound();
  std::printf("ok packet-units\nfullest %d of %d slots: %d cells per frame, %d carried, %d frames\n", w.n, w.cap, w.s, w.car, w.maxv);
  return 0;
}
