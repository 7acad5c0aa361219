// packet_sync.hpp — the sizes of the packet-mode stage and its FEC sync rule, one cell at a time, free of HIP: the sync kernel's lane
// (k_packet.hip, through packet.hpp) and tests/host_sanitize/packet_units.cpp run this text.  dabhip.h (dabhip_packet) has the rule in words.
#pragma once

#include <cstdint>

#include "../../include/dabhip.h"

#ifdef __HIPCC__
#define DABHIP_PK_HD __host__ __device__
#else
#define DABHIP_PK_HD
#endif

namespace dabhip {

// A sub-channel of 8 s kbit/s carries s cells of 24 bytes per ETI frame.  An FEC frame is 94 data cells (the 2256-byte application table) and
// 9 FEC cells of 2 header and 22 RS bytes: 192 parity bytes, then 6 zero bytes.  Z = table | parity (2448 bytes); code word r (0..11) is
// Z[r + 12 c], c = 0..203, byte c the coefficient of x^(203 - c).  Field, generator roots (alpha^0..alpha^15) and decoder: rs_code.hpp.
constexpr int kPkCell = 24;
constexpr int kPkDataCells = 94, kPkFecCells = 9, kPkFrameCells = 103;
constexpr int kPkTable = kPkDataCells * kPkCell;         // 2256
constexpr int kPkRows = 12;
constexpr int kPkN = 204, kPkK = 188, kPkRoots = 16, kPkT = 8;
constexpr int kPkFecPayload = 22;
constexpr int kPkFecAddress = 1022;
constexpr int kPkCarry = 102;                            // cells a lane keeps between pushes at most
constexpr int kPkHitHeaders = 5;                         // a synced frame is a hit with at least this many of its 9 FEC headers
constexpr int kPkMissLimit = 3;                          // the K-th consecutive miss loses sync (dabplus.hpp: kSyncFailLimit)
constexpr int kPkNoCounter = 15;

// the FEC counter (0..8) of a cell whose first two bytes are an FEC cell's header (length code 00, counter, address 1022), else kPkNoCounter
DABHIP_PK_HD inline int fec_counter(uint8_t b0, uint8_t b1)
{
  const int cnt = (b0 >> 2) & 15;
  return ((b0 >> 6) == 0 && (b0 & 3) == 3 && b1 == 0xfe && cnt < kPkFecCells) ? cnt : kPkNoCounter;
}

// where byte c of code word r lies in the 103 cells of an FEC frame
DABHIP_PK_HD inline int fec_byte_offset(int r, int c)
{
  if (c < kPkK) return kPkRows * c + r;
  const int i = kPkRows * (c - kPkK) + r;
  return (kPkDataCells + i / kPkFecPayload) * kPkCell + 2 + i % kPkFecPayload;
}

// state of one (stream, sub-channel), carried from push to push
struct PacketSync {
  int32_t synced;
  int32_t misses;                           // consecutive missed frames
  int32_t stl;                              // STL of the unbroken stream, 0: none
  int32_t ncar;                             // cells in the carry buffer: the stream's unconsumed cells
  int32_t good;                             // synced: FEC cells of the frame in progress that carried their own header
  int32_t runlen;                           // unsynced: FEC headers 0 .. runlen - 1 seen in the last runlen cells
  int64_t next_cell;                        // cells received since creation
};
static_assert(sizeof(PacketSync) == 32, "PacketSync layout");


// ---- the sync rule, one cell at a time ------------------------------------------------------------
// Positions are the lane's virtual cell numbers of this push: the carried cells first, then the new ones.  lo is the first cell no unit has
// consumed.  feed() takes cell u (its FEC counter h); on a unit it calls emit(first cell, flags).  It returns true when the third miss lost
// sync: the caller then feeds cells lo + 1 .. u again (as an unsynced lane), which cannot lose sync a second time.
struct PacketWalkState {
  PacketSync st;
  int32_t lo;
  int64_t skipped, frames, misses, losses;
};

template <class Emit>
DABHIP_PK_HD inline bool packet_feed(PacketWalkState& w, int32_t u, int h, Emit&& emit)
{
  PacketSync& st = w.st;
  if (st.synced) {
    const int ph = u - w.lo;
    if (ph >= kPkDataCells && h == ph - kPkDataCells) ++st.good;
    if (ph < kPkFrameCells - 1) return false;
    const bool hit = st.good >= kPkHitHeaders;
    st.good = 0;
    if (hit) {
      st.misses = 0;
      emit(w.lo, static_cast<int>(DABHIP_PACKET_FROM_FEC));
      ++w.frames;
    } else {
      if (++st.misses >= kPkMissLimit) {
        st.synced = 0;
        st.misses = 0;
        st.runlen = 0;
        ++w.losses;
        return true;
      }
      emit(w.lo, static_cast<int>(DABHIP_PACKET_FROM_MISS));
      ++w.frames;
      ++w.misses;
    }
    w.lo = u + 1;
    return false;
  }
  st.runlen = h == st.runlen ? st.runlen + 1 : (h == 0 ? 1 : 0);
  if (st.runlen < kPkFecCells) return false;
  const int32_t k = u - (kPkFecCells - 1);
  if (k - kPkDataCells >= w.lo) {
    w.skipped += k - kPkDataCells - w.lo;
    emit(k - kPkDataCells, static_cast<int>(DABHIP_PACKET_FROM_FEC));
    ++w.frames;
  } else {
    w.skipped += u + 1 - w.lo;
  }
  w.lo = u + 1;
  st.synced = 1;
  st.misses = 0;
  st.good = 0;
  st.runlen = 0;
  return false;
}

// a break of the stream at virtual cell n (the next to come): everything unconsumed is dropped
DABHIP_PK_HD inline void packet_break(PacketWalkState& w, int32_t n)
{
  w.skipped += n - w.lo;
  if (w.st.synced) ++w.losses;
  w.st.synced = w.st.misses = w.st.good = w.st.runlen = 0;
  w.st.stl = 0;
  w.lo = n;
}

// the end of a push with n cells: an unsynced lane lets go of the cells no later run can reach (a run found later starts at n - 8 or after)
DABHIP_PK_HD inline void packet_push_end(PacketWalkState& w, int32_t n)
{
  if (!w.st.synced && n - w.lo > kPkCarry) {
    w.skipped += n - kPkCarry - w.lo;
    w.lo = n - kPkCarry;
  }
  w.st.ncar = n - w.lo;
}

}  // namespace dabhip
