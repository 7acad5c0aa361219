// ts_sync.hpp — the sizes of the MPEG-2 TS stage (ETSI TS 102 427), its sync rule 64 slots at a time, the map from a lane's byte positions to
// the frames of a push and the bound on the units a push can give, free of HIP: the kernels (k_ts.hip, through ts.hpp), the host object
// (ts.cpp) and tests/host_sanitize/ts_units.cpp run this text.  dabhip.h (dabhip_ts) has the rules in words.
#pragma once

#include <cstdint>

#include "../../include/dabhip.h"

#ifdef __HIPCC__
#define DABHIP_TS_HD __host__ __device__
#else
#define DABHIP_TS_HD
#endif

namespace dabhip {

// A code word is 204 bytes, 188 TS bytes and 16 parity bytes (the code is packet_sync.hpp's, its decoder rs_code.hpp's).  Byte k of the word whose slot starts at stream
// position P lies at P + k + 204 (k mod 12): the convolutional interleaver (I = 12, M = 17) in closed form.  So a word needs the
// kTsLook = 203 + 204 * 11 + 1 bytes from P on, and a lane carries kTsLook - 1 bytes at most from push to push.
constexpr int kTsSlot = 204, kTsData = 188;
constexpr int kTsBranches = 12;
constexpr int kTsRun = 5;                                // a run: 0x47 at p + 204 i, i = 0..4
constexpr int kTsRunSpan = kTsSlot * (kTsRun - 1);       // 816: the run at p is decided once byte p + 816 is on hand
constexpr int kTsLook = 2448;
constexpr int kTsCarry = kTsLook - 1;                    // 2447
constexpr int kTsCarryStride = kTsLook;                  // bytes per lane in a carry buffer
constexpr int kTsMissLimit = 3;
constexpr int kTsSyncByte = 0x47;
constexpr int kTsNullPid = 0x1fff;
constexpr int kTsChunk = 64;                             // slots judged at a time: one ballot
constexpr int kTsFrameBytesMax = DABHIP_ETI_BYTES - 16;  // payload bytes of one sub-channel in one ETI frame at most (NST = 1: 12 header bytes + 4 of STC)
constexpr int kTsStlMax = kTsFrameBytesMax / 8;          // 766: the largest STL the locate rule accepts

// where byte k of the code word whose slot starts at P lies
DABHIP_TS_HD inline int64_t ts_byte_pos(int64_t P, int k) { return P + k + kTsSlot * (k % kTsBranches); }

// state of one (stream, sub-channel), carried from push to push
struct TsSync {
  int32_t synced;
  int32_t misses;                           // consecutive missed slots
  int32_t stl;                              // STL of the unbroken stream, 0: none
  int32_t ncar;                             // bytes in the carry buffer: the stream's unconsumed bytes
  int64_t next_pos;                         // bytes received since creation
  int64_t pad;
};
static_assert(sizeof(TsSync) == 32, "TsSync layout");

// ---- the synced rule, up to 64 slots at a time ----------------------------------------------------------------------------------------------
// Slots 0 .. nvalid - 1 (1 <= nvalid <= 64) all have their look-ahead; bit i of hits: slot i starts with 0x47.  misses_in (0 .. 2): the
// consecutive misses before slot 0.  Slot by slot the rule is: a hit clears the miss count and gives a packet; a miss adds 1, and the 3rd in a
// row loses sync at that slot, which gives no packet and ends the chunk; any other miss gives a packet flagged FROM_MISS.
struct TsChunkStep {
  int32_t npackets;                         // slots 0 .. npackets - 1 give packets
  int32_t lost;                             // sync is lost at slot npackets (< nvalid); the search resumes one byte after its start
  uint64_t from_miss;                       // bit i: packet i comes from a missed slot
  int32_t misses;                           // the miss count carried out (0 when lost)
};

DABHIP_TS_HD inline TsChunkStep ts_chunk_step(uint64_t hits, int nvalid, int misses_in)
{
  const uint64_t valid = nvalid >= 64 ? ~uint64_t{0} : ((uint64_t{1} << nvalid) - 1);
  const uint64_t h = hits & valid, m = ~hits & valid;
  // bit i of third: slot i is the 3rd miss in a row, the carried misses counted in
  uint64_t third = m & (m << 1) & (m << 2);
  if (misses_in >= 1 && (m & 3) == 3) third |= 2;
  if (misses_in >= 2 && (m & 1)) third |= 1;
  TsChunkStep r;
  if (third) {
    r.npackets = __builtin_ctzll(third);
    r.lost = 1;
    r.from_miss = m & ((uint64_t{1} << r.npackets) - 1);     // npackets <= 63 here
    r.misses = 0;
    return r;
  }
  r.npackets = nvalid;
  r.lost = 0;
  r.from_miss = m;
  if (!h) {
    r.misses = misses_in + nvalid;          // nothing but misses: 2 at most with the carried ones, or sync would be lost
  } else {
    r.misses = nvalid - 1 - (63 - __builtin_clzll(h));    // the misses above the last hit are the ones carried out (2 at most)
  }
  return r;
}

// ---- positions ------------------------------------------------------------------------------------------------------------------------------
// A lane's virtual positions in one push: its carried bytes 0 .. ncar - 1, then the payload of its new frames in order.  byte0(v) is the
// position of frame v's first byte; a frame that gives no bytes shares the byte0 of the frame after it (or the push's end).  The frame that
// holds position u >= ncar is therefore the LAST one with byte0 <= u.
template <class Byte0>
DABHIP_TS_HD inline int ts_frame_of(int nnew, int32_t u, Byte0&& byte0)
{
  int lo = 0, hi = nnew - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (byte0(mid) <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Slots decidable with `have` unconsumed bytes from the next slot on (each needs its kTsLook bytes; consecutive slots start 204 apart).
DABHIP_TS_HD inline int64_t ts_slots_ready(int64_t have) { return have < kTsLook ? 0 : (have - kTsLook) / kTsSlot + 1; }

// The units (packets) one lane can give in one push that brings nframes frames of STL stl on top of ncar carried bytes.  Units start at
// distinct positions at least 204 apart (a sync loss moves on by one byte and finds the next run no earlier than that), and each has its
// look-ahead on hand, so this is ts_slots_ready of all the bytes.
DABHIP_TS_HD inline int64_t ts_unit_bound(int ncar, int64_t nframes, int stl) { return ts_slots_ready(ncar + nframes * 8 * static_cast<int64_t>(stl)); }

// Unsynced with the search at q and `end` bytes on hand and no run found: the search waits at max(q, end - 816)
DABHIP_TS_HD inline int64_t ts_search_wait(int64_t q, int64_t end) { return q > end - kTsRunSpan ? q : end - kTsRunSpan; }

}  // namespace dabhip
