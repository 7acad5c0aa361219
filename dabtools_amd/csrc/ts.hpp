// ts.hpp — MPEG-2 TS sub-channels (ETSI TS 102 427): the device-side types of the kernels (k_ts.hip), shared with the host object (ts.cpp).
// The sizes, the sync rule and the position map are in ts_sync.hpp (free of HIP); dabhip.h has the rules in words; the plain-numpy
// restatement of all of it is tests/ts_model.py.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dabhip.h"
#include "packet.hpp"
#include "ts_sync.hpp"

namespace dabhip {

// where one requested sub-channel sits in one new ETI frame of the push: [stream][frame][sub]
struct TsLoc {
  const uint8_t* ptr;                       // first payload byte; null: absent, STL 0, or past the frame (locate)
  int32_t stl;
  int32_t byte0;                            // the lane's virtual position of its first byte (layout)
  int32_t seg;                              // breaks of the lane's stream up to and including the one in front of this frame (layout)
  int32_t pad;
};
static_assert(sizeof(TsLoc) == 24, "TsLoc layout");

// a unit (one code word) in its lane's slot (sync) and in the push's list (jobs): its slot's first byte in the lane's virtual positions
struct TsSlot {
  int32_t u0;
  int32_t flags;                            // DABHIP_TS_FROM_MISS
};
struct TsUnit {
  int32_t lane, u0;
  int32_t flags, pad;
  int64_t pos;                              // of its slot's first byte, since creation
};
static_assert(sizeof(TsSlot) == 8 && sizeof(TsUnit) == 24, "ts unit layout");

// what the layout pass leaves per lane for the kernels behind it
struct TsLane {
  int32_t nv;                               // virtual positions of this push: carried bytes + new bytes
  int32_t ncar;                             // carried bytes coming in
  int32_t flag0;                            // its first word in the run-flag buffer (64 positions a word)
  int32_t lo;                               // sync: first unconsumed position at the push's end; nv - lo bytes carry out
};
static_assert(sizeof(TsLane) == 16, "TsLane layout");

// The word buffer: words in groups of 64; in a group, four bytes of a word lie together and the 64 words side by side, so that the syndrome
// kernel's 64 lanes read 256 contiguous bytes per load: byte k of word w at ((w / 64) 51 + k / 4) 256 + (w % 64) 4 + k % 4.
DABHIP_TS_HD inline int64_t ts_word_byte(int64_t w, int k) { return ((w >> 6) * (kTsSlot / 4) + (k >> 2)) * 256 + (w & 63) * 4 + (k & 3); }
DABHIP_TS_HD inline int64_t ts_word_buffer_bytes(int64_t nwords) { return ((nwords + 63) >> 6) * 64 * kTsSlot; }

enum TsCounter : int { kTsCntPackets, kTsCntFromMiss, kTsCntSyncLosses, kTsCntSkipped, kTsCntRsCorrected, kTsCntRsFailed, kTsCntBadSync, kTsCntNull, kTsCntN = 8 };

// totals[]: the units of the push, the flag words handed out, "the flag buffer is too small" (layout), "a lane passed its slots" (sync)
enum TsTotal : int { kTsTotUnits, kTsTotFlagWords, kTsTotOverflow, kTsTotSlotOverflow, kTsTotN = 4 };

constexpr int kTsSyncWaves = 4;                          // lanes (waves) per workgroup of the layout and sync kernels

}  // namespace dabhip
