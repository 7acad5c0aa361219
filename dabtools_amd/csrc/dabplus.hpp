// dabplus.hpp — DAB+ audio superframes (ETSI TS 102 563): the sizes, the audio-superframe header rules and the fire code, shared by the
// synthetic modulator (synth.cpp), the host object (dabplus.cpp) and the kernels (k_dabplus.hip), plus the device-side types of those kernels.
// The field and the decoder of the RS(120,110) code are rs_code.hpp's.  The plain-numpy restatement of all of it is tests/dabplus_model.py.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dabhip.h"
#include "eti_push.hpp"

namespace dabhip {

// A sub-channel of 8 s kbit/s carries 24 s bytes per logical frame; 5 frames form a superframe of 120 s bytes: 110 s audio bytes, then 10 s RS
// parity bytes.  Codeword j (0 <= j < s) is superframe bytes j + k s, k = 0..119 (the "virtual interleaving"); byte k is the coefficient of
// x^(119 - k), and the generator has the roots alpha^0..alpha^9 (rs_code.hpp).
constexpr int kRsN = 120, kRsK = 110, kRsRoots = 10, kRsT = 5;
constexpr int kSfFrames = 5;
constexpr int kFctMod = 250;
constexpr int kMaxAus = 6;
constexpr int kMaxS = 72;                   // 576 kbit/s, the largest sub-channel a CIF holds with room to spare
// Superframe sync (dabhip.h: dabhip_dabplus_push): sync is lost at the K-th consecutive candidate whose raw fire code fails.
constexpr int kSyncFailLimit = 3;

// (dac_rate, sbr_flag) -> number of AUs and the start of AU 0 (the header's length: 3 bytes + 12 bits per further AU, padded to a byte)
__host__ __device__ inline void au_layout(int dac_rate, int sbr_flag, int* num_aus, int* start0)
{
  const int n = dac_rate ? (sbr_flag ? 3 : 6) : (sbr_flag ? 2 : 4);
  *num_aus = n;
  *start0 = 3 + (12 * (n - 1) + 7) / 8;
}

// au_start[i] (i >= 1), the 12-bit field at bit 24 + 12 (i - 1) of the superframe
__host__ __device__ inline int au_start_field(const uint8_t* sf, int i)
{
  const int bit = 24 + 12 * (i - 1);
  const int v = (sf[bit >> 3] << 8) | sf[(bit >> 3) + 1];
  return (bit & 7) ? (v & 0xfff) : (v >> 4);
}

// Fire code over superframe bytes 2..10: generator x^16+x^14+x^13+x^12+x^11+x^5+x^3+x^2+x+1 (0x782F), initial value 0, no inversion.
// It is good when it equals bytes 0..1 (most significant byte first).
__host__ __device__ inline uint16_t fire_code(const uint8_t* b2)
{
  uint32_t c = 0;
  for (int i = 0; i < 9; ++i) {
    c ^= static_cast<uint32_t>(b2[i]) << 8;
    for (int k = 0; k < 8; ++k) c = (c & 0x8000u) ? ((c << 1) ^ 0x782Fu) & 0xffffu : (c << 1) & 0xffffu;
  }
  return static_cast<uint16_t>(c);
}

// ---- device-side records of k_dabplus.hip ----------------------------------------------------------------------------------------------------
// where one requested sub-channel sits in one ETI frame (locate kernel): [stream][virtual frame][sub]
struct DabPlusLoc {
  const uint8_t* ptr;                       // first payload byte; null: absent, or not a DAB+ sub-channel (STL 0, not a multiple of 3, > 216, past the frame)
  int32_t stl;
  uint8_t fct;
  uint8_t raw_fire;                         // fire code of the first 11 payload bytes good (as received)
  uint8_t pad[2];
};
static_assert(sizeof(DabPlusLoc) == 16, "DabPlusLoc layout");

// sync state of one (stream, sub-channel), carried from push to push
struct DabPlusSync {
  int32_t synced;
  int32_t fails;                            // consecutive candidates with a failing raw fire code
  int32_t stl;                              // the locked STL
  int32_t last_fct;                         // FCT of the last frame of the last superframe
  int32_t back;                             // frames at the end of the last push not consumed yet (<= 4): the next walk starts there
  int32_t pad[3];
};

// one superframe of this push: its frames are virtual frames v0 .. v0 + 4 of its stream
struct DabPlusJob {
  int32_t stream, sub, v0, s;
  int64_t data_base;                        // first of its 110 s corrected bytes in the data buffer
  int32_t cw_base;                          // its first codeword in the push's codeword numbering
  int32_t slot;                             // its candidate slot (sync kernel output)
};

// the superframe sync kernel's candidate: virtual frame of the first frame, s, and its first codeword among its lane's
struct DabPlusCand {
  int32_t v0, s, cw_off;
};

// the frames of one push: stream s's virtual frames are its ncarry[s] carried frames (carry + (4 s + v) 6144), then its nnew[s] new ones
// (frames + (base[s] + v - ncarry[s]) 6144).  An EtiFrames (eti_push.hpp) with the carry beside it; the fields keep the order the kernels'
// arguments were compiled with
struct DabPlusFrames {
  const uint8_t* frames;
  const uint8_t* carry;
  const int64_t* base;
  const int* nnew;
  const int* ncarry;
  int aligned;                              // frames 16-byte aligned: the carry copy goes by 16 bytes
};

enum DabPlusCounter : int { kCntSuperframes, kCntFireFails, kCntRsCorrected, kCntRsFailed, kCntAus, kCntAuCrcFails, kCntSyncLosses, kCntN = 8 };

}  // namespace dabhip
