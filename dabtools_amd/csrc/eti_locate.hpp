// eti_locate.hpp — where the requested sub-channels sit in one ETI(NI) frame: the walk over the frame's stream characterisation (STC) that the
// locate kernels of k_dabplus.hip, k_packet.hip and k_ts.hip share.  Each kernel clears its own records first and passes what it stores, and what
// it accepts, as the callable.  Free of the HIP runtime: tests/host_sanitize/eti_push_units.cpp, a plain g++ program, runs this text.
#pragma once

#include <cstdint>

#include "../../include/dabhip.h"

#ifdef __HIPCC__
#define DABHIP_ETI_HD __host__ __device__ __forceinline__
#else
#define DABHIP_ETI_HD inline
#endif

namespace dabhip {

// f: the frame's 6144 bytes.  take(q, stl, fits, p) once for every requested SubChId subch[q] (nsub <= 64) that the STC lists: its STL, whether
// its 8 stl payload bytes end inside the frame, and where they begin.  Entries behind one that runs past the frame are not reached.
template <class Take>
DABHIP_ETI_HD void eti_stc_walk(const uint8_t* f, const int32_t* subch, int nsub, Take take)
{
  const int ficf = f[5] >> 7, nst = f[5] & 0x7f;
  int off = 12 + 4 * nst + 96 * ficf;
  uint64_t seen = 0;                                 // a SubChId listed twice in the STC: its first entry counts
  for (int i = 0; i < nst; ++i) {
    const int scid = f[8 + 4 * i] >> 2;
    const int stl = ((f[8 + 4 * i + 2] & 3) << 8) | f[8 + 4 * i + 3];
    const bool fits = off + 8 * stl <= DABHIP_ETI_BYTES;
    for (int q = 0; q < nsub; ++q) {
      if (subch[q] != scid || (seen >> q & 1)) continue;
      seen |= uint64_t{1} << q;
      take(q, stl, fits, f + off);
    }
    off += 8 * stl;
    if (off > DABHIP_ETI_BYTES) break;
  }
}

}  // namespace dabhip
