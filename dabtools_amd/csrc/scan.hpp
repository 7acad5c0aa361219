// scan.hpp — what scan.cpp (the block scan's host object) and k_scan.hip (its kernels) share.  The arithmetic: include/dabhip.h, "block scan"; the
// host rule: scan_blocks.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dabhip {

constexpr int kScanGroup = 8;      // G: segments of a stream one workgroup transforms and sums before it adds to the stream's spectrum

// One stream of one push.  Its samples live in two places, as the ingest stage's: [carry_from, new_from) in `carry`, [new_from, end) in `src`.
struct ScanDesc {
  const void* carry;
  const void* src;
  void* keep;                      // the carry of the next push: samples [keep_from, end)
  unsigned long long* power;       // the stream's P: 4096 bins in transform order
  int64_t carry_from, new_from, end;
  int64_t first_seg;               // this push completes segments [first_seg, first_seg + nseg): samples [4096 seg, 4096 seg + 4096)
  int64_t keep_from;
  int32_t nseg;
  int32_t pad;
};

// nco: 4096 words (cos | sin << 16, int16 each), as the tuned mode's kernels take it.  Adds the power of every descriptor's segments to its P.
hipError_t launch_scan_transform(int format, const ScanDesc* descs, int nstreams, int64_t max_nseg, const uint32_t* nco, hipStream_t stream);
hipError_t launch_scan_keep(int format, const ScanDesc* descs, int nstreams, int64_t max_keep, hipStream_t stream);

}  // namespace dabhip
