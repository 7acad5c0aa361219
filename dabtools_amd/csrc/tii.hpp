// tii.hpp — what tii.cpp (the engine's hook and the stage entry) and k_tii.hip (the kernel) share.  The arithmetic: include/dabhip.h, "TII"; the host
// rule: tii_detect.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.hpp"
#include "tii_detect.hpp"

namespace dabhip {

constexpr int kTiiRow = kTiiSums + 8;      // words of a row of sums: T[192], the frames counted at [192], padding to 64 bytes

// One launch: a workgroup per descriptor.  Descriptor d belongs to stream d / max_calls of iq.
//   w0 == nullptr (a decode): the descriptor counts by the header's rule, window and step come from its fields, and it adds to row d / max_calls;
//   w0 != nullptr (the stage entry): every descriptor counts with window start w0[d] (0 .. 608, checked by the host) and step[d], and adds to row d.
struct TiiArgs {
  const uint8_t* const* iq;
  const CallDesc* descs;
  int max_calls;
  const int32_t* w0;
  const uint32_t* step;
  unsigned long long* sums;      // rows of kTiiRow words
};
// nco: 4096 words (cos | sin << 16, int16 each), as the block scan's kernel takes it
hipError_t launch_tii(const TiiArgs& a, size_t ndesc, const uint32_t* nco, hipStream_t stream);

}  // namespace dabhip
