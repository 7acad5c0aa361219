// fixed_butterfly.hpp — the radix-2 butterfly of the fixed-point transforms (include/dabhip.h, "block scan" step 2; "TII" uses the same), shared by
// k_scan.hip and k_tii.hip: the two roundings of a butterfly are written once.  cs: an entry of the tuned mode's NCO table as the kernels hold it,
// cos | sin << 16, int16 each in Q14.  Both factors of every product fit 24 bits (the header's range argument).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dabhip {

// b e^(-j theta): (bI c + bQ s + 8192) >> 14, (bQ c - bI s + 8192) >> 14, arithmetic shifts
__device__ __forceinline__ int2 rotate_q14(int2 b, uint32_t cs)
{
  const int c = static_cast<short>(cs & 0xffffu), s = static_cast<short>(cs >> 16);
  return int2{(__mul24(b.x, c) + __mul24(b.y, s) + 8192) >> 14, (__mul24(b.y, c) - __mul24(b.x, s) + 8192) >> 14};
}
// a' = (a + t + 1) >> 1, b' = (a - t + 1) >> 1 per rail
__device__ __forceinline__ void halve(int2& a, int2& b, int ti, int tq)
{
  const int2 a0 = a;
  a = int2{(a0.x + ti + 1) >> 1, (a0.y + tq + 1) >> 1};
  b = int2{(a0.x - ti + 1) >> 1, (a0.y - tq + 1) >> 1};
}
__device__ __forceinline__ void butterfly(int2& a, int2& b, uint32_t cs)
{
  const int2 t = rotate_q14(b, cs);
  halve(a, b, t.x, t.y);
}

}  // namespace dabhip
