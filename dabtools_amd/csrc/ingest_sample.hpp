// ingest_sample.hpp — step 1 of the ingest stage (include/dabhip.h): a sample of one of the four formats to the 16-bit domain.  Shared by the kernels
// that read captures where the caller left them, k_ingest.hip and k_scan.hip, with the launch wrappers' dispatch on the format.  Device code, but for that.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

namespace dabhip {
namespace {

template <int F> struct Sample;
template <> struct Sample<0> { typedef uchar2 type; };
template <> struct Sample<1> { typedef char2 type; };
template <> struct Sample<2> { typedef short2 type; };
template <> struct Sample<3> { typedef float2 type; };

__device__ __forceinline__ int cf32_to_16(float f)
{
  float v = f * 32768.0f;
  v = (v == v) ? v : 0.0f;                                       // NaN -> 0
  v = v < -32768.0f ? -32768.0f : v > 32767.0f ? 32767.0f : v;
  return static_cast<int>(rintf(v));                             // ties to even
}
// what LDS holds of a sample: the 16-bit-domain value, or for the 8-bit formats that value / 256
template <int F>
__device__ __forceinline__ int2 convert(typename Sample<F>::type s)
{
  if constexpr (F == 0) return int2{static_cast<int>(s.x) - 127, static_cast<int>(s.y) - 127};
  else if constexpr (F == 3) return int2{cf32_to_16(s.x), cf32_to_16(s.y)};
  else return int2{static_cast<int>(s.x), static_cast<int>(s.y)};
}
template <int F> constexpr int post_shift() { return F <= 1 ? 8 : 0; }

// fn(std::integral_constant<int, format>()) launches; returns what the launch left
template <class Fn>
hipError_t by_format(int format, Fn fn)
{
  switch (format) {
    case 0: fn(std::integral_constant<int, 0>()); break;
    case 1: fn(std::integral_constant<int, 1>()); break;
    case 2: fn(std::integral_constant<int, 2>()); break;
    case 3: fn(std::integral_constant<int, 3>()); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace
}  // namespace dabhip
