// k_ingest.hip — the ingest stage's kernels: cu8 / cs8 / cs16 / cf32 IQ at Fin -> the canonical cu8 at 2.048 Msps (the arithmetic: include/dabhip.h,
// "ingest stage"; the host rule: ingest_plan.hpp).  Integer throughout, so the bytes are those of tests/ingest_model.py whatever the launch shape.
//
// ingest_resample_kernel: one workgroup of 256 threads per kTilesPerGroup consecutive tiles of kIngestTile outputs of one stream (grid.y = stream).
//   LDS: the tap table (L rows of T/2 + 1 words: T/2 pairs of int16 taps in REVERSED order, one word of padding so that the row stride is odd), loaded
//   once per workgroup, and per tile the input samples it reaches, converted to int16 and stored as pairs: word 2w = (I[2w], I[2w+1]), word 2w+1 the same
//   of Q, tile start even.  An output reads T/2 such double words (ds_read_b64), shifts each rail by 16 bits where its first sample is odd
//   (v_alignbit_b32) and feeds v_dot2_i32_i16 with the tap pair: two multiply-accumulates per rail and instruction.  The 8-bit formats keep
//   x / 256 in LDS (cu8's (255 - 127) 256 = 32768 is no int16) and scale the sum by 256 afterwards: the same integer.
//   Positions: the tile's first output, its floor(m M / L) and its phase are 64-bit and per tile; a sample's are 32-bit offsets from them.
// ingest_bypass_kernel: L/M = 1/1, conversion and requantisation only.
// ingest_energy_kernel: sum(I^2 + Q^2) of a stream's samples [0, W) as an exact 64-bit integer, one workgroup per stream whose gain window closes.
// ingest_keep_kernel: the samples the next push needs, into the other carry buffer.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ingest.hpp"
#include "ingest_plan.hpp"

namespace dabhip {
namespace {

typedef short __attribute__((ext_vector_type(2))) vshort2;
constexpr int kThreads = 256;
constexpr int kTilesPerGroup = 8;

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

// sample n of the stream (absolute position), zero outside [carry_from, end)
template <int F>
__device__ __forceinline__ int2 fetch(const IngestDesc& d, int64_t n)
{
  typedef typename Sample<F>::type S;
  if (n < d.carry_from || n >= d.end) return int2{0, 0};
  if (n < d.new_from) return convert<F>(static_cast<const S*>(d.carry)[n - d.carry_from]);
  return convert<F>(static_cast<const S*>(d.src)[n - d.new_from]);
}

__device__ __forceinline__ unsigned requantise(int v, uint32_t gain)
{
  const long long t = static_cast<long long>(v) * static_cast<long long>(gain) + 32768;
  const int o = 127 + static_cast<int>(t >> 16);
  return static_cast<unsigned>(o < 0 ? 0 : o > 255 ? 255 : o);
}

template <int F>
__global__ __launch_bounds__(kThreads) void ingest_resample_kernel(const IngestDesc* __restrict__ descs, const uint32_t* __restrict__ table, int L, int M, int T,
                                                                  int table_words, int span_words)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const IngestDesc d = descs[blockIdx.y];
  const int tile_first = blockIdx.x * kTilesPerGroup;
  if (static_cast<int64_t>(tile_first) * kIngestTile >= d.nout) return;
  uint32_t* tab = lds;
  uint32_t* xw = lds + table_words;                              // table_words is even: 8-byte aligned
  short* xs = reinterpret_cast<short*>(xw);
  for (int i = threadIdx.x; i < table_words; i += kThreads) tab[i] = table[i];
  const int row = T / 2 + 1, half = T / 2;
  for (int t = 0; t < kTilesPerGroup; ++t) {
    const int64_t o0 = static_cast<int64_t>(tile_first + t) * kIngestTile;      // within this push
    if (o0 >= d.nout) break;
    const int cnt = static_cast<int>(d.nout - o0 < kIngestTile ? d.nout - o0 : kIngestTile);
    // 64-bit, once per tile: m0 M = n0 L + p0
    const unsigned long long mm = static_cast<unsigned long long>(d.first_out + o0) * static_cast<unsigned long long>(M);
    const int64_t n0 = static_cast<int64_t>(mm / static_cast<unsigned>(L));
    const unsigned p0 = static_cast<unsigned>(mm % static_cast<unsigned>(L));
    const int64_t start0 = n0 - half + 1;                        // first input sample of the tile's first output
    const int e = static_cast<int>(start0 & 1);
    const int64_t tile0 = start0 - e;                            // even
    __syncthreads();                                             // the tile before is done with xw (and the table is there)
    for (int i = threadIdx.x; i < 2 * span_words; i += kThreads) {
      const int2 v = fetch<F>(d, tile0 + i);
      const int at = (i >> 1) * 4 + (i & 1);
      xs[at] = static_cast<short>(v.x);
      xs[at + 2] = static_cast<short>(v.y);
    }
    __syncthreads();
    const uint2* xp = reinterpret_cast<const uint2*>(xw);
#pragma unroll
    for (int r = 0; r < kIngestTile / kThreads; ++r) {
      const int o = threadIdx.x + r * kThreads;
      if (o >= cnt) break;
      const unsigned q = p0 + static_cast<unsigned>(o) * static_cast<unsigned>(M);
      const unsigned dn = q / static_cast<unsigned>(L), p = q - dn * static_cast<unsigned>(L);
      const int s = e + static_cast<int>(dn);
      const unsigned sh = (s & 1) * 16u;
      const uint2* x = xp + (s >> 1);
      const uint32_t* tp = tab + p * row;
      uint2 lo = x[0];
      int acc_i = 0, acc_q = 0;
      for (int j = 0; j < half; ++j) {
        const uint2 hi = x[j + 1];
        const uint32_t tw = tp[j];
        const uint32_t ai = __builtin_amdgcn_alignbit(hi.x, lo.x, sh), aq = __builtin_amdgcn_alignbit(hi.y, lo.y, sh);
        acc_i = __builtin_amdgcn_sdot2(__builtin_bit_cast(vshort2, ai), __builtin_bit_cast(vshort2, tw), acc_i, false);
        acc_q = __builtin_amdgcn_sdot2(__builtin_bit_cast(vshort2, aq), __builtin_bit_cast(vshort2, tw), acc_q, false);
        lo = hi;
      }
      const int vi = (acc_i * (1 << post_shift<F>()) + 8192) >> 14, vq = (acc_q * (1 << post_shift<F>()) + 8192) >> 14;
      const unsigned pair = requantise(vi, d.gain) | requantise(vq, d.gain) << 8;
      reinterpret_cast<unsigned short*>(d.out)[o0 + o] = static_cast<unsigned short>(pair);
    }
  }
}

template <int F>
__global__ __launch_bounds__(kThreads) void ingest_bypass_kernel(const IngestDesc* __restrict__ descs)
{
  const IngestDesc d = descs[blockIdx.y];
  const int64_t o = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (o >= d.nout) return;
  const int2 v = fetch<F>(d, d.first_out + o);
  const unsigned pair = requantise(v.x * (1 << post_shift<F>()), d.gain) | requantise(v.y * (1 << post_shift<F>()), d.gain) << 8;
  reinterpret_cast<unsigned short*>(d.out)[o] = static_cast<unsigned short>(pair);
}

template <int F>
__global__ __launch_bounds__(kThreads) void ingest_energy_kernel(const IngestDesc* __restrict__ descs, unsigned long long* __restrict__ energy)
{
  __shared__ unsigned long long part[kThreads];
  const IngestDesc d = descs[blockIdx.x];
  if (d.energy_slot < 0) return;
  unsigned long long sum = 0;
  for (int64_t n = threadIdx.x; n < kIngestGainWindow; n += kThreads) {
    const int2 v = fetch<F>(d, n);
    const long long i = static_cast<long long>(v.x) * (1 << post_shift<F>()), q = static_cast<long long>(v.y) * (1 << post_shift<F>());
    sum += static_cast<unsigned long long>(i * i + q * q);
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) energy[d.energy_slot] = part[0];
}

template <int F>
__global__ __launch_bounds__(kThreads) void ingest_keep_kernel(const IngestDesc* __restrict__ descs)
{
  typedef typename Sample<F>::type S;
  const IngestDesc d = descs[blockIdx.y];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x, n = d.keep_from + i;
  if (n >= d.end) return;
  static_cast<S*>(d.keep)[i] = n < d.new_from ? static_cast<const S*>(d.carry)[n - d.carry_from] : static_cast<const S*>(d.src)[n - d.new_from];
}

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

hipError_t launch_ingest_resample(int format, const IngestDesc* descs, int nstreams, int max_nout, const uint32_t* table, int L, int M, int T, hipStream_t stream)
{
  if (nstreams <= 0 || nstreams > 65535 || max_nout <= 0) return nstreams > 65535 ? hipErrorInvalidValue : hipSuccess;
  if (T == 0) {
    const dim3 grid(static_cast<unsigned>((max_nout + kThreads - 1) / kThreads), static_cast<unsigned>(nstreams));
    return by_format(format, [&](auto f) { hipLaunchKernelGGL(ingest_bypass_kernel<decltype(f)::value>, grid, dim3(kThreads), 0, stream, descs); });
  }
  IngestRatio r;
  r.L = L; r.M = M; r.T = T;
  const int table_words = static_cast<int>((r.lds_table_bytes() / 4 + 1) & ~size_t(1));
  const int span_words = r.tile_span() / 2 + 2;                  // per rail
  const size_t lds_bytes = static_cast<size_t>(table_words) * 4 + static_cast<size_t>(span_words) * 8;
  const int tiles = (max_nout + kIngestTile - 1) / kIngestTile;
  const dim3 grid(static_cast<unsigned>((tiles + kTilesPerGroup - 1) / kTilesPerGroup), static_cast<unsigned>(nstreams));
  return by_format(format, [&](auto f) {
    auto* k = ingest_resample_kernel<decltype(f)::value>;
    if (lds_bytes > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)) != hipSuccess) return;
    hipLaunchKernelGGL(k, grid, dim3(kThreads), lds_bytes, stream, descs, table, L, M, T, table_words, span_words);
  });
}

hipError_t launch_ingest_energy(int format, const IngestDesc* descs, int nstreams, unsigned long long* energy, hipStream_t stream)
{
  if (nstreams <= 0) return hipSuccess;
  return by_format(format, [&](auto f) { hipLaunchKernelGGL(ingest_energy_kernel<decltype(f)::value>, dim3(static_cast<unsigned>(nstreams)), dim3(kThreads), 0, stream, descs, energy); });
}

hipError_t launch_ingest_keep(int format, const IngestDesc* descs, int nstreams, int64_t max_keep, hipStream_t stream)
{
  if (nstreams <= 0 || nstreams > 65535 || max_keep <= 0) return nstreams > 65535 ? hipErrorInvalidValue : hipSuccess;
  const dim3 grid(static_cast<unsigned>((max_keep + kThreads - 1) / kThreads), static_cast<unsigned>(nstreams));
  return by_format(format, [&](auto f) { hipLaunchKernelGGL(ingest_keep_kernel<decltype(f)::value>, grid, dim3(kThreads), 0, stream, descs); });
}

}  // namespace dabhip
