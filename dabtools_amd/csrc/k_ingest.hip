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
// The tuned mode (dabhip_ingest_create_tuned): one descriptor per OUTPUT stream, the channels of an input stream share its carry and src.
// ingest_tune_kernel: ingest_resample_kernel with the mixer where the tile is loaded -- a sample is read in the full 16-bit domain, turned by the NCO
//   entry of its absolute position (table: 4096 words of (cos, sin) in LDS behind the tile; every lane of a load looks up another entry, which LDS
//   serves at a few cycles per wave and the vector cache at one line per lane) and clamped to int16, once per input sample of the tile; the tap loop
//   is the same.  Its energy form computes v of outputs [0, W) of the channels whose window closes, 8 tiles per workgroup, and adds
//   sum(vI^2 + vQ^2) to the channel's slot with one 64-bit atomic add per wave (integer: the order does not matter).
// ingest_tune_bypass_kernel: Fin = 2,048,000: the mixer only, the NCO entry read through the cache (one lookup per output and no tile to share it).
#include <hip/hip_runtime.h>

#include "ingest.hpp"
#include "ingest_plan.hpp"
#include "ingest_sample.hpp"

namespace dabhip {
namespace {

typedef short __attribute__((ext_vector_type(2))) vshort2;
constexpr int kThreads = 256;
constexpr int kTilesPerGroup = 8;

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

// one output: T/2 double words of the tile from x on, against the phase's T/2 tap pairs
__device__ __forceinline__ void tap_loop(const uint2* x, const uint32_t* tp, int half, unsigned sh, int* acc_i, int* acc_q)
{
  uint2 lo = x[0];
  int ai = 0, aq = 0;
  for (int j = 0; j < half; ++j) {
    const uint2 hi = x[j + 1];
    const uint32_t tw = tp[j];
    const uint32_t xi = __builtin_amdgcn_alignbit(hi.x, lo.x, sh), xq = __builtin_amdgcn_alignbit(hi.y, lo.y, sh);
    ai = __builtin_amdgcn_sdot2(__builtin_bit_cast(vshort2, xi), __builtin_bit_cast(vshort2, tw), ai, false);
    aq = __builtin_amdgcn_sdot2(__builtin_bit_cast(vshort2, xq), __builtin_bit_cast(vshort2, tw), aq, false);
    lo = hi;
  }
  *acc_i = ai;
  *acc_q = aq;
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
      int acc_i = 0, acc_q = 0;
      tap_loop(x, tp, half, sh, &acc_i, &acc_q);
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

// ---- the tuned mode ---------------------------------------------------------------------------------------------------------------------
// y of the sample at absolute position n (include/dabhip.h, tuned mode, step 2): x e^(-j theta), theta = n step mod 2^32, clamped to int16
__device__ __forceinline__ int2 mix(int2 x, int64_t n, uint32_t step, const uint32_t* nco)
{
  const uint32_t theta = static_cast<uint32_t>(static_cast<uint64_t>(n)) * step;
  const uint32_t cs = nco[(theta + (1u << 19)) >> 20];            // the sum wraps: index 4096 is index 0
  const int c = static_cast<short>(cs & 0xffffu), s = static_cast<short>(cs >> 16);
  const int yi = (x.x * c + x.y * s + 8192) >> 14, yq = (x.y * c - x.x * s + 8192) >> 14;
  return int2{yi < -32768 ? -32768 : yi > 32767 ? 32767 : yi, yq < -32768 ? -32768 : yq > 32767 ? 32767 : yq};
}
template <int F>
__device__ __forceinline__ int2 fetch16(const IngestDesc& d, int64_t n)
{
  const int2 v = fetch<F>(d, n);
  return int2{v.x * (1 << post_shift<F>()), v.y * (1 << post_shift<F>())};
}
// a workgroup's sum into energy[slot]: every lane of every wave arrives here; one 64-bit atomic add per wave
__device__ __forceinline__ void add_energy(unsigned long long sum, unsigned long long* energy, int slot)
{
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(&energy[slot], sum);
}

// kEnergy: outputs [0, W) of the descriptors with an energy slot, their energy instead of their bytes
template <int F, bool kEnergy>
__global__ __launch_bounds__(kThreads) void ingest_tune_kernel(const IngestDesc* __restrict__ descs, const uint32_t* __restrict__ table, const uint32_t* __restrict__ nco_table,
                                                              unsigned long long* __restrict__ energy, int L, int M, int T, int table_words, int span_words)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const IngestDesc d = descs[blockIdx.y];
  if (kEnergy && d.energy_slot < 0) return;
  const int64_t first_out = kEnergy ? 0 : d.first_out, nout = kEnergy ? kIngestGainWindow : d.nout;
  const int tile_first = blockIdx.x * kTilesPerGroup;
  if (static_cast<int64_t>(tile_first) * kIngestTile >= nout) return;
  uint32_t* tab = lds;
  uint32_t* xw = lds + table_words;                              // table_words is even: 8-byte aligned
  uint32_t* nco = xw + 2 * span_words;
  short* xs = reinterpret_cast<short*>(xw);
  for (int i = threadIdx.x; i < table_words; i += kThreads) tab[i] = table[i];
  for (int i = threadIdx.x; i < kTuneNcoSize; i += kThreads) nco[i] = nco_table[i];
  const int row = T / 2 + 1, half = T / 2;
  unsigned long long sum = 0;
  for (int t = 0; t < kTilesPerGroup; ++t) {
    const int64_t o0 = static_cast<int64_t>(tile_first + t) * kIngestTile;
    if (o0 >= nout) break;
    const int cnt = static_cast<int>(nout - o0 < kIngestTile ? nout - o0 : kIngestTile);
    const unsigned long long mm = static_cast<unsigned long long>(first_out + o0) * static_cast<unsigned long long>(M);
    const int64_t n0 = static_cast<int64_t>(mm / static_cast<unsigned>(L));
    const unsigned p0 = static_cast<unsigned>(mm % static_cast<unsigned>(L));
    const int64_t start0 = n0 - half + 1;
    const int e = static_cast<int>(start0 & 1);
    const int64_t tile0 = start0 - e;
    __syncthreads();                                             // the tile before is done with xw (and both tables are there)
    for (int i = threadIdx.x; i < 2 * span_words; i += kThreads) {
      const int2 y = mix(fetch16<F>(d, tile0 + i), tile0 + i, d.step, nco);
      const int at = (i >> 1) * 4 + (i & 1);
      xs[at] = static_cast<short>(y.x);
      xs[at + 2] = static_cast<short>(y.y);
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
      int acc_i = 0, acc_q = 0;
      tap_loop(xp + (s >> 1), tab + p * row, half, (s & 1) * 16u, &acc_i, &acc_q);
      const int vi = (acc_i + 8192) >> 14, vq = (acc_q + 8192) >> 14;
      if constexpr (kEnergy) {
        sum += static_cast<unsigned long long>(static_cast<long long>(vi) * vi + static_cast<long long>(vq) * vq);
      } else {
        const unsigned pair = requantise(vi, d.gain) | requantise(vq, d.gain) << 8;
        reinterpret_cast<unsigned short*>(d.out)[o0 + o] = static_cast<unsigned short>(pair);
      }
    }
  }
  if constexpr (kEnergy) add_energy(sum, energy, d.energy_slot);
}

template <int F, bool kEnergy>
__global__ __launch_bounds__(kThreads) void ingest_tune_bypass_kernel(const IngestDesc* __restrict__ descs, const uint32_t* __restrict__ nco_table, unsigned long long* __restrict__ energy)
{
  const IngestDesc d = descs[blockIdx.y];
  if (kEnergy && d.energy_slot < 0) return;
  const int64_t first_out = kEnergy ? 0 : d.first_out, nout = kEnergy ? kIngestGainWindow : d.nout;
  const int64_t o = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (static_cast<int64_t>(blockIdx.x) * kThreads >= nout) return;                       // whole workgroups leave: add_energy synchronises
  const int2 v = o < nout ? mix(fetch16<F>(d, first_out + o), first_out + o, d.step, nco_table) : int2{0, 0};
  if constexpr (kEnergy) {
    add_energy(static_cast<unsigned long long>(static_cast<long long>(v.x) * v.x + static_cast<long long>(v.y) * v.y), energy, d.energy_slot);
  } else if (o < nout) {
    const unsigned pair = requantise(v.x, d.gain) | requantise(v.y, d.gain) << 8;
    reinterpret_cast<unsigned short*>(d.out)[o] = static_cast<unsigned short>(pair);
  }
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

// energy != nullptr: the energy form (outputs [0, W) of the descriptors with a slot; the slots are zero beforehand)
hipError_t launch_ingest_tune(int format, const IngestDesc* descs, int nouts, int max_nout, const uint32_t* table, const uint32_t* nco, unsigned long long* energy, int L, int M, int T,
                              hipStream_t stream)
{
  if (energy) max_nout = static_cast<int>(kIngestGainWindow);
  if (nouts <= 0 || nouts > 65535 || max_nout <= 0) return nouts > 65535 ? hipErrorInvalidValue : hipSuccess;
  if (T == 0) {
    const dim3 grid(static_cast<unsigned>((max_nout + kThreads - 1) / kThreads), static_cast<unsigned>(nouts));
    return by_format(format, [&](auto f) {
      if (energy) hipLaunchKernelGGL((ingest_tune_bypass_kernel<decltype(f)::value, true>), grid, dim3(kThreads), 0, stream, descs, nco, energy);
      else hipLaunchKernelGGL((ingest_tune_bypass_kernel<decltype(f)::value, false>), grid, dim3(kThreads), 0, stream, descs, nco, energy);
    });
  }
  IngestRatio r;
  r.L = L; r.M = M; r.T = T;
  const int table_words = static_cast<int>((r.lds_table_bytes() / 4 + 1) & ~size_t(1));
  const int span_words = r.tile_span() / 2 + 2;                  // per rail
  const size_t lds_bytes = ingest_tune_lds_bytes(r);             // table, tile, NCO table: the kernel's order
  if (lds_bytes > kTuneMaxLdsBytes) return hipErrorInvalidValue;
  const int tiles = (max_nout + kIngestTile - 1) / kIngestTile;
  const dim3 grid(static_cast<unsigned>((tiles + kTilesPerGroup - 1) / kTilesPerGroup), static_cast<unsigned>(nouts));
  return by_format(format, [&](auto f) {
    auto launch = [&](auto* k) {
      if (lds_bytes > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)) != hipSuccess) return;
      hipLaunchKernelGGL(k, grid, dim3(kThreads), lds_bytes, stream, descs, table, nco, energy, L, M, T, table_words, span_words);
    };
    if (energy) launch(ingest_tune_kernel<decltype(f)::value, true>);
    else launch(ingest_tune_kernel<decltype(f)::value, false>);
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
