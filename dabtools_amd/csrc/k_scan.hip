// k_scan.hip — the block scan's kernels: the fixed-point 4096-point transform of include/dabhip.h, "block scan", and the exact power sum.  Integer
// throughout and rounded only where the header says, so the spectrum is that of tests/scan_model.py whatever the launch shape.
//
// scan_transform_kernel: one workgroup of 256 threads per kScanGroup consecutive segments of one stream (grid.y = stream).  A thread holds 16 points
//   in registers and the 12 radix-2 stages are three passes of 4 stages each, with two exchanges through LDS between them:
//     pass 0 (h = 1 .. 8):      thread t holds the bit-reversed segment's indices 16 t + j -- samples bitrev4(j) 256 + bitrev8(t) of the segment, read where
//                               the caller (or the carry) left them and converted on the way;
//     pass 1 (h = 16 .. 128):   thread (hi, lo) = (t >> 4, t & 15) holds indices 256 hi + 16 j + lo;
//     pass 2 (h = 256 .. 2048): thread t holds indices 256 j + t, which are the bins it then owns.
//   A stage's butterflies pair the registers whose j differ in one bit, and a butterfly rounds exactly as the header's does (fixed_butterfly.hpp,
//   shared with k_tii.hip).  The two rails are two
//   LDS arrays of words, index i at i + (i >> 4): the stride of 17 spreads pass 0's writes (16 t + j) and pass 1's accesses over all banks.  The
//   twiddles are the tuned mode's NCO table, 16 KiB in LDS; pass 0's are known when the code is compiled (those of h = 1, 2 are 1 and -j: exact, no
//   product).  Both factors of every product fit 24 bits (the header's range proof): v_mul_i32_i24.
//   The workgroup sums XI^2 + XQ^2 of its segments in 64-bit registers and adds them to the stream's P with one 64-bit atomic add per bin.
// scan_keep_kernel: the unfinished segment's samples into the other carry buffer.
#include <hip/hip_runtime.h>

#include "fixed_butterfly.hpp"
#include "ingest_sample.hpp"
#include "scan.hpp"

namespace dabhip {
namespace {

constexpr int kThreads = 256;
constexpr int kSize = 4096;
constexpr int kRailWords = kSize + kSize / 16;

__device__ __forceinline__ int padded(int i) { return i + (i >> 4); }
constexpr int bitrev4(int j) { return (j & 1) << 3 | (j & 2) << 1 | (j & 4) >> 1 | (j & 8) >> 3; }

// sample n of the stream (absolute position) in the 16-bit domain
template <int F>
__device__ __forceinline__ int2 fetch16(const ScanDesc& d, int64_t n)
{
  typedef typename Sample<F>::type S;
  if (n < d.carry_from || n >= d.end) return int2{0, 0};
  const int2 v = n < d.new_from ? convert<F>(static_cast<const S*>(d.carry)[n - d.carry_from]) : convert<F>(static_cast<const S*>(d.src)[n - d.new_from]);
  return int2{v.x * (1 << post_shift<F>()), v.y * (1 << post_shift<F>())};
}


// four stages on the 16 registers of a thread: register j is index base + j 16^P, and low = base mod 16^P
template <int P>
__device__ __forceinline__ void pass(int2 (&v)[16], int low, const uint32_t* nco)
{
  constexpr int stride = 1 << (4 * P);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int h = stride << s, per = 2048 / h;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j & (1 << s)) continue;
      const int t = (low + (j & ((1 << s) - 1)) * stride) * per;
      int2& a = v[j];
      int2& b = v[j | (1 << s)];
      if (P == 0 && t == 0) halve(a, b, b.x, b.y);                // c = 16384, s = 0: (x 16384 + 8192) >> 14 = x
      else if (P == 0 && t == 1024) halve(a, b, b.y, -b.x);       // c = 0, s = 16384
      else butterfly(a, b, nco[t]);
    }
  }
}

template <int F>
__global__ __launch_bounds__(kThreads) void scan_transform_kernel(const ScanDesc* __restrict__ descs, const uint32_t* __restrict__ nco_table)
{
  __shared__ uint32_t nco[kSize];
  __shared__ int rail_i[kRailWords], rail_q[kRailWords];
  const ScanDesc d = descs[blockIdx.y];
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kScanGroup;
  if (g0 >= d.nseg) return;
  const int tid = threadIdx.x, hi = tid >> 4, lo = tid & 15;
  const int rev8 = static_cast<int>(__brev(static_cast<unsigned>(tid)) >> 24);
  for (int i = tid; i < kSize; i += kThreads) nco[i] = nco_table[i];
  const int count = static_cast<int>(d.nseg - g0 < kScanGroup ? d.nseg - g0 : kScanGroup);
  unsigned long long power[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) power[j] = 0;
  for (int g = 0; g < count; ++g) {
    const int64_t n0 = (d.first_seg + g0 + g) * kSize;
    int2 v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = fetch16<F>(d, n0 + bitrev4(j) * 256 + rev8);
    __syncthreads();                                             // the table is there, and the segment before is done with the rails
    pass<0>(v, 0, nco);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      rail_i[padded(16 * tid + j)] = v[j].x;
      rail_q[padded(16 * tid + j)] = v[j].y;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = int2{rail_i[padded(256 * hi + 16 * j + lo)], rail_q[padded(256 * hi + 16 * j + lo)]};
    pass<1>(v, lo, nco);
#pragma unroll
    for (int j = 0; j < 16; ++j) {                               // where this thread read them: nobody else touches these words in between
      rail_i[padded(256 * hi + 16 * j + lo)] = v[j].x;
      rail_q[padded(256 * hi + 16 * j + lo)] = v[j].y;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = int2{rail_i[padded(256 * j + tid)], rail_q[padded(256 * j + tid)]};
    pass<2>(v, tid, nco);
#pragma unroll
    for (int j = 0; j < 16; ++j) power[j] += static_cast<unsigned long long>(static_cast<long long>(v[j].x) * v[j].x + static_cast<long long>(v[j].y) * v[j].y);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) atomicAdd(&d.power[256 * j + tid], power[j]);      // integers: the order of the workgroups does not matter
}

template <int F>
__global__ __launch_bounds__(kThreads) void scan_keep_kernel(const ScanDesc* __restrict__ descs)
{
  typedef typename Sample<F>::type S;
  const ScanDesc d = descs[blockIdx.y];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x, n = d.keep_from + i;
  if (n >= d.end) return;
  static_cast<S*>(d.keep)[i] = n < d.new_from ? static_cast<const S*>(d.carry)[n - d.carry_from] : static_cast<const S*>(d.src)[n - d.new_from];
}

}  // namespace

hipError_t launch_scan_transform(int format, const ScanDesc* descs, int nstreams, int64_t max_nseg, const uint32_t* nco, hipStream_t stream)
{
  if (nstreams <= 0 || nstreams > 65535 || max_nseg <= 0 || max_nseg > 65536) return nstreams > 65535 || max_nseg > 65536 ? hipErrorInvalidValue : hipSuccess;
  const dim3 grid(static_cast<unsigned>((max_nseg + kScanGroup - 1) / kScanGroup), static_cast<unsigned>(nstreams));
  return by_format(format, [&](auto f) { hipLaunchKernelGGL(scan_transform_kernel<decltype(f)::value>, grid, dim3(kThreads), 0, stream, descs, nco); });
}

hipError_t launch_scan_keep(int format, const ScanDesc* descs, int nstreams, int64_t max_keep, hipStream_t stream)
{
  if (nstreams <= 0 || nstreams > 65535 || max_keep <= 0 || max_keep >= kSize) return nstreams > 65535 || max_keep >= kSize ? hipErrorInvalidValue : hipSuccess;
  const dim3 grid(static_cast<unsigned>((max_keep + kThreads - 1) / kThreads), static_cast<unsigned>(nstreams));
  return by_format(format, [&](auto f) { hipLaunchKernelGGL(scan_keep_kernel<decltype(f)::value>, grid, dim3(kThreads), 0, stream, descs); });
}

}  // namespace dabhip
