// k_tii.hip — transmitter identification's kernel: the de-rotated, fixed-point 2048-point transform of a window of the null symbol and the fold of
// its power onto T[24][8] (include/dabhip.h, "TII").  Integer throughout and rounded only where the header says, so the sums are those of
// tests/tii_model.py whatever the launch shape.
//
// tii_kernel: one workgroup of 256 threads per descriptor; one that does not count leaves at once.  A thread holds 8 points in registers and the 11
//   radix-2 stages are four passes (3 + 3 + 3 + 2 stages) with three exchanges through LDS between them -- 8 registers pair over three stages:
//     pass 0 (h = 1 .. 4):      thread t holds the bit-reversed window's indices 8 t + j -- samples bitrev3(j) 256 + bitrev8(t) of the window, read through
//                               the frame's view, converted and de-rotated on the way;
//     pass 1 (h = 8 .. 32):     thread (hi, lo) = (t >> 3, t & 7) holds indices 64 hi + 8 j + lo;
//     pass 2 (h = 64 .. 256):   thread (hi, lo) = (t >> 6, t & 63) holds indices 512 hi + 64 j + lo;
//     pass 3 (h = 512, 1024):   thread t holds indices 512 j + t and 512 j + t + 256 (j < 4), which are the bins it then owns.
//   The butterfly is the block scan's (fixed_butterfly.hpp).  Both rails of a point are one 8-byte LDS word, index i at i + (i >> 3): the stride of 9
//   spreads pass 0's writes.  The mixer's table, 16 KiB in LDS, serves the de-rotation and the twiddles.  The fold is reduced in LDS (192 64-bit
//   sums) and leaves as 192 64-bit atomic adds to the row, one more for the count of frames: integers, so the order of the workgroups does not matter.
#include <hip/hip_runtime.h>

#include "fixed_butterfly.hpp"
#include "tii.hpp"

namespace dabhip {
namespace {

constexpr int kThreads = 256;
constexpr int kSize = kTiiWindow;
constexpr int kTable = 4096;
constexpr int kRailWords = kSize + kSize / 8;

__device__ __forceinline__ int padded(int i) { return i + (i >> 3); }
constexpr int bitrev3(int j) { return (j & 1) << 2 | (j & 2) | (j & 4) >> 2; }

// NS stages on the 2^NS registers of v: register j is index base + j 2^LOG, and low = base mod 2^LOG
template <int LOG, int NS>
__device__ __forceinline__ void pass(int2* v, int low, const uint32_t* nco)
{
  constexpr int stride = 1 << LOG;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int h = stride << s, per = 2048 / h;
#pragma unroll
    for (int j = 0; j < (1 << NS); ++j) {
      if (j & (1 << s)) continue;
      const int t = (low + (j & ((1 << s) - 1)) * stride) * per;
      int2& a = v[j];
      int2& b = v[j | (1 << s)];
      if (LOG == 0 && t == 0) halve(a, b, b.x, b.y);                // c = 16384, s = 0: (x 16384 + 8192) >> 14 = x
      else if (LOG == 0 && t == 1024) halve(a, b, b.y, -b.x);       // c = 0, s = 16384
      else butterfly(a, b, nco[t]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void tii_kernel(const TiiArgs a, const uint32_t* __restrict__ nco_table)
{
  __shared__ uint32_t nco[kTable];
  __shared__ int2 rail[kRailWords];
  __shared__ unsigned long long fold[kTiiSums];
  const size_t d = blockIdx.x;
  const CallDesc& desc = a.descs[d];
  int w0;
  uint32_t step;
  size_t row;
  if (a.w0) {
    w0 = a.w0[d];
    step = a.step[d];
    row = d;
  } else {
    // the header's counting rule; the same for every thread of the workgroup
    const int fine = desc.fine_timeshift;
    const double ffs = desc.fine_freq_shift;
    if (desc.status != 2 || fine < -kTiiMaxShift || fine > kTiiMaxShift || !(fabs(ffs) < 1024000.0)) return;
    w0 = kTiiW0 + fine;
    const double f = 1000.0 * desc.coarse_freq_shift + ffs + desc.nco_hz;
    step = static_cast<uint32_t>(static_cast<long long>(rint(f * 4294967296.0 / 2048000.0)));
    row = d / static_cast<size_t>(a.max_calls);
  }
  const uint8_t* const stream = a.iq[d / static_cast<size_t>(a.max_calls)];
  const int tid = threadIdx.x;
  for (int i = tid; i < kTable; i += kThreads) nco[i] = nco_table[i];
  if (tid < kTiiSums) fold[tid] = 0;
  __syncthreads();

  int2 v[8];
  const int rev8 = static_cast<int>(__brev(static_cast<unsigned>(tid)) >> 24);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int n = bitrev3(j) * 256 + rev8;                          // 0 .. 2047: frame positions up to 2 (608 + 2047) + 1, far below the tail bytes
    const unsigned w = frame_u16(stream, desc.view, 2 * (w0 + n));
    const int2 x = int2{(static_cast<int>(w & 255u) - 127) * 128, (static_cast<int>(w >> 8) - 127) * 128};
    const uint32_t theta = step * static_cast<uint32_t>(n);
    v[j] = rotate_q14(x, nco[(theta + (1u << 19)) >> 20]);
  }
  pass<0, 3>(v, 0, nco);
#pragma unroll
  for (int j = 0; j < 8; ++j) rail[padded(8 * tid + j)] = v[j];
  __syncthreads();
  {
    const int hi = tid >> 3, lo = tid & 7;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rail[padded(64 * hi + 8 * j + lo)];
    pass<3, 3>(v, lo, nco);
#pragma unroll
    for (int j = 0; j < 8; ++j) rail[padded(64 * hi + 8 * j + lo)] = v[j];      // where this thread read them: nobody else touches these words in between
  }
  __syncthreads();
  {
    const int hi = tid >> 6, lo = tid & 63;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rail[padded(512 * hi + 64 * j + lo)];
    pass<6, 3>(v, lo, nco);
#pragma unroll
    for (int j = 0; j < 8; ++j) rail[padded(512 * hi + 64 * j + lo)] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < 2; ++g) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[4 * g + j] = rail[padded(512 * j + tid + 256 * g)];
    pass<9, 2>(v + 4 * g, tid + 256 * g, nco);
  }
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int slot = tii_slot_of_bin(512 * j + tid + 256 * g);
      const int2 X = v[4 * g + j];
      if (slot >= 0) atomicAdd(&fold[slot], static_cast<unsigned long long>(static_cast<long long>(X.x) * X.x + static_cast<long long>(X.y) * X.y));
    }
  __syncthreads();
  unsigned long long* const out = a.sums + row * kTiiRow;
  if (tid < kTiiSums) atomicAdd(&out[tid], fold[tid]);
  else if (tid == kTiiSums) atomicAdd(&out[kTiiSums], 1ull);
}

}  // namespace

hipError_t launch_tii(const TiiArgs& a, size_t ndesc, const uint32_t* nco, hipStream_t stream)
{
  if (ndesc == 0) return hipSuccess;
  if (ndesc > 0x7fffffffu || a.max_calls <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tii_kernel, dim3(static_cast<unsigned>(ndesc)), dim3(kThreads), 0, stream, a, nco);
  return hipGetLastError();
}

}  // namespace dabhip
