// k_dir.hip — the ensemble directory out of ETI frames (dabhip.h: "ensemble directory"; the rules are dir_figs.hpp's, the types dir.hpp's).
//
// fibs   a thread per (stream, new frame, FIB): the frame's header, the CRC over 30 bytes, the FIG walk (dir_walk_fib, the text the host runs
//        too).  Its facts go to the FIB's own 32 slots, so their order needs no atomics; its counts go to the FIB's DirFib record.
// merge  a wave per stream.  The stream's tables (196 entries of 88 bytes) are staged in LDS.  The wave takes the DirFib records 64 at a time, a
//        lane each, sums their counts per lane, and visits only the FIBs a ballot shows to hold facts.  A table of services or packet
//        components lies one entry per lane: finding a key is one compare and one ballot, appending is the table's count.  The payload of a
//        fact is compared and stored a byte per lane; a ballot says whether it altered anything.  No thread ever walks a stream alone, and
//        nothing is added atomically: the wave owns its stream.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace dabhip {

namespace {

constexpr int kFibsBlock = 256;

__global__ void __launch_bounds__(kFibsBlock) dir_fibs_kernel(EtiFrames fr, int maxv, DirFib* fibs, DirFact* facts)
{
  const int s = blockIdx.x;
  const int t = blockIdx.y * kFibsBlock + threadIdx.x;
  const int v = t / 3, q = t - 3 * v;
  if (v >= maxv || v >= fr.nnew[s]) return;
  const int64_t g = (fr.base[s] + v) * 3 + q;
  const uint8_t* frame = fr.frames + (fr.base[s] + v) * DABHIP_ETI_BYTES;
  DirFib rec = {0, 0, 0, 0, 0, {0, 0, 0}};
  if (q == 0) rec.cls |= kDirFrame;
  int off = 0;
  const int cls = dir_frame_class(frame, &off);
  if (cls != 0) {
    if (q == 0) rec.cls |= cls == 1 ? kDirFrameNoFic : kDirFrameSkipped;
  } else {
    const uint8_t* fib = frame + off + kDirFibBytes * q;           // off <= 268: the FIB ends at byte 364 at most
    rec.cls |= kDirFibSeen;
    if (!dir_fib_crc_ok(fib)) {
      rec.cls |= kDirFibCrcFailed;
    } else {
      const DirFibStat st = dir_walk_fib(fib, facts + g * kDirFactSlots);
      rec.nfacts = static_cast<uint8_t>(st.nfacts);
      rec.figs = static_cast<uint8_t>(st.figs);
      rec.truncated = static_cast<uint8_t>(st.truncated);
      rec.ignored = static_cast<uint8_t>(st.ignored);
    }
  }
  fibs[g] = rec;
}

__device__ inline int64_t wave_sum(int64_t x)
{
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned lo = __shfl_xor(static_cast<unsigned>(x), d), hi = __shfl_xor(static_cast<unsigned>(static_cast<uint64_t>(x) >> 32), d);
    x += static_cast<int64_t>(static_cast<uint64_t>(hi) << 32 | lo);
  }
  return x;
}

__global__ void __launch_bounds__(64) dir_merge_kernel(EtiFrames fr, const DirFib* fibs, const DirFact* facts, DirStream* state, int* ok_fibs)
{
  __shared__ DirEntry tab[kDirEntries];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int nnew = fr.nnew[s];
  if (nnew == 0) {
    if (lane == 0) ok_fibs[s] = 0;
    return;
  }
  DirStream& ds = state[s];
  constexpr int kWords = static_cast<int>(sizeof(DirEntry) * kDirEntries / 4);
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(ds.e);
    uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
    for (int w = lane; w < kWords; w += 64) dst[w] = src[w];
  }
  int nsvc = ds.nsvc, npkt = ds.npkt;
  const int64_t frame0 = ds.counters[kDirCntFrames];
  __syncthreads();

  // per-lane sums of the DirFib records' counts; changed / dropped are the wave's own (the same in every lane)
  int c_frames = 0, c_nofic = 0, c_skipped = 0, c_fibs = 0, c_crc = 0, c_figs = 0, c_trunc = 0, c_ign = 0, c_facts = 0;
  int64_t changed = 0, dropped = 0;
  const int64_t g0 = fr.base[s] * 3;
  const int nfib = 3 * nnew;
  for (int c0 = 0; c0 < nfib; c0 += 64) {
    DirFib rec = {0, 0, 0, 0, 0, {0, 0, 0}};
    if (c0 + lane < nfib) rec = fibs[g0 + c0 + lane];
    c_frames += (rec.cls & kDirFrame) != 0;
    c_nofic += (rec.cls & kDirFrameNoFic) != 0;
    c_skipped += (rec.cls & kDirFrameSkipped) != 0;
    c_fibs += (rec.cls & kDirFibSeen) != 0;
    c_crc += (rec.cls & kDirFibCrcFailed) != 0;
    c_figs += rec.figs;
    c_trunc += rec.truncated;
    c_ign += rec.ignored;
    c_facts += rec.nfacts;
    unsigned long long busy = __ballot(rec.nfacts != 0);
    while (busy) {
      const int l = __builtin_ctzll(busy);
      busy &= busy - 1;
      const int n = min(__shfl(static_cast<int>(rec.nfacts), l), kDirFactSlots);
      const int64_t frame = frame0 + (c0 + l) / 3;
      const DirFact* f = facts + (g0 + c0 + l) * kDirFactSlots;
      for (int i = 0; i < n; ++i, ++f) {
        const int kind = f->kind, pd = f->pd;
        const uint32_t key = f->key;
        int idx, part = 0;
        if (kind == kDirEns00 || kind == kDirEns09 || kind == kDirEns10 || kind == kDirLblEns) {
          idx = kind == kDirEns00 ? 0 : kind == kDirEns09 ? 1 : kind == kDirEns10 ? 2 : 3;
        } else if (kind == kDirSub01 || kind == kDirFec14) {
          idx = kDirSubBase + static_cast<int>(key & 63);
          part = kind == kDirFec14;
        } else if (kind == kDirSvc02 || kind == kDirLblSvc || kind == kDirPkt03) {
          const bool svc = kind != kDirPkt03;
          const int base = svc ? kDirSvcBase : kDirPktBase;
          const int count = svc ? nsvc : npkt;
          part = kind == kDirLblSvc;
          const DirEntry& mine = tab[base + lane];
          const unsigned long long hit = __ballot(lane < count && mine.key == key && mine.pd == pd);
          if (hit) {
            idx = base + __builtin_ctzll(hit);
          } else if (count < kDirTable) {
            idx = base + count;
            if (svc) ++nsvc; else ++npkt;
            if (lane == 0) {
              tab[idx].key = key;
              tab[idx].pd = static_cast<uint8_t>(pd);
            }
            __syncthreads();
          } else {
            ++dropped;
            continue;
          }
        } else {
          continue;                                      // (no such kind comes out of dir_walk_fib)
        }
        DirEntry& e = tab[idx];
        const int len = dir_fact_len(kind);
        uint8_t* dst = part ? e.part1 : e.part0;
        const int have = e.have;
        const bool mine = lane < len;
        const uint8_t nb = mine ? f->payload[lane] : 0;
        const unsigned long long diff = __ballot(mine && dst[lane] != nb);
        const bool change = ((have >> part) & 1) && diff != 0;
        __syncthreads();                                 // every lane has read e.have before lane 0 writes it
        if (mine) dst[lane] = nb;
        if (lane == 0) {
          if (have == 0) e.first = frame;
          e.last = frame;
          e.have = static_cast<uint8_t>(have | (1 << part));
          if (change) ++e.changes;
        }
        changed += change;
        __syncthreads();
      }
    }
  }
  __syncthreads();
  {
    uint32_t* dst = reinterpret_cast<uint32_t*>(ds.e);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tab);
    for (int w = lane; w < kWords; w += 64) dst[w] = src[w];
  }
  const int64_t sums[9] = {wave_sum(c_frames), wave_sum(c_nofic), wave_sum(c_skipped), wave_sum(c_fibs), wave_sum(c_crc),
                           wave_sum(c_figs),   wave_sum(c_trunc), wave_sum(c_ign),     wave_sum(c_facts)};
  if (lane == 0) {
    ds.nsvc = nsvc;
    ds.npkt = npkt;
    for (int k = 0; k < 9; ++k) ds.counters[k] += sums[k];
    ds.counters[kDirCntChanged] += changed;
    ds.counters[kDirCntDropped] += dropped;
    ok_fibs[s] = static_cast<int>(sums[3] - sums[4]);
  }
}

}  // namespace

hipError_t launch_dir_fibs(const EtiFrames& fr, int nstreams, int maxv, DirFib* fibs, DirFact* facts, hipStream_t stream)
{
  if (nstreams <= 0 || maxv <= 0) return hipSuccess;
  const dim3 grid(static_cast<unsigned>(nstreams), static_cast<unsigned>((3 * maxv + kFibsBlock - 1) / kFibsBlock));
  hipLaunchKernelGGL(dir_fibs_kernel, grid, dim3(kFibsBlock), 0, stream, fr, maxv, fibs, facts);
  return hipGetLastError();
}

hipError_t launch_dir_merge(const EtiFrames& fr, int nstreams, const DirFib* fibs, const DirFact* facts, DirStream* state, int* ok_fibs, hipStream_t stream)
{
  if (nstreams <= 0) return hipSuccess;
  hipLaunchKernelGGL(dir_merge_kernel, dim3(static_cast<unsigned>(nstreams)), dim3(64), 0, stream, fr, fibs, facts, state, ok_fibs);
  return hipGetLastError();
}

}  // namespace dabhip
