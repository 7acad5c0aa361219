// k_ts.hip — MPEG-2 transport stream packets out of ETI frames in device memory (ETSI TS 102 427: stream-mode sub-channels with the outer
// code RS(204,188) and the convolutional byte interleaver I = 12, M = 17), for many streams and sub-channels at once.  dabhip.h (dabhip_ts) has
// the rules; ts_sync.hpp the sizes, the sync rule 64 slots at a time and the position map; ts.hpp the types.
//
//   locate    one thread per (stream, new frame): FC / STC header, where each requested SubChId sits and its STL
//   layout    one wave per lane (a lane is a (stream, sub-channel)), 64 frames at a time by prefix sums: the lane's virtual byte positions
//             (carried bytes, then the frames' payload), the breaks of its stream, its place in the run-flag buffer
//   runs      parallel over the positions of every lane: one bit per position, "0x47 here and 204, 408, 612 and 816 bytes on, all of one
//             unbroken stream"; a wave's ballot is one 64-bit word of flags
//   sync      one wave per lane from the state of the previous push.  Unsynced it searches 64 words of flags per ballot; synced it loads the
//             bytes at 64 slot starts, takes a ballot and lets ts_chunk_step say which slots give packets and whether sync is lost.  The units
//             (code words) go to fixed slots per lane, so the order is deterministic without atomics
//   scan      one workgroup: prefix sums over the lanes' unit counts; jobs: one workgroup per lane -> the push's unit list
//   gather    one thread per byte of every code word: P + k + 204 (k mod 12) read from the carry or the frame where it lies, byte by byte
//             (so aligned or not), into the word buffer (ts.hpp: ts_word_byte)
//   syndrome  one lane per code word: the 16 syndromes by Horner (rs_code.hpp's step) through an LDS table, four bytes per load, 64 lanes 256
//             contiguous bytes
//   decode    the code words with errors only: Berlekamp-Massey, Chien, Forney and the check by syndromes (rs_code.hpp's rs_solve, the packet
//             stage's tables), in place
//   parse     one thread per packet: its record, its 188 bytes, the counters
//   carry     one workgroup per lane: its unconsumed bytes (at most 2447), for the next push
//
// No scalar-memory writes anywhere.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "eti_locate.hpp"
#include "kernels.hpp"
#include "rs_code.hpp"
#include "ts.hpp"

namespace dabhip {
namespace {

constexpr int kEti = DABHIP_ETI_BYTES;
constexpr int kSyncWaves = kTsSyncWaves;

__global__ void __launch_bounds__(256) ts_locate_kernel(EtiFrames fr, const int32_t* subch, int nsub, int nstreams, int maxv, TsLoc* loc)
{
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(nstreams) * maxv) return;
  const int s = static_cast<int>(t / maxv), v = static_cast<int>(t % maxv);
  if (v >= fr.nnew[s]) return;
  const uint8_t* f = fr.frames + (fr.base[s] + v) * kEti;
  TsLoc* out = loc + t * nsub;
  for (int q = 0; q < nsub; ++q) out[q] = TsLoc{nullptr, 0, 0, 0, 0};
  eti_stc_walk(f, subch, nsub, [out](int q, int stl, bool fits, const uint8_t* p) {
    out[q].stl = stl;
    if (fits && stl > 0) out[q].ptr = p;
  });
}

// the lane of this wave (kSyncWaves waves to a workgroup), or -1
__device__ inline int wave_lane(int nlanes)
{
  const int lane = blockIdx.x * kSyncWaves + (threadIdx.x >> 6);
  return lane < nlanes ? lane : -1;
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ inline int wave_scan(int x, int l)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (l >= d) x += y;
  }
  return x;
}

// A frame breaks the stream in front of it when it gives no bytes, or when its STL differs from that of the frame before it (which gave
// bytes).  So the breaks and the frames' first positions are prefix sums, taken 64 frames at a time.
__global__ void __launch_bounds__(64 * kSyncWaves) ts_layout_kernel(EtiFrames fr, int nlanes, int nsub, int maxv, TsLoc* loc, const TsSync* sync, TsLane* lanes,
                                                                    int flag_cap, int* totals)
{
  const int lane = wave_lane(nlanes);
  if (lane < 0) return;
  const int l = threadIdx.x & 63;
  const int s = lane / nsub, q = lane % nsub;
  const int nnew = fr.nnew[s];
  TsLoc* lc = loc + static_cast<int64_t>(s) * maxv * nsub + q;
  const TsSync st = sync[lane];
  int run = st.ncar, seg = 0, prev_stl = st.stl;
  for (int c0 = 0; c0 < nnew; c0 += 64) {
    const int v = c0 + l;
    const bool have = v < nnew;
    int stl = 0;
    if (have) {
      const TsLoc x = lc[static_cast<int64_t>(v) * nsub];
      stl = x.ptr ? x.stl : 0;
    }
    int before = __shfl_up(stl, 1);
    if (l == 0) before = prev_stl;
    const int brk = have && (stl == 0 || (before != 0 && stl != before));
    const int bytes = 8 * stl;
    const int sum_bytes = wave_scan(bytes, l), sum_brk = wave_scan(brk, l);
    if (have) {
      TsLoc& x = lc[static_cast<int64_t>(v) * nsub];
      x.byte0 = run + sum_bytes - bytes;
      x.seg = seg + sum_brk;
    }
    run += __shfl(sum_bytes, 63);
    seg += __shfl(sum_brk, 63);
    prev_stl = __shfl(stl, 63);
  }
  if (l == 0) {
    const int nwords = (run + 63) >> 6;
    int flag0 = nwords ? atomicAdd(totals + kTsTotFlagWords, nwords) : 0;
    if (flag0 + nwords > flag_cap) {                 // never, by ts.cpp's bound; if ever, the push fails and nothing behind this reads the flags
      totals[kTsTotOverflow] = 1;
      flag0 = 0;
    }
    lanes[lane] = TsLane{run, st.ncar, flag0, 0};
  }
}

// a lane's virtual positions: carried bytes, then the frames of the push
struct TsView {
  const TsLoc* lc;                                   // the lane's entry of frame 0; frame v is lc[v * nsub]
  const uint8_t* carry;                              // the lane's carried bytes
  int nsub, nnew, ncar;
};

__device__ inline TsView ts_view(const EtiFrames& fr, const TsLoc* loc, int lane, int nsub, int maxv, const uint8_t* carry, int ncar)
{
  const int s = lane / nsub, q = lane % nsub;
  return TsView{loc + static_cast<int64_t>(s) * maxv * nsub + q, carry + static_cast<int64_t>(lane) * kTsCarryStride, nsub, fr.nnew[s], ncar};
}

__device__ inline const TsLoc& view_frame(const TsView& v, int u)
{
  const int f = ts_frame_of(v.nnew, u, [&](int i) { return v.lc[static_cast<int64_t>(i) * v.nsub].byte0; });
  return v.lc[static_cast<int64_t>(f) * v.nsub];
}

// the byte at position u < nv
__device__ inline uint8_t view_byte(const TsView& v, int u)
{
  if (u < v.ncar) return v.carry[u];
  const TsLoc& x = view_frame(v, u);
  return x.ptr[u - x.byte0];
}

// the byte at u and the count of breaks in front of it (0 for a carried byte)
__device__ inline uint8_t view_byte_seg(const TsView& v, int u, int& seg)
{
  seg = 0;
  if (u < v.ncar) return v.carry[u];
  const TsLoc& x = view_frame(v, u);
  seg = x.seg;
  return x.ptr[u - x.byte0];
}

// Workgroup b works on lane b / per_lane; its 4 waves take words (b % per_lane) * 4 + wave, then 4 per_lane further, ...
__global__ void __launch_bounds__(256) ts_runs_kernel(EtiFrames fr, int nlanes, int nsub, int maxv, int per_lane, const TsLoc* loc, const TsLane* lanes,
                                                     const uint8_t* carry, const int* totals, unsigned long long* flags)
{
  if (totals[kTsTotOverflow]) return;
  const int lane = blockIdx.x / per_lane;
  if (lane >= nlanes) return;
  const TsLane L = lanes[lane];
  const int nwords = (L.nv + 63) >> 6;
  const int l = threadIdx.x & 63;
  const TsView view = ts_view(fr, loc, lane, nsub, maxv, carry, L.ncar);
  for (int w = (blockIdx.x % per_lane) * 4 + (threadIdx.x >> 6); w < nwords; w += 4 * per_lane) {
    const int p = w * 64 + l;
    bool run = false;
    if (p + kTsRunSpan < L.nv) {
      int seg0, seg4;
      if (view_byte_seg(view, p, seg0) == kTsSyncByte && view_byte_seg(view, p + kTsRunSpan, seg4) == kTsSyncByte && seg0 == seg4)
        run = view_byte(view, p + kTsSlot) == kTsSyncByte && view_byte(view, p + 2 * kTsSlot) == kTsSyncByte && view_byte(view, p + 3 * kTsSlot) == kTsSyncByte;
    }
    const unsigned long long word = __ballot(run);
    if (l == 0) flags[L.flag0 + w] = word;
  }
}

__global__ void __launch_bounds__(64 * kSyncWaves) ts_sync_kernel(EtiFrames fr, int nlanes, int nsub, int maxv, const TsLoc* loc, TsSync* sync, TsLane* lanes,
                                                                  const uint8_t* carry, const unsigned long long* flags, TsSlot* slots, int cap, int* nunits,
                                                                  int64_t* counters, int* totals)
{
  if (totals[kTsTotOverflow]) return;
  const int lane = wave_lane(nlanes);
  if (lane < 0) return;
  const int l = threadIdx.x & 63;
  TsSync st = sync[lane];
  const TsLane L = lanes[lane];
  const TsView view = ts_view(fr, loc, lane, nsub, maxv, carry, L.ncar);
  const unsigned long long* fl = flags + L.flag0;
  TsSlot* mine = slots + static_cast<int64_t>(lane) * cap;
  // everything below is the same in all 64 lanes of the wave
  int lo = 0, n = 0;
  int64_t skipped = 0, losses = 0, from_miss = 0;

  // the first run flag at or above `from` and below `end`, or -1: 64 words of flags per ballot
  const auto find_run = [&](int from, int end) {
    const int w0 = from >> 6, wend = (end + 63) >> 6;
    for (int wb = w0; wb < wend; wb += 64) {
      const int w = wb + l;
      unsigned long long x = w < wend ? fl[w] : 0;
      if (w == w0) x &= ~0ull << (from & 63);
      const unsigned long long any = __ballot(x != 0);
      if (!any) continue;
      const int f = __builtin_ctzll(any);
      const unsigned xl = __shfl(static_cast<unsigned>(x), f), xh = __shfl(static_cast<unsigned>(x >> 32), f);
      const unsigned long long xf = (static_cast<unsigned long long>(xh) << 32) | xl;
      const int p = (wb + f) * 64 + __builtin_ctzll(xf);
      return p < end ? p : -1;
    }
    return -1;
  };

  // the rule over the unbroken stream that ends at `end`
  const auto segment = [&](int end) {
    for (;;) {
      if (!st.synced) {
        const int p = find_run(lo, end);
        if (p < 0) {
          const int wait = static_cast<int>(ts_search_wait(lo, end));
          skipped += wait - lo;
          lo = wait;
          return;
        }
        skipped += p - lo;
        lo = p;
        st.synced = 1;
        st.misses = 0;
      }
      const int64_t ready = ts_slots_ready(end - lo);
      if (ready <= 0) return;
      const int m = ready < kTsChunk ? static_cast<int>(ready) : kTsChunk;
      const bool hit = l < m && view_byte(view, lo + kTsSlot * l) == kTsSyncByte;
      const TsChunkStep r = ts_chunk_step(__ballot(hit), m, st.misses);
      if (l < r.npackets && n + l < cap) mine[n + l] = TsSlot{lo + kTsSlot * l, (r.from_miss >> l & 1) ? DABHIP_TS_FROM_MISS : 0};
      n += r.npackets;
      from_miss += __popcll(r.from_miss);
      lo += kTsSlot * r.npackets;
      if (r.lost) {
        ++losses;
        ++skipped;
        ++lo;
        st.synced = 0;
        st.misses = 0;
      } else {
        st.misses = r.misses;
      }
    }
  };

  const int s = lane / nsub;
  const int nnew = fr.nnew[s];
  int seg_before = 0;
  for (int c0 = 0; c0 < nnew; c0 += 64) {
    const int v = c0 + l;
    const int sg = v < nnew ? view.lc[static_cast<int64_t>(v) * nsub].seg : 0;
    int before = __shfl_up(sg, 1);
    if (l == 0) before = seg_before;
    unsigned long long brk = __ballot(v < nnew && sg != before);
    seg_before = __shfl(sg, 63);
    while (brk) {
      const int f = __builtin_ctzll(brk);
      brk &= brk - 1;
      const int at = view.lc[static_cast<int64_t>(c0 + f) * nsub].byte0;
      segment(at);
      skipped += at - lo;                            // the break: every byte not consumed yet goes, and sync with them
      if (st.synced) ++losses;
      st.synced = st.misses = 0;
      lo = at;
    }
  }
  segment(L.nv);
  if (l != 0) return;
  if (nnew > 0) {
    const TsLoc& last = view.lc[static_cast<int64_t>(nnew - 1) * nsub];
    st.stl = last.ptr ? last.stl : 0;
  }
  st.next_pos += L.nv - L.ncar;
  st.ncar = L.nv - lo;
  sync[lane] = st;
  lanes[lane].lo = lo;
  nunits[lane] = n <= cap ? n : 0;
  if (n > cap) totals[kTsTotSlotOverflow] = 1;       // never, by ts_unit_bound; if ever, the push fails instead of losing the lane's units
  int64_t* cnt = counters + static_cast<int64_t>(lane) * kTsCntN;
  cnt[kTsCntPackets] += n <= cap ? n : 0;
  cnt[kTsCntFromMiss] += from_miss;
  cnt[kTsCntSyncLosses] += losses;
  cnt[kTsCntSkipped] += skipped;
}

// one workgroup of 1024: lanes split in contiguous chunks, a block scan of the units per lane -> the lanes' bases
__global__ void __launch_bounds__(1024) ts_scan_kernel(int nlanes, const int* nunits, int* lane_unit_base, int* totals)
{
  __shared__ int sh[1024];
  const int t = threadIdx.x;
  const int chunk = (nlanes + 1023) / 1024;
  const int a = t * chunk < nlanes ? t * chunk : nlanes, b = a + chunk < nlanes ? a + chunk : nlanes;
  int nu = 0;
  for (int i = a; i < b; ++i) nu += nunits[i];
  sh[t] = nu;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {               // inclusive Hillis-Steele scan
    const int x = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  int u = sh[t] - nu;
  for (int i = a; i < b; ++i) {
    lane_unit_base[i] = u;
    u += nunits[i];
  }
  if (t == 1023) {
    lane_unit_base[nlanes] = sh[1023];
    totals[kTsTotUnits] = sh[1023];
  }
}

// one workgroup per lane: its slots into the push's unit list, in (stream, sub-channel, time) order
__global__ void __launch_bounds__(256) ts_jobs_kernel(const TsSlot* slots, int cap, const int* nunits, const int* lane_unit_base, const TsSync* sync, const TsLane* lanes,
                                                     TsUnit* units, int64_t unit_cap)
{
  const int lane = blockIdx.x;
  const int n = nunits[lane];
  if (n == 0) return;
  const int64_t pos0 = sync[lane].next_pos - lanes[lane].nv;   // of virtual position 0 (next_pos is the push's end already)
  const int base = lane_unit_base[lane];
  if (base + static_cast<int64_t>(n) > unit_cap) return;       // never, by ts.cpp's bound; the host sees the total and fails the push
  TsUnit* out = units + base;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const TsSlot sl = slots[static_cast<int64_t>(lane) * cap + i];
    out[i] = TsUnit{lane, sl.u0, sl.flags, 0, pos0 + sl.u0};
  }
}

// Thread t writes byte t of the word buffer: in group g = t / 13056, byte k = 4 ((t % 13056) / 256) + t % 4 of word 64 g + (t % 256) / 4.
__global__ void __launch_bounds__(256) ts_gather_kernel(EtiFrames fr, const TsUnit* units, const int* totals, const TsLoc* loc, int maxv, int nsub,
                                                       const uint8_t* carry, const TsLane* lanes, uint8_t* words)
{
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t g = t / (64 * kTsSlot);
  const int r = static_cast<int>(t % (64 * kTsSlot));
  const int64_t w = g * 64 + ((r & 255) >> 2);
  if (w >= totals[kTsTotUnits]) return;
  const int k = 4 * (r >> 8) + (r & 3);
  const TsUnit un = units[w];
  const TsView view = ts_view(fr, loc, un.lane, nsub, maxv, carry, lanes[un.lane].ncar);
  words[t] = view_byte(view, static_cast<int>(ts_byte_pos(un.u0, k)));
}

// The hot path: syndromes S_i = r(alpha^i) by Horner, byte 0 first, a lane per code word.  A clean code word (all syndromes zero) is done
// here; the others leave their syndromes for the decode kernel, which keeps this loop's register count low.
__global__ void __launch_bounds__(256) ts_syndrome_kernel(const int* totals, const uint8_t* gf_global, const uint8_t* words, uint8_t* cw_status, uint32_t* syn)
{
  __shared__ uint32_t mul_w[kPkRoots * 64];          // GfRs::mul
  const uint32_t* src = reinterpret_cast<const uint32_t*>(gf_global);
  for (int i = threadIdx.x; i < kPkRoots * 64; i += blockDim.x) mul_w[i] = src[i];
  __syncthreads();
  const uint8_t* mul = reinterpret_cast<const uint8_t*>(mul_w);
  const int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (w >= totals[kTsTotUnits]) return;
  const uint32_t* z = reinterpret_cast<const uint32_t*>(words) + (w >> 6) * (kTsSlot / 4) * 64 + (w & 63);
  uint32_t S[kPkRoots] = {0};
#pragma unroll 3
  for (int c = 0; c < kTsSlot / 4; ++c) {
    const uint32_t four = z[c * 64];
#pragma unroll
    for (int j = 0; j < 4; ++j) rs_horner(mul, S, (four >> (8 * j)) & 0xff);
  }
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < kPkRoots; ++i) any |= S[i];
  cw_status[w] = any ? 0xfe : 0;
  if (any) rs_pack(S, syn + w * 4);
}

// The error path of the code words the syndrome kernel left (status 0xfe): corrected in place in the word buffer, status = symbols corrected
// or 0xff.  A workgroup without such a code word returns before it loads the tables.
__global__ void __launch_bounds__(256) ts_decode_kernel(const int* totals, const uint8_t* gf_global, uint8_t* words, uint8_t* cw_status, const uint32_t* syn)
{
  __shared__ GfRs<kPkRoots> g;
  const int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool need = w < totals[kTsTotUnits] && cw_status[w] == 0xfe;
  if (!__syncthreads_or(need)) return;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(gf_global);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&g);
    for (int i = threadIdx.x; i < static_cast<int>(sizeof(g) / 4); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  if (!need) return;
  uint8_t S8[kPkRoots];
  const uint32_t* o = syn + w * 4;
#pragma unroll
  for (int i = 0; i < kPkRoots; ++i) S8[i] = static_cast<uint8_t>(o[i >> 2] >> (8 * (i & 3)));
  int pos[kPkT] = {0};
  uint8_t val[kPkT] = {0};
  const int n = rs_solve<kPkN, kPkRoots, kPkT>(g, S8, pos, val);
  if (n < 0) {
    cw_status[w] = 0xff;
    return;
  }
  for (int i = 0; i < n; ++i) words[ts_word_byte(w, pos[i])] ^= val[i];
  cw_status[w] = static_cast<uint8_t>(n);
}

// One thread per packet: the record from the first four bytes after decoding, the 188 bytes, the lane's counters.
__global__ void __launch_bounds__(256) ts_parse_kernel(const TsUnit* units, const int* totals, const uint8_t* words, const uint8_t* cw_status, dabhip_ts_rec* recs,
                                                      uint8_t* data, int64_t* counters)
{
  const int64_t w = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (w >= totals[kTsTotUnits]) return;
  const TsUnit un = units[w];
  const uint32_t* z = reinterpret_cast<const uint32_t*>(words) + (w >> 6) * (kTsSlot / 4) * 64 + (w & 63);
  uint32_t* out = reinterpret_cast<uint32_t*>(data + w * kTsData);
  const uint32_t head = z[0];
  out[0] = head;
#pragma unroll 4
  for (int c = 1; c < kTsData / 4; ++c) out[c] = z[c * 64];
  const int b0 = head & 0xff, b1 = (head >> 8) & 0xff, b2 = (head >> 16) & 0xff, b3 = head >> 24;
  const uint8_t st = cw_status[w];
  dabhip_ts_rec r = {};
  r.pos = un.pos;
  r.pid = static_cast<uint16_t>(((b1 & 0x1f) << 8) | b2);
  r.continuity = static_cast<uint8_t>(b3 & 15);
  r.flags = static_cast<uint8_t>(un.flags | (st == 0xff ? DABHIP_TS_RS_FAILED : 0) | ((b1 & 0x80) ? DABHIP_TS_TEI : 0) | ((b1 & 0x40) ? DABHIP_TS_PUSI : 0) |
                                 (b0 != kTsSyncByte ? DABHIP_TS_BAD_SYNC : 0));
  r.corrected = st == 0xff ? 0 : st;
  recs[w] = r;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters + static_cast<int64_t>(un.lane) * kTsCntN);
  if (r.corrected) atomicAdd(cnt + kTsCntRsCorrected, static_cast<unsigned long long>(r.corrected));
  if (st == 0xff) atomicAdd(cnt + kTsCntRsFailed, 1ull);
  if (b0 != kTsSyncByte) atomicAdd(cnt + kTsCntBadSync, 1ull);
  if (r.pid == kTsNullPid) atomicAdd(cnt + kTsCntNull, 1ull);
}

// a lane's unconsumed bytes (positions lo .. nv - 1) into the other carry buffer
__global__ void __launch_bounds__(256) ts_carry_kernel(EtiFrames fr, const TsLoc* loc, int maxv, int nsub, const uint8_t* carry, const TsLane* lanes, const int* totals,
                                                      uint8_t* carry_next)
{
  if (totals[kTsTotOverflow]) return;
  const int lane = blockIdx.x;
  const TsLane L = lanes[lane];
  const int n = L.nv - L.lo;                         // 2447 at most: a synced lane waits for its look-ahead, an unsynced one within 816 of the end
  if (n <= 0 || n > kTsCarry) return;
  const TsView view = ts_view(fr, loc, lane, nsub, maxv, carry, L.ncar);
  uint8_t* dst = carry_next + static_cast<int64_t>(lane) * kTsCarryStride;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = view_byte(view, L.lo + i);
}

}  // namespace

hipError_t launch_ts_locate(const EtiFrames& fr, const int32_t* subch, int nsub, int nstreams, int maxv, TsLoc* loc, const TsSync* sync, TsLane* lanes, int flag_cap,
                            int* totals, hipStream_t stream)
{
  const int64_t n = static_cast<int64_t>(nstreams) * maxv;
  const int nlanes = nstreams * nsub;
  if (n > 0) ts_locate_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, stream>>>(fr, subch, nsub, nstreams, maxv, loc);
  ts_layout_kernel<<<(nlanes + kSyncWaves - 1) / kSyncWaves, 64 * kSyncWaves, 0, stream>>>(fr, nlanes, nsub, maxv, loc, sync, lanes, flag_cap, totals);
  return hipGetLastError();
}

hipError_t launch_ts_runs(const EtiFrames& fr, int nlanes, int nsub, int maxv, int per_lane, const TsLoc* loc, const TsLane* lanes, const uint8_t* carry,
                          const int* totals, uint64_t* flags, hipStream_t stream)
{
  ts_runs_kernel<<<static_cast<unsigned>(static_cast<int64_t>(nlanes) * per_lane), 256, 0, stream>>>(fr, nlanes, nsub, maxv, per_lane, loc, lanes, carry, totals,
                                                                                                      reinterpret_cast<unsigned long long*>(flags));
  return hipGetLastError();
}

hipError_t launch_ts_sync(const EtiFrames& fr, int nlanes, int nsub, int maxv, const TsLoc* loc, TsSync* sync, TsLane* lanes, const uint8_t* carry,
                          const uint64_t* flags, TsSlot* slots, int cap, int* nunits, int64_t* counters, int* totals, hipStream_t stream)
{
  ts_sync_kernel<<<(nlanes + kSyncWaves - 1) / kSyncWaves, 64 * kSyncWaves, 0, stream>>>(fr, nlanes, nsub, maxv, loc, sync, lanes, carry,
                                                                                        reinterpret_cast<const unsigned long long*>(flags), slots, cap, nunits, counters,
                                                                                        totals);
  return hipGetLastError();
}

hipError_t launch_ts_jobs(int nlanes, const TsSlot* slots, int cap, const int* nunits, int* lane_unit_base, const TsSync* sync, const TsLane* lanes, TsUnit* units,
                          int64_t unit_cap, int* totals, hipStream_t stream)
{
  ts_scan_kernel<<<1, 1024, 0, stream>>>(nlanes, nunits, lane_unit_base, totals);
  ts_jobs_kernel<<<nlanes, 256, 0, stream>>>(slots, cap, nunits, lane_unit_base, sync, lanes, units, unit_cap);
  return hipGetLastError();
}

hipError_t launch_ts_gather(const EtiFrames& fr, const TsUnit* units, const int* totals, int64_t nunits, const TsLoc* loc, int maxv, int nsub, const uint8_t* carry,
                            const TsLane* lanes, uint8_t* words, hipStream_t stream)
{
  const int64_t n = ts_word_buffer_bytes(nunits);
  if (n > 0) ts_gather_kernel<<<static_cast<unsigned>(n / 256), 256, 0, stream>>>(fr, units, totals, loc, maxv, nsub, carry, lanes, words);
  return hipGetLastError();
}

hipError_t launch_ts_syndrome(const int* totals, int64_t nunits, const uint8_t* gf_tables, const uint8_t* words, uint8_t* cw_status, uint32_t* syn, hipStream_t stream)
{
  if (nunits > 0) ts_syndrome_kernel<<<static_cast<unsigned>((nunits + 255) / 256), 256, 0, stream>>>(totals, gf_tables, words, cw_status, syn);
  return hipGetLastError();
}

hipError_t launch_ts_decode(const int* totals, int64_t nunits, const uint8_t* gf_tables, uint8_t* words, uint8_t* cw_status, const uint32_t* syn, hipStream_t stream)
{
  if (nunits > 0) ts_decode_kernel<<<static_cast<unsigned>((nunits + 255) / 256), 256, 0, stream>>>(totals, gf_tables, words, cw_status, syn);
  return hipGetLastError();
}

hipError_t launch_ts_parse(const TsUnit* units, const int* totals, int64_t nunits, const uint8_t* words, const uint8_t* cw_status, dabhip_ts_rec* recs, uint8_t* data,
                           int64_t* counters, hipStream_t stream)
{
  if (nunits > 0) ts_parse_kernel<<<static_cast<unsigned>((nunits + 255) / 256), 256, 0, stream>>>(units, totals, words, cw_status, recs, data, counters);
  return hipGetLastError();
}

hipError_t launch_ts_carry(const EtiFrames& fr, int nlanes, const TsLoc* loc, int maxv, int nsub, const uint8_t* carry, const TsLane* lanes, const int* totals,
                           uint8_t* carry_next, hipStream_t stream)
{
  if (nlanes > 0) ts_carry_kernel<<<nlanes, 256, 0, stream>>>(fr, loc, maxv, nsub, carry, lanes, totals, carry_next);
  return hipGetLastError();
}

}  // namespace dabhip
