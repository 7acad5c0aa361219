// k_dabplus.hip — DAB+ audio superframes out of ETI frames in device memory (ETSI TS 102 563), for many streams and sub-channels at once.
//
//   locate   one thread per (stream, frame): FC / STC header, where each requested SubChId sits, its STL, FCT and raw fire code
//   sync     one lane per (stream, sub-channel), walking that stream's frames in order from the state of the previous push (dabhip.h has the rule);
//            candidates go to fixed slots per lane (at most frames / 5 + 1), so the order is deterministic without atomics
//   scan     one workgroup: prefix sums over the lanes' superframe and codeword counts; jobs: one thread per candidate -> the push's
//            superframe list, codeword and data numbering
//   rs       one lane per codeword: syndromes and the data copy (the hot path); then, for the codewords with errors only, Berlekamp-Massey,
//            Chien search, Forney and the check by syndromes in a second kernel.  The code's tables, its Horner step and its solver are
//            rs_code.hpp's, shared with k_packet.hip and k_ts.hip; the addressing (loc_at, the stride s) is this file's
//   au       one wave per superframe: fire code, header, au_start checks, AU CRCs, the record, the counters
//   carry    one workgroup per stream: the last 4 frames, for the next push
//
// The frames are read in place through the locate table (the carried ones from the carry buffer).  No scalar-memory writes anywhere.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dabplus.hpp"
#include "eti_locate.hpp"
#include "kernels.hpp"
#include "rs_code.hpp"

namespace dabhip {
namespace {

constexpr int kEti = DABHIP_ETI_BYTES;

__device__ inline const DabPlusLoc& loc_at(const DabPlusLoc* loc, int stream, int v, int sub, int maxv, int nsub)
{
  return loc[(static_cast<int64_t>(stream) * maxv + v) * nsub + sub];
}

__global__ void __launch_bounds__(256) dabplus_locate_kernel(DabPlusFrames fr, const int32_t* subch, int nsub, int nstreams, int maxv, DabPlusLoc* loc)
{
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(nstreams) * maxv) return;
  const int s = static_cast<int>(t / maxv), v = static_cast<int>(t % maxv);
  const int c = fr.ncarry[s];
  if (v >= c + fr.nnew[s]) return;
  const uint8_t* f = v < c ? fr.carry + (static_cast<int64_t>(s) * 4 + v) * kEti : fr.frames + (fr.base[s] + (v - c)) * kEti;
  const uint8_t fct = f[4];
  DabPlusLoc* out = loc + t * nsub;
  for (int q = 0; q < nsub; ++q) out[q] = DabPlusLoc{nullptr, 0, fct, 0, {0, 0}};
  eti_stc_walk(f, subch, nsub, [out](int q, int stl, bool fits, const uint8_t* p) {
    out[q].stl = stl;
    if (fits && stl > 0 && stl % 3 == 0 && stl <= 3 * kMaxS) {        // s <= 72: the au kernel's LDS copy of a superframe
      out[q].ptr = p;
      out[q].raw_fire = fire_code(p + 2) == ((p[0] << 8) | p[1]);
    }
  });
}

__global__ void __launch_bounds__(64) dabplus_sync_kernel(DabPlusFrames fr, int nstreams, int nsub, int maxv, const DabPlusLoc* loc, DabPlusSync* sync,
                                                          DabPlusCand* cand, int cap, int* ncand, int* lane_cw, int64_t* counters)
{
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nstreams * nsub) return;
  const int s = lane / nsub, q = lane % nsub;
  DabPlusSync st = sync[lane];
  const int total = fr.ncarry[s] + fr.nnew[s];
  int f = fr.ncarry[s] - st.back;
  int n = 0, losses = 0, ncw = 0;
  while (f + 4 < total) {
    DabPlusLoc w[kSfFrames];
    for (int i = 0; i < kSfFrames; ++i) w[i] = loc_at(loc, s, f + i, q, maxv, nsub);
    bool same = true;
    for (int i = 0; i < kSfFrames; ++i) same = same && w[i].ptr != nullptr && w[i].stl == w[0].stl;
    for (int i = 0; i < kSfFrames - 1; ++i) same = same && (w[i].fct + 1) % kFctMod == w[i + 1].fct;
    const bool raw = w[0].ptr != nullptr && w[0].raw_fire;
    if (!st.synced) {
      if (same && raw) {
        st.synced = 1;
        st.fails = 0;
        st.stl = w[0].stl;
      } else {
        ++f;
        continue;
      }
    } else {
      if (!same || w[0].stl != st.stl || (st.last_fct + 1) % kFctMod != w[0].fct) {
        st.synced = 0;
        ++losses;
        continue;                                   // search again from this frame
      }
      st.fails = raw ? 0 : st.fails + 1;
      if (st.fails >= kSyncFailLimit) {
        st.synced = 0;
        ++losses;
        ++f;
        continue;
      }
    }
    if (n < cap) cand[static_cast<int64_t>(lane) * cap + n] = DabPlusCand{f, w[0].stl / 3, ncw};
    ++n;
    ncw += w[0].stl / 3;
    st.last_fct = w[4].fct;
    f += kSfFrames;
  }
  st.back = total - f;
  sync[lane] = st;
  ncand[lane] = n < cap ? n : cap;
  lane_cw[lane] = ncw;
  counters[static_cast<int64_t>(lane) * kCntN + kCntSuperframes] += n < cap ? n : cap;
  counters[static_cast<int64_t>(lane) * kCntN + kCntSyncLosses] += losses;
}

// one workgroup of 1024: lanes split in contiguous chunks, a block scan of (superframes, codewords) per lane -> the lanes' bases
__global__ void __launch_bounds__(1024) dabplus_scan_kernel(int nlanes, const int* ncand, const int* lane_cw, int* lane_sf_base, int* lane_cw_base, int* totals)
{
  __shared__ int sh_sf[1024], sh_cw[1024];
  const int t = threadIdx.x;
  const int chunk = (nlanes + 1023) / 1024;
  const int a = t * chunk < nlanes ? t * chunk : nlanes, b = a + chunk < nlanes ? a + chunk : nlanes;
  int nsf = 0, ncw = 0;
  for (int l = a; l < b; ++l) {
    nsf += ncand[l];
    ncw += lane_cw[l];
  }
  sh_sf[t] = nsf;
  sh_cw[t] = ncw;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {             // inclusive Hillis-Steele scan
    const int x = t >= d ? sh_sf[t - d] : 0, y = t >= d ? sh_cw[t - d] : 0;
    __syncthreads();
    sh_sf[t] += x;
    sh_cw[t] += y;
    __syncthreads();
  }
  int sf = sh_sf[t] - nsf, cw = sh_cw[t] - ncw;
  for (int l = a; l < b; ++l) {
    lane_sf_base[l] = sf;
    lane_cw_base[l] = cw;
    sf += ncand[l];
    cw += lane_cw[l];
  }
  if (t == 1023) {
    lane_sf_base[nlanes] = sh_sf[1023];
    totals[0] = sh_sf[1023];
    totals[1] = sh_cw[1023];
  }
}

// one thread per candidate slot: the push's superframe list in (stream, sub-channel, time) order
__global__ void __launch_bounds__(256) dabplus_jobs_kernel(int nlanes, int nsub, const DabPlusCand* cand, int cap, const int* ncand, const int* lane_sf_base,
                                                         const int* lane_cw_base, DabPlusJob* jobs)
{
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(nlanes) * cap) return;
  const int l = static_cast<int>(t / cap), i = static_cast<int>(t % cap);
  if (i >= ncand[l]) return;
  const DabPlusCand c = cand[t];
  const int cw = lane_cw_base[l] + c.cw_off;
  jobs[lane_sf_base[l] + i] = DabPlusJob{l / nsub, l % nsub, c.v0, c.s, static_cast<int64_t>(cw) * kRsK, cw, i};
}

// the superframe of codeword cw: the last job with cw_base <= cw
__device__ inline int job_of(const DabPlusJob* jobs, int nsf, int cw)
{
  int lo = 0, hi = nsf - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].cw_base <= cw) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The hot path: syndromes S_i = r(alpha^i) by Horner, byte 0 first, and the received data bytes copied out.  Row k of a superframe is
// contiguous across the lanes of that superframe, so the byte gathers from the five frames coalesce.  A clean codeword (all syndromes zero)
// is done here; the others leave their syndromes for the decode kernel, which keeps this loop's register count low.
__global__ void __launch_bounds__(256) dabplus_syndrome_kernel(const DabPlusJob* jobs, const int* totals, const DabPlusLoc* loc, int maxv, int nsub,
                                                              const uint8_t* gf_global, uint8_t* data, uint8_t* cw_status, uint32_t* syn)
{
  __shared__ uint32_t mul_w[kRsRoots * 64];          // GfRs::mul, x alpha^i for i = 0..9
  const uint32_t* src = reinterpret_cast<const uint32_t*>(gf_global);
  for (int i = threadIdx.x; i < kRsRoots * 64; i += blockDim.x) mul_w[i] = src[i];
  __syncthreads();
  const uint8_t* mul = reinterpret_cast<const uint8_t*>(mul_w);
  const int nsf = totals[0], ncw = totals[1];
  const int cw = blockIdx.x * blockDim.x + threadIdx.x;
  if (cw >= ncw) return;
  const DabPlusJob jb = jobs[job_of(jobs, nsf, cw)];
  const int s = jb.s, j = cw - jb.cw_base;
  uint8_t* out = data + jb.data_base + j;
  uint32_t S[kRsRoots] = {0};
  for (int m = 0; m < kSfFrames; ++m) {
    const uint8_t* p = loc_at(loc, jb.stream, jb.v0 + m, jb.sub, maxv, nsub).ptr + j;
#pragma unroll 4
    for (int r = 0; r < 24; ++r) {
      const uint8_t b = p[r * s];
      const int k = 24 * m + r;
      if (k < kRsK) out[k * s] = b;
      rs_horner(mul, S, b);
    }
  }
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < kRsRoots; ++i) any |= S[i];
  cw_status[cw] = any ? 0xfe : 0;
  if (any) rs_pack(S, syn + static_cast<int64_t>(cw) * 4);
}

// The error path of the codewords the syndrome kernel left (status 0xfe): corrected bytes written over the copied ones, status = symbols
// corrected or 0xff.  A workgroup without such a codeword returns before it loads the tables.
__global__ void __launch_bounds__(256) dabplus_decode_kernel(const DabPlusJob* jobs, const int* totals, const DabPlusLoc* loc, int maxv, int nsub,
                                                            const uint8_t* gf_global, uint8_t* data, uint8_t* cw_status, const uint32_t* syn)
{
  __shared__ GfRs<kRsRoots> g;
  const int nsf = totals[0], ncw = totals[1];
  const int cw = blockIdx.x * blockDim.x + threadIdx.x;
  const bool need = cw < ncw && cw_status[cw] == 0xfe;
  if (!__syncthreads_or(need)) return;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(gf_global);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&g);
    for (int i = threadIdx.x; i < static_cast<int>(sizeof(g) / 4); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  if (!need) return;
  const DabPlusJob jb = jobs[job_of(jobs, nsf, cw)];
  const int s = jb.s, j = cw - jb.cw_base;
  uint8_t S8[kRsRoots];
  const uint32_t* o = syn + static_cast<int64_t>(cw) * 4;
#pragma unroll
  for (int i = 0; i < kRsRoots; ++i) S8[i] = static_cast<uint8_t>(o[i >> 2] >> (8 * (i & 3)));
  int pos[kRsT] = {0};
  uint8_t val[kRsT] = {0};
  const int n = rs_solve<kRsN, kRsRoots, kRsT>(g, S8, pos, val);
  if (n < 0) {
    cw_status[cw] = 0xff;
    return;
  }
  uint8_t* out = data + jb.data_base + j;
  for (int r = 0; r < n; ++r) {
    const int k = pos[r];
    if (k < kRsK) out[k * s] ^= val[r];
  }
  cw_status[cw] = static_cast<uint8_t>(n);
}

// GF(2)[x] modulo the CRC generator G = x^16 + x^12 + x^5 + 1: a b mod G
__device__ inline uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (int i = 0; i < 16; ++i)
    if (b >> i & 1) p ^= a << i;
  for (int i = 30; i >= 16; --i)
    if (p >> i & 1) p ^= 0x11021u << (i - 16);
  return p;
}

// One wave per superframe.  The AU CRCs are split over the wave: the register of the table-driven CRC over bytes M from initial value I is
// (I x^(8 |M|) + M(x) x^16) mod G, so each lane runs the CRC of its slice of the superframe from 0 and shifts it past the rest of each AU it
// touches (xpow8[n] = x^(8 n) mod G); the wave XORs the parts per AU.  The superframe comes into LDS by 16-byte loads from the 16-byte
// boundary below it (the data buffer has 16 bytes of slack at its end).
__global__ void __launch_bounds__(64) dabplus_au_kernel(const DabPlusJob* jobs, const DabPlusLoc* loc, int maxv, int nsub, const uint8_t* data,
                                                       const uint8_t* cw_status, const uint16_t* crc_tab_global, const uint16_t* xpow8,
                                                       dabhip_dabplus_sf* recs, int64_t* counters)
{
  __shared__ uint4 raw[(kRsK * kMaxS + 31) / 16];
  __shared__ uint16_t crc_tab[256];
  __shared__ int sh_starts[kMaxAus + 1], sh_layout;
  const int sf = blockIdx.x, t = threadIdx.x;
  const DabPlusJob jb = jobs[sf];
  const int len = kRsK * jb.s;
  const int64_t base16 = jb.data_base & ~static_cast<int64_t>(15);
  const int lead = static_cast<int>(jb.data_base - base16), nvec = (lead + len + 15) / 16;
  const uint4* src = reinterpret_cast<const uint4*>(data + base16);
  for (int i = t; i < nvec; i += 64) raw[i] = src[i];
  for (int i = t; i < 256; i += 64) crc_tab[i] = crc_tab_global[i];
  const uint8_t* buf = reinterpret_cast<const uint8_t*>(raw) + lead;
  int fixed = 0, failed = 0;
  for (int j = t; j < jb.s; j += 64) {
    const uint8_t st = cw_status[jb.cw_base + j];
    if (st == 0xff) ++failed; else fixed += st;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    fixed += __shfl_xor(fixed, d);
    failed += __shfl_xor(failed, d);
  }
  __syncthreads();
  dabhip_dabplus_sf rec = {};
  if (t == 0) {
    rec.stream = jb.stream;
    rec.sub = jb.sub;
    rec.fct = loc_at(loc, jb.stream, jb.v0, jb.sub, maxv, nsub).fct;
    rec.s = jb.s;
    rec.fire_ok = fire_code(buf + 2) == ((buf[0] << 8) | buf[1]);
    const uint8_t b2 = buf[2];
    rec.rfa = b2 >> 7;
    rec.dac_rate = (b2 >> 6) & 1;
    rec.sbr_flag = (b2 >> 5) & 1;
    rec.aac_channel_mode = (b2 >> 4) & 1;
    rec.ps_flag = (b2 >> 3) & 1;
    rec.mpeg_surround_config = b2 & 7;
    int n = 0, start0 = 0;
    au_layout(rec.dac_rate, rec.sbr_flag, &n, &start0);
    rec.num_aus = n;
    int layout = rec.fire_ok;
    sh_starts[0] = start0;
    for (int i = 1; i < n; ++i) sh_starts[i] = au_start_field(buf, i);
    sh_starts[n] = len;
    for (int i = 0; i < n; ++i) layout = layout && sh_starts[i + 1] - sh_starts[i] >= 3 && sh_starts[i + 1] <= len;
    rec.layout_ok = layout;
    sh_layout = layout ? n : 0;
  }
  __syncthreads();
  const int nau = sh_layout;
  const int slice = (len + 63) / 64, lo = t * slice, hi = lo + slice < len ? lo + slice : len;
  uint32_t crc_ok = 0;
  for (int i = 0; i < nau; ++i) {
    const int a = sh_starts[i], e = sh_starts[i + 1] - 2;          // CRC over [a, e), stored in e, e + 1
    const int x = lo > a ? lo : a, y = hi < e ? hi : e;
    uint32_t part = 0;
    if (x < y) {
      uint32_t c = 0;
      for (int k = x; k < y; ++k) c = (crc_tab[(buf[k] ^ (c >> 8)) & 0xff] ^ (c << 8)) & 0xffff;
      part = crc_mulmod(c, xpow8[e - y]);
    }
    for (int d = 32; d >= 1; d >>= 1) part ^= __shfl_xor(part, d);
    const uint32_t reg = part ^ crc_mulmod(0xffff, xpow8[e - a]);
    if ((reg ^ 0xffff) == static_cast<uint32_t>((buf[e] << 8) | buf[e + 1])) crc_ok |= 1u << i;
  }
  if (t == 0) {
    for (int i = 0; i < nau; ++i) {
      rec.au_start[i] = static_cast<uint16_t>(sh_starts[i]);
      rec.au_len[i] = static_cast<uint16_t>(sh_starts[i + 1] - sh_starts[i]);
    }
    rec.crc_ok = crc_ok;
    rec.rs_corrected = fixed;
    rec.rs_failed = failed;
    recs[sf] = rec;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters + (static_cast<int64_t>(jb.stream) * nsub + jb.sub) * kCntN);
    atomicAdd(cnt + kCntFireFails, rec.fire_ok ? 0ull : 1ull);
    atomicAdd(cnt + kCntRsCorrected, static_cast<unsigned long long>(fixed));
    atomicAdd(cnt + kCntRsFailed, static_cast<unsigned long long>(failed));
    atomicAdd(cnt + kCntAus, static_cast<unsigned long long>(nau));
    atomicAdd(cnt + kCntAuCrcFails, static_cast<unsigned long long>(nau - __popc(crc_ok)));
  }
}

// the last min(4, carried + new) frames of every stream into the other carry buffer
__global__ void __launch_bounds__(256) dabplus_carry_kernel(DabPlusFrames fr, uint8_t* carry_next)
{
  const int s = blockIdx.x;
  const int c = fr.ncarry[s], total = c + fr.nnew[s];
  const int keep = total < 4 ? total : 4;
  for (int i = 0; i < keep; ++i) {
    const int v = total - keep + i;
    const uint8_t* src = v < c ? fr.carry + (static_cast<int64_t>(s) * 4 + v) * kEti : fr.frames + (fr.base[s] + (v - c)) * kEti;
    uint8_t* dst = carry_next + (static_cast<int64_t>(s) * 4 + i) * kEti;
    if (fr.aligned) {
      for (int w = threadIdx.x; w < kEti / 16; w += blockDim.x) reinterpret_cast<uint4*>(dst)[w] = reinterpret_cast<const uint4*>(src)[w];
    } else {
      for (int w = threadIdx.x; w < kEti; w += blockDim.x) dst[w] = src[w];
    }
  }
}

}  // namespace

hipError_t launch_dabplus_locate(const DabPlusFrames& fr, const int32_t* subch, int nsub, int nstreams, int maxv, DabPlusLoc* loc, hipStream_t stream)
{
  const int64_t n = static_cast<int64_t>(nstreams) * maxv;
  if (n > 0) dabplus_locate_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, stream>>>(fr, subch, nsub, nstreams, maxv, loc);
  return hipGetLastError();
}

hipError_t launch_dabplus_sync(const DabPlusFrames& fr, int nstreams, int nsub, int maxv, const DabPlusLoc* loc, DabPlusSync* sync, DabPlusCand* cand,
                               int cap, int* ncand, int* lane_cw, int64_t* counters, DabPlusJob* jobs, int* lane_sf_base, int* lane_cw_base, int* totals,
                               hipStream_t stream)
{
  const int nlanes = nstreams * nsub;
  const int64_t slots = static_cast<int64_t>(nlanes) * cap;
  dabplus_sync_kernel<<<(nlanes + 63) / 64, 64, 0, stream>>>(fr, nstreams, nsub, maxv, loc, sync, cand, cap, ncand, lane_cw, counters);
  dabplus_scan_kernel<<<1, 1024, 0, stream>>>(nlanes, ncand, lane_cw, lane_sf_base, lane_cw_base, totals);
  dabplus_jobs_kernel<<<static_cast<unsigned>((slots + 255) / 256), 256, 0, stream>>>(nlanes, nsub, cand, cap, ncand, lane_sf_base, lane_cw_base, jobs);
  return hipGetLastError();
}

hipError_t launch_dabplus_rs(const DabPlusJob* jobs, const int* totals, int ncw, const DabPlusLoc* loc, int maxv, int nsub, const uint8_t* gf_tables,
                             uint8_t* data, uint8_t* cw_status, uint32_t* syn, hipStream_t stream)
{
  if (ncw <= 0) return hipSuccess;
  dabplus_syndrome_kernel<<<(ncw + 255) / 256, 256, 0, stream>>>(jobs, totals, loc, maxv, nsub, gf_tables, data, cw_status, syn);
  dabplus_decode_kernel<<<(ncw + 255) / 256, 256, 0, stream>>>(jobs, totals, loc, maxv, nsub, gf_tables, data, cw_status, syn);
  return hipGetLastError();
}

hipError_t launch_dabplus_au(const DabPlusJob* jobs, int nsf, const DabPlusLoc* loc, int maxv, int nsub, const uint8_t* data, const uint8_t* cw_status,
                             const uint16_t* crc_tab, dabhip_dabplus_sf* recs, int64_t* counters, hipStream_t stream)
{
  if (nsf > 0) dabplus_au_kernel<<<nsf, 64, 0, stream>>>(jobs, loc, maxv, nsub, data, cw_status, crc_tab, crc_tab + 256, recs, counters);
  return hipGetLastError();
}

hipError_t launch_dabplus_carry(const DabPlusFrames& fr, int nstreams, uint8_t* carry_next, hipStream_t stream)
{
  if (nstreams > 0) dabplus_carry_kernel<<<nstreams, 256, 0, stream>>>(fr, carry_next);
  return hipGetLastError();
}

}  // namespace dabhip
