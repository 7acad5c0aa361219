// k_edi.hip — EDI packets out of ETI frames in device memory (ETSI TS 102 693 over TS 102 821: TAG items in an AF packet, PFT fragments, RS(255,207)),
// for many streams at once.  dabhip.h (dabhip_edi) has the rules; edi_plan.hpp the same as pure functions; edi.hpp the types.
//
//   plan      one thread per (stream, new frame): the frame's header, whether it is accepted, l and every size of PFT (edi_plan.hpp)
//   scan      one wave per stream, 64 frames per step by wave prefix sums: the rank among the accepted frames (SEQ), the FCT wraps (FCTH), the
//             frame's first packet and byte among its stream's; the stream's state and counters.  Then one workgroup: the streams' bases
//   assemble  one workgroup per accepted frame: the AF packet in LDS from the frame, byte by byte (so aligned or not); the CRC-16 in parallel
//             (64 contiguous pieces, combined by powers of x^8 mod the polynomial in a wave scan); dwords out to the work buffer
//   rs        the hot path: a wave per frame, a lane per chunk.  The frame's packet comes through LDS (contiguous dwords in), the 48-byte
//             remainder lies in twelve registers, a step is a shift by one byte and an XOR with one 48-byte row of the feedback table in LDS
//   fragment  one workgroup per accepted frame: the PF headers with their HCRC, then a thread per output byte: the copy (modes 0, 1) or the
//             interleaving gather out of the packet and the parity (mode 2); a thread per packet writes its record
//
// No scalar-memory writes anywhere.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "edi.hpp"

namespace dabhip {
namespace {

constexpr int kEti = DABHIP_ETI_BYTES;
constexpr int kWorkWords = kEdiWorkStride / 4;

__global__ void __launch_bounds__(256) edi_plan_kernel(EtiFrames fr, EdiConfig cfg, int nstreams, int maxv, EdiFrame* out)
{
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(nstreams) * maxv) return;
  const int s = static_cast<int>(t / maxv), v = static_cast<int>(t % maxv);
  if (v >= fr.nnew[s]) return;
  const int64_t g = fr.base[s] + v;
  const EdiHead h = edi_parse(fr.frames + g * kEti);
  EdiFrame x = {};
  x.stream = s;
  x.valid = h.valid;
  if (h.valid) {
    x.l = h.l;
    x.p = edi_plan(h.l, cfg.mode, cfg.recover, cfg.max_frag);
    x.fcth = h.fct;                                    // the scan reads FCT and FICF here and leaves FCTH
    x.seq = h.ficf;
  }
  out[g] = x;
}

// inclusive prefix sum over the 64 lanes of a wave
template <class T>
__device__ inline T wave_scan(T x, int l)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d);
    if (l >= d) x += y;
  }
  return x;
}

__global__ void __launch_bounds__(64 * kEdiScanWaves) edi_scan_kernel(EtiFrames fr, EdiConfig cfg, int nstreams, EdiFrame* frames, EdiState* state, int64_t* counters,
                                                                      int64_t* sums)
{
  const int s = blockIdx.x * kEdiScanWaves + (threadIdx.x >> 6);
  if (s >= nstreams) return;
  const int l = threadIdx.x & 63;
  const int nnew = fr.nnew[s];
  EdiFrame* mine = frames + fr.base[s];
  EdiState st = state[s];
  // the same in all 64 lanes
  int64_t bytes = 0, accepted = 0, nofic = 0, chunks = 0;
  int packets = 0;
  for (int c0 = 0; c0 < nnew; c0 += 64) {
    const int v = c0 + l;
    const bool have = v < nnew;
    EdiFrame x = {};
    if (have) x = mine[v];
    const bool acc = have && x.valid;
    const int fct = x.fcth, ficf = x.seq;
    const unsigned long long mask = __ballot(acc);
    // the accepted frame in front of this one: the nearest accepted lane below, else the one carried in
    const unsigned long long below = mask & ((1ull << l) - 1);
    const int prev_lane = below ? 63 - __builtin_clzll(below) : 0;
    int prev_fct = __shfl(fct, prev_lane);
    bool have_prev = below != 0;
    if (!have_prev) {
      prev_fct = st.last_fct;
      have_prev = st.started != 0;
    }
    const int wrap = acc && have_prev && fct < prev_fct;
    const int f = acc ? x.p.f : 0;
    const int nbytes = acc ? edi_out_bytes(x.p, cfg.mode, x.l) : 0;
    const int rank = wave_scan(static_cast<int>(acc), l), wraps = wave_scan(wrap, l), pk = wave_scan(f, l);
    const int64_t by = wave_scan(static_cast<int64_t>(nbytes), l);
    if (have) {
      x.number = st.frames + v;
      if (acc) {
        x.seq = (st.seq_next + rank - 1) & 0xFFFF;
        x.fcth = (st.fcth + wraps) % kEdiFcthMod;
        x.pkt_local = packets + pk - f;
        x.byte_local = bytes + by - nbytes;
      }
      mine[v] = x;
    }
    const int nacc = __popcll(mask);
    if (nacc) {
      const int last = 63 - __builtin_clzll(mask);
      st.last_fct = __shfl(fct, last);
      st.fcth = (st.fcth + __shfl(wraps, 63)) % kEdiFcthMod;
      st.seq_next = (st.seq_next + nacc) & 0xFFFF;
      st.started = 1;
    }
    accepted += nacc;
    nofic += __popcll(__ballot(acc && !ficf));
    chunks += __shfl(wave_scan(acc ? x.p.c : 0, l), 63);
    packets += __shfl(pk, 63);
    bytes += __shfl(by, 63);
  }
  if (l != 0) return;
  st.frames += nnew;
  state[s] = st;
  int64_t* cnt = counters + static_cast<int64_t>(s) * kEdiCntN;
  cnt[kEdiCntFrames] += nnew;
  cnt[kEdiCntSkipped] += nnew - accepted;
  cnt[kEdiCntNoFic] += nofic;
  cnt[kEdiCntPackets] += packets;
  cnt[kEdiCntBytes] += bytes;
  cnt[kEdiCntChunks] += chunks;
  sums[2 * s] = packets;
  sums[2 * s + 1] = bytes;
}

// one workgroup of 1024: the streams in contiguous runs, a block scan of their packets and bytes -> the streams' bases, the totals behind them
__global__ void __launch_bounds__(1024) edi_bases_kernel(int nstreams, const int64_t* sums, int64_t* bases)
{
  __shared__ int64_t sh[2][1024];
  const int t = threadIdx.x;
  const int run = (nstreams + 1023) / 1024;
  const int a = t * run < nstreams ? t * run : nstreams, b = a + run < nstreams ? a + run : nstreams;
  int64_t np = 0, nb = 0;
  for (int i = a; i < b; ++i) {
    np += sums[2 * i];
    nb += sums[2 * i + 1];
  }
  sh[0][t] = np;
  sh[1][t] = nb;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {                 // inclusive Hillis-Steele scan
    const int64_t x = t >= d ? sh[0][t - d] : 0, y = t >= d ? sh[1][t - d] : 0;
    __syncthreads();
    sh[0][t] += x;
    sh[1][t] += y;
    __syncthreads();
  }
  int64_t p = sh[0][t] - np, q = sh[1][t] - nb;
  for (int i = a; i < b; ++i) {
    bases[2 * i] = p;
    bases[2 * i + 1] = q;
    p += sums[2 * i];
    q += sums[2 * i + 1];
  }
  if (t == 1023) {
    bases[2 * nstreams] = sh[0][1023];
    bases[2 * nstreams + 1] = sh[1][1023];
  }
}

// one byte into the CRC register through the 256-entry table of edi_crc_byte(0, .)
__device__ inline uint32_t crc_step(const uint16_t* table, uint32_t reg, uint32_t b) { return ((reg << 8) & 0xFFFF) ^ table[(reg >> 8) ^ b]; }

__global__ void __launch_bounds__(256) edi_assemble_kernel(EtiFrames fr, const EdiFrame* frames, uint8_t* work)
{
  __shared__ uint32_t pk_w[kWorkWords];
  __shared__ int item_at[kEdiMaxNst], src_at[kEdiMaxNst], item_stl[kEdiMaxNst];
  __shared__ uint16_t crc_t[256];
  const int64_t g = blockIdx.x;
  const EdiFrame x = frames[g];
  if (!x.valid) return;                                // the whole workgroup
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  crc_t[t] = edi_crc_byte(0, static_cast<uint8_t>(t));
  uint8_t* pk = reinterpret_cast<uint8_t*>(pk_w);
  const uint8_t* f = fr.frames + g * kEti;
  const EdiHead h = edi_head(f);
  const int nwords = (x.l + kEdiMaxChunks + 15) / 16 * 4;                // the packet and the zeros behind it that the chunks may reach: <= kWorkWords
  for (int i = t; i < nwords; i += 256) pk_w[i] = 0;
  __syncthreads();
  const int items0 = kEdiAfHead + kEdiPtrItem + kEdiDetiHead + kEdiFic * h.ficf;
  const int mst0 = 12 + 4 * h.nst;
  if (w == 0) {                                        // the est items' places by a prefix sum, and their 11 bytes
    const int stl = l < h.nst ? edi_stc_stl(f, l) : 0;
    const int before = wave_scan(stl, l) - stl;
    if (l < h.nst) {
      item_at[l] = items0 + kEdiEstHead * l + 8 * before;
      src_at[l] = mst0 + kEdiFic * h.ficf + 8 * before;
      item_stl[l] = stl;
      edi_put_est(pk + item_at[l], l + 1, f + 8 + 4 * l);
    }
  } else if (w == 1) {
    if (l == 0) {
      edi_put_af_head(pk, static_cast<uint32_t>(x.l - kEdiAfOver), static_cast<uint32_t>(x.seq));
      edi_put_ptr(pk + kEdiAfHead);
      edi_put_deti(pk + kEdiAfHead + kEdiPtrItem, h, x.fcth);
    }
  } else if (h.ficf) {
    const int i = t - 128;
    if (i < kEdiFic) pk[kEdiAfHead + kEdiPtrItem + kEdiDetiHead + i] = f[mst0 + i];
  }
  __syncthreads();
  for (int e = w; e < h.nst; e += 4) {                 // a wave per entry: its 8 STL bytes
    const int n = 8 * item_stl[e];
    const uint8_t* src = f + src_at[e];
    uint8_t* dst = pk + item_at[e] + kEdiEstHead;
    for (int b = l; b < n; b += 64) dst[b] = src[b];
  }
  __syncthreads();
  // The CRC over the n = l - 2 bytes in front of it, by wave 0 (a workgroup's cost is its wave instructions, and the combine below has as many
  // for one wave as for four): lane i runs piece i from 0 through the table, the 64 pieces of ceil(n / 64) bytes lying so that the last one
  // ends at n (the first ones are short or empty).  Then every shift is by whole pieces, and a wave prefix scan combines them: at distance d
  // a lane takes its neighbour's register times x^(8 piece d), a multiplier that is the same in all lanes and squares from step to step.
  // The start value 0xFFFF is the complement of the first two bytes.
  const int n = x.l - 2;
  if (w == 0) {
    const int piece = edi_crc_piece(n);
    const int e = n - (63 - l) * piece, a = e - piece > 0 ? e - piece : 0;
    uint32_t v = 0, mult = 1;
    for (int i = a; i < e; ++i) v = crc_step(crc_t, v, i < 2 ? pk[i] ^ 0xFFu : pk[i]);
    for (int i = 0; i < piece; ++i) mult = crc_step(crc_t, mult, 0);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(v, d);
      if (l >= d) v ^= edi_crc_mulmod(static_cast<uint16_t>(up), static_cast<uint16_t>(mult));
      mult = edi_crc_mulmod(static_cast<uint16_t>(mult), static_cast<uint16_t>(mult));
    }
    if (l == 63) edi_put16(pk + n, ~v & 0xFFFF);
  }
  __syncthreads();
  uint32_t* dst = reinterpret_cast<uint32_t*>(work + g * kEdiWorkStride);
  for (int i = t; i < nwords; i += 256) dst[i] = pk_w[i];
}

// The remainder's 48 bytes in twelve dwords, byte 0 (the coefficient of x^47) the low byte of r[0].  One step: the feedback byte is the message
// byte plus byte 0; the remainder moves up by one byte and takes the row of the table.
__global__ void __launch_bounds__(64 * kEdiRsWaves) edi_rs_kernel(int64_t nframes, const EdiFrame* frames, const uint8_t* table_global, const uint8_t* work,
                                                                  uint8_t* parity)
{
  __shared__ alignas(16) uint32_t table_w[256 * kEdiRsP / 4];
  __shared__ alignas(16) uint32_t pk_w[kEdiRsFrames][kWorkWords];
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(table_global);
    for (int i = threadIdx.x; i < 256 * kEdiRsP / 4; i += blockDim.x) table_w[i] = src[i];
  }
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  // every wave of the workgroup goes round the same number of times, so that the barriers meet
  for (int64_t g0 = static_cast<int64_t>(blockIdx.x) * kEdiRsFrames; g0 < nframes; g0 += static_cast<int64_t>(gridDim.x) * kEdiRsFrames) {
    const int64_t g = g0 + w;
    EdiFrame x = {};
    if (g < nframes) x = frames[g];
    const int c = x.valid ? x.p.c : 0, k = x.p.k;
    __syncthreads();                                   // the previous round's reads of pk_w are done
    if (c > 0) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(work + g * kEdiWorkStride);
      const int nwords = (c * k + 3) / 4;              // <= l + 31 bytes: inside what assemble wrote
      for (int i = l; i < nwords; i += 64) pk_w[w][i] = src[i];
    }
    __syncthreads();
    const int ci = l;
    if (ci >= c) continue;
    uint32_t r[12] = {0};
    const uint8_t* chunk = reinterpret_cast<const uint8_t*>(pk_w[w]) + ci * k;
    for (int i = 0; i < kEdiRsK; ++i) {
      const uint32_t d = i < k ? chunk[i] : 0;
      const uint32_t v = (d ^ r[0]) & 0xFF;
      const uint4* row = reinterpret_cast<const uint4*>(table_w + 12 * v);
      const uint4 t0 = row[0], t1 = row[1], t2 = row[2];
#pragma unroll
      for (int j = 0; j < 11; ++j) r[j] = (r[j] >> 8) | (r[j + 1] << 24);
      r[11] >>= 8;
      r[0] ^= t0.x; r[1] ^= t0.y; r[2] ^= t0.z; r[3] ^= t0.w;
      r[4] ^= t1.x; r[5] ^= t1.y; r[6] ^= t1.z; r[7] ^= t1.w;
      r[8] ^= t2.x; r[9] ^= t2.y; r[10] ^= t2.z; r[11] ^= t2.w;
    }
    uint4* out = reinterpret_cast<uint4*>(parity + (g * kEdiMaxChunks + ci) * kEdiRsP);
    out[0] = uint4{r[0], r[1], r[2], r[3]};
    out[1] = uint4{r[4], r[5], r[6], r[7]};
    out[2] = uint4{r[8], r[9], r[10], r[11]};
  }
}

__global__ void __launch_bounds__(256) edi_fragment_kernel(EdiConfig cfg, const EdiFrame* frames, const int64_t* bases, const uint8_t* work, const uint8_t* parity,
                                                          uint8_t* out, dabhip_edi_rec* recs)
{
  __shared__ uint8_t head[kEdiMaxFrags][16];
  const int64_t g = blockIdx.x;
  const EdiFrame x = frames[g];
  if (!x.valid) return;                                // the whole workgroup
  const int t = threadIdx.x;
  const EdiPlan p = x.p;
  const int mode = cfg.mode;
  const int hb = edi_pf_head_bytes(mode);
  for (int i = t; i < p.f; i += 256) {                 // a thread per packet: its header and its record
    if (mode) edi_put_pf(head[i], static_cast<uint32_t>(x.seq), static_cast<uint32_t>(i), static_cast<uint32_t>(p.f), mode == 2,
                         static_cast<uint32_t>(edi_packet_bytes(p, mode, x.l, i) - hb), static_cast<uint32_t>(p.k), static_cast<uint32_t>(p.z));
    dabhip_edi_rec r = {};
    r.offset = x.byte_local + edi_packet_offset(p, mode, i);
    r.frame = x.number;
    r.length = edi_packet_bytes(p, mode, x.l, i);
    r.findex = i;
    r.fcount = p.f;
    r.seq = static_cast<uint16_t>(x.seq);
    recs[bases[2 * x.stream] + x.pkt_local + i] = r;
  }
  __syncthreads();
  const uint8_t* pk = work + g * kEdiWorkStride;
  uint8_t* dst = out + bases[2 * x.stream + 1] + x.byte_local;
  const int n = edi_out_bytes(p, mode, x.l);
  if (mode == 0) {
    for (int o = t; o < n; o += 256) dst[o] = pk[o];
    return;
  }
  const int stride = hb + p.s;
  const uint8_t* par = parity + g * kEdiMaxChunks * kEdiRsP;
  const int cw = p.k + kEdiRsP;
  for (int o = t; o < n; o += 256) {
    const int i = o / stride, j = o % stride - hb;
    uint8_t v;
    if (j < 0) {
      v = head[i][j + hb];
    } else if (mode == 1) {
      v = pk[i * p.s + j];
    } else {
      const int b = edi_block_index(p, i, j);
      const int ci = b / cw, q = b % cw;
      v = b >= p.B ? 0 : q < p.k ? pk[ci * p.k + q] : par[ci * kEdiRsP + q - p.k];
    }
    dst[o] = v;
  }
}

}  // namespace

hipError_t launch_edi_plan(const EtiFrames& fr, EdiConfig cfg, int nstreams, int maxv, EdiFrame* out, hipStream_t stream)
{
  const int64_t n = static_cast<int64_t>(nstreams) * maxv;
  if (n > 0) edi_plan_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, stream>>>(fr, cfg, nstreams, maxv, out);
  return hipGetLastError();
}

hipError_t launch_edi_scan(const EtiFrames& fr, EdiConfig cfg, int nstreams, EdiFrame* frames, EdiState* state, int64_t* counters, int64_t* sums, int64_t* bases,
                           hipStream_t stream)
{
  edi_scan_kernel<<<(nstreams + kEdiScanWaves - 1) / kEdiScanWaves, 64 * kEdiScanWaves, 0, stream>>>(fr, cfg, nstreams, frames, state, counters, sums);
  edi_bases_kernel<<<1, 1024, 0, stream>>>(nstreams, sums, bases);
  return hipGetLastError();
}

hipError_t launch_edi_assemble(const EtiFrames& fr, int64_t nframes, const EdiFrame* frames, uint8_t* work, hipStream_t stream)
{
  if (nframes > 0) edi_assemble_kernel<<<static_cast<unsigned>(nframes), 256, 0, stream>>>(fr, frames, work);
  return hipGetLastError();
}

hipError_t launch_edi_rs(int64_t nframes, const EdiFrame* frames, const uint8_t* table, const uint8_t* work, uint8_t* parity, hipStream_t stream)
{
  if (nframes <= 0) return hipGetLastError();
  // workgroups that stay: each loads the table once and goes round over the frames, kEdiRsFrames at a time
  const int64_t groups = (nframes + kEdiRsFrames - 1) / kEdiRsFrames;
  const unsigned grid = static_cast<unsigned>(groups < 2048 ? groups : 2048);
  edi_rs_kernel<<<grid, 64 * kEdiRsWaves, 0, stream>>>(nframes, frames, table, work, parity);
  return hipGetLastError();
}

hipError_t launch_edi_fragment(EdiConfig cfg, int64_t nframes, const EdiFrame* frames, const int64_t* bases, const uint8_t* work, const uint8_t* parity, uint8_t* out,
                               dabhip_edi_rec* recs, hipStream_t stream)
{
  if (nframes > 0) edi_fragment_kernel<<<static_cast<unsigned>(nframes), 256, 0, stream>>>(cfg, frames, bases, work, parity, out, recs);
  return hipGetLastError();
}

}  // namespace dabhip
