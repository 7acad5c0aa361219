// k_edirx.hip — ETI frames out of EDI packets in device memory (AF packets, PFT fragments with or without RS(255,207)), for many streams at
// once.  dabhip.h (dabhip_edirx) has the rules; edirx_plan.hpp the same as pure functions; edirx.hpp the types.
//
//   parse    one thread per packet: its header checked against its length, the HCRC included (edirx_check_packet)
//   window   one lane per stream walks its packets' parsed headers through the window rule (edirx_window_step) on the stream's state, held
//            in LDS while it walks; the groups it touches and their fate go to fixed slots, so no order is raced for.  Then one workgroup:
//            the bases
//   gather   the carried bytes of the touched groups into the work buffer, then a wave per packet scatters its payload to its final place
//            (FEC: de-interleaved, byte j of fragment i to j f + i)
//   rs       the hot path: the words with erasures are listed; a wave per listed word: lane i owns syndrome i and coefficient i of the locator
//            and the evaluator, the locator grows by a factor (1 + X x) per erasure with a neighbour exchange, then a lane per erasure
//            evaluates Forney's quotient (first root alpha^0).  Log / antilog tables, the word and the logs of every polynomial lie in LDS,
//            so a sum of products is one independent table read per term; the erasure positions come from the group's mask of held fragments
//   frame    one workgroup per candidate: the AF packet in LDS, "AF" / LEN / the CRC-16 split over a wave, the TAG walk by one thread
//            (edirx_walk), the 6144 bytes of the ETI frame in LDS with both CRCs
//   emit     one lane per stream ranks its frames (counters, records); a workgroup per frame copies it to its place
//   carry    the groups still open keep their bytes
//
// No scalar-memory writes anywhere.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "edirx.hpp"

namespace dabhip {
namespace {

constexpr int kEti = DABHIP_ETI_BYTES;
constexpr int kEdirxWindowLanes = 16;

__device__ inline int slot0(const EdirxPush& p, int s) { return p.first[s] + s * p.depth; }

// the stream whose run [bases[2 s + which], bases[2 s + 2 + which]) holds x (x below the total)
__device__ inline int stream_of(const int64_t* bases, int nstreams, int which, int64_t x)
{
  int lo = 0, hi = nstreams - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bases[2 * mid + which] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(256) edirx_parse_kernel(EdirxPush p, EdirxHdr* hdr)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.npackets) return;
  const int64_t a = p.off[i];
  hdr[i] = edirx_check_packet(p.data + a, p.off[i + 1] - a);
}

struct WindowSink {
  EdirxMeta* meta;
  int32_t* fin;
  int stream, ntouched, ncand;
  __device__ void touch(EdirxGroup& g) { if (g.local < 0) g.local = ntouched++; }
  __device__ void joined(EdirxStream& st, int e) { touch(st.open[e]); }
  __device__ void put(const EdirxGroup& g, int status, int cand, int e)
  {
    EdirxMeta m;
    m.g = g;
    m.status = status;
    m.stream = stream;
    m.cand = cand;
    m.entry = e;
    meta[g.local] = m;
  }
  __device__ void finalise(EdirxStream& st, int e, bool ready)
  {
    EdirxGroup& g = st.open[e];
    touch(g);
    put(g, ready ? 1 : 2, ready ? ncand : -1, e);
    if (ready) fin[ncand++] = g.local;
  }
};

// kEdirxWindowLanes streams to a workgroup: each lane's state (1288 bytes) and counters lie in LDS while it walks, so a step's chain of
// dependent reads is LDS reads, and the next packet's header is loaded while this one is taken.
__global__ void __launch_bounds__(kEdirxWindowLanes) edirx_window_kernel(EdirxPush p, const EdirxHdr* hdr, EdirxStream* state, int64_t* counters, EdirxMeta* meta,
                                                                         int32_t* fin, int32_t* joined, int64_t* sums)
{
  __shared__ EdirxStream sh_st[kEdirxWindowLanes];
  __shared__ int64_t sh_cnt[kEdirxWindowLanes][kEdirxCntN];
  const int s = blockIdx.x * kEdirxWindowLanes + threadIdx.x;
  if (s >= p.nstreams) return;
  EdirxStream& st = sh_st[threadIdx.x];
  st = state[s];
  int64_t* cnt = sh_cnt[threadIdx.x];
  for (int i = 0; i < kEdirxCntN; ++i) cnt[i] = 0;
  const int first = p.first[s], n = p.npk[s], g0 = slot0(p, s);
  WindowSink sink = {meta + g0, fin + g0, s, 0, 0};
  for (int e = 0; e < p.depth; ++e) {
    st.open[e].local = -1;
    st.open[e].carried = st.open[e].used;
  }
  EdirxHdr h = {};
  if (n > 0) h = hdr[first];
  for (int i = 0; i < n; ++i) {
    EdirxHdr ahead = h;
    if (i + 1 < n) ahead = hdr[first + i + 1];
    const int e = edirx_window_step(st, p.depth, h, cnt, sink);
    joined[first + i] = e < 0 ? -1 : g0 + st.open[e].local;
    h = ahead;
  }
  if (p.flush == -1 || p.flush == s) edirx_flush(st, p.depth, cnt, sink);
  for (int e = 0; e < p.depth; ++e)
    if (st.open[e].used && st.open[e].local >= 0) sink.put(st.open[e], 0, -1, e);
  state[s] = st;
  for (int i = 0; i < kEdirxCntN; ++i) counters[static_cast<int64_t>(s) * kEdirxCntN + i] += cnt[i];
  sums[2 * s] = sink.ntouched;
  sums[2 * s + 1] = sink.ncand;
}

// one workgroup of 1024: the streams in contiguous runs, a block scan of the two sums -> the streams' bases, the totals behind them
__global__ void __launch_bounds__(1024) edirx_bases_kernel(int nstreams, const int64_t* sums, int64_t* bases)
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
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t x = t >= d ? sh[0][t - d] : 0, y = t >= d ? sh[1][t - d] : 0;
    __syncthreads();
    sh[0][t] += x;
    sh[1][t] += y;
    __syncthreads();
  }
  int64_t pp = sh[0][t] - np, q = sh[1][t] - nb;
  for (int i = a; i < b; ++i) {
    bases[2 * i] = pp;
    bases[2 * i + 1] = q;
    pp += sums[2 * i];
    q += sums[2 * i + 1];
  }
  if (t == 1023) {
    bases[2 * nstreams] = sh[0][1023];
    bases[2 * nstreams + 1] = sh[1][1023];
  }
}

// the meta slot of touched group x (a workgroup-uniform value)
__device__ inline int touched_slot(const EdirxPush& p, const int64_t* bases, int64_t x)
{
  const int s = stream_of(bases, p.nstreams, 0, x);
  return slot0(p, s) + static_cast<int>(x - bases[2 * s]);
}

__global__ void __launch_bounds__(256) edirx_carry_in_kernel(EdirxPush p, const EdirxMeta* meta, const int64_t* bases, const uint8_t* carry, uint8_t* work)
{
  const int64_t x = blockIdx.x;
  const EdirxMeta& m = meta[touched_slot(p, bases, x)];
  if (!m.g.carried) return;
  const uint4* src = reinterpret_cast<const uint4*>(carry + (static_cast<int64_t>(m.stream) * p.depth + m.entry) * kEdirxStride);
  uint4* dst = reinterpret_cast<uint4*>(work + x * kEdirxStride);
  for (int i = threadIdx.x; i < kEdirxStride / 16; i += 256) dst[i] = src[i];
}

__global__ void __launch_bounds__(256) edirx_scatter_kernel(EdirxPush p, const EdirxHdr* hdr, const EdirxMeta* meta, const int32_t* joined, const int64_t* bases,
                                                           uint8_t* work)
{
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (i >= p.npackets) return;
  const int slot = joined[i];
  if (slot < 0) return;
  const EdirxHdr h = hdr[i];
  const int s = meta[slot].stream;
  const int64_t x = bases[2 * s] + (slot - slot0(p, s));
  int at, step;
  edirx_place(h, &at, &step);                          // at + (plen - 1) step < kEdirxStride: the window rule's reach, or the tail
  const uint8_t* src = p.data + p.off[i] + h.head;
  uint8_t* dst = work + x * kEdirxStride + at;
  for (int j = l; j < h.plen; j += 64) dst[j * step] = src[j];
}

__global__ void __launch_bounds__(256) edirx_cand_kernel(EdirxPush p, int64_t ncand, const EdirxMeta* meta, const int32_t* fin, const int64_t* bases, EdirxCand* cands,
                                                         uint8_t* ers, int32_t* list, int32_t* nlist)
{
  // a thread per (candidate, word)
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t c = t >> 5;
  const int w = static_cast<int>(t & 31);
  if (c >= ncand) return;                              // whole waves: 32 words to a candidate, two candidates to a wave
  const int s = stream_of(bases, p.nstreams, 1, c);
  const int g0 = slot0(p, s);
  const int slot = g0 + fin[g0 + static_cast<int>(c - bases[2 * s + 1])];
  const EdirxGroup& g = meta[slot].g;
  if (w == 0) cands[c] = EdirxCand{slot, static_cast<int32_t>(bases[2 * s] + g.local)};
  int n = 0;
  if (g.kind == kEdirxPfFec && g.nrecv < g.fcount && w < g.fcount * g.plen / (g.rsk + kEdiRsP)) n = edirx_word_erasures(g.mask, g.fcount, g.rsk, w, nullptr);
  ers[t] = static_cast<uint8_t>(n);
  // one atomic add per wave: its lanes with a word to list take consecutive places
  const unsigned long long has = __ballot(n > 0);
  if (has == 0) return;
  const int lane = threadIdx.x & 63, leader = __ffsll(has) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(nlist, __popcll(has));
  base = __shfl(base, leader);
  if (n > 0) list[base + __popcll(has & ((1ull << lane) - 1))] = static_cast<int32_t>(t);
}

// ---- the erasure decoder --------------------------------------------------------------------------------------------------------------------
constexpr int kLogZero = 255;                          // "log" of 0 in the tables below: a term with it is masked out
struct RsShared {
  uint8_t exp[512];
  uint8_t log[256];
  uint8_t word[256];                                   // the 255 bytes of the code word, 0 at the erasures
  uint8_t lword[256];                                  // their logs
  uint8_t elog[kEdiRsP];                               // log of the erasures' locators X = alpha^(254 - place)
  uint16_t eat[kEdiRsP];                               // their places among the code word's bytes in the RS block
  uint8_t lsyn[kEdiRsP], llam[kEdiRsP + 1], lom[kEdiRsP], lval[kEdiRsP];    // logs of the syndromes, the locator, the evaluator, the values
};

// One wave per workgroup, so that a barrier is the wave's own.  Sums of products are taken term by term from logs kept in LDS (one table read
// per term, the terms independent of each other), not by Horner's chain of dependent reads; only the locator's growth is a chain.
__global__ void __launch_bounds__(64) edirx_rs_kernel(const EdirxMeta* meta, const EdirxCand* cands, const uint8_t* gf, const int32_t* list, const int32_t* nlist,
                                                      int32_t* rsfail, uint8_t* work)
{
  __shared__ RsShared sh;
  const int l = threadIdx.x;
  for (int i = l; i < 768; i += 64) (i < 512 ? sh.exp[i] : sh.log[i - 512]) = gf[i];
  const int total = *nlist;
  for (int idx = blockIdx.x; idx < total; idx += gridDim.x) {
    const int entry = list[idx], c = entry >> 5, w = entry & 31;
    const EdirxCand cand = cands[c];
    const EdirxGroup& g = meta[cand.slot].g;
    const int f = g.fcount, k = g.rsk, cw = k + kEdiRsP;
    const uint64_t mask[4] = {g.mask[0], g.mask[1], g.mask[2], g.mask[3]};
    uint8_t* block = work + static_cast<int64_t>(cand.work) * kEdirxStride + w * cw;
    __syncthreads();                                   // the tables; the previous word's reads
    for (int t = l; t < 256; t += 64) sh.word[t] = 0;
    __syncthreads();
    int ne = 0;
    for (int t0 = 0; t0 < cw; t0 += 64) {
      const int t = t0 + l;
      const bool have = t < cw;
      const bool erased = have && !edirx_held(mask, (w * cw + t) % f);
      const int place = edirx_cw_index(k, t);
      if (have && !erased) sh.word[place] = block[t];
      const unsigned long long bal = __ballot(erased);
      const int at = ne + __popcll(bal & ((1ull << l) - 1));
      if (erased && at < kEdiRsP) {
        sh.elog[at] = static_cast<uint8_t>(254 - place);
        sh.eat[at] = static_cast<uint16_t>(t);
      }
      ne += __popcll(bal);
    }
    if (ne > kEdiRsP) {                                // not in a ready group; nothing is written past the 48
      if (l == 0) rsfail[c] = 1;
      continue;
    }
    __syncthreads();
    for (int t = l; t < 256; t += 64) {
      const uint32_t v = sh.word[t];
      sh.lword[t] = v ? sh.log[v] : kLogZero;
    }
    __syncthreads();
    // syndrome i = sum of byte j times alpha^(i (254 - j)) over the data bytes and the parity bytes (the 207 - k bytes between are zero)
    const int i = l < kEdiRsP ? l : 0;
    uint32_t s = 0;
    {
      int e = i * 254 % 255;
      for (int j = 0; j < k; ++j) {
        const uint32_t lr = sh.lword[j], v = sh.exp[lr + e];
        s ^= lr == kLogZero ? 0 : v;
        e -= i;
        if (e < 0) e += 255;
      }
      e = i * (kEdiRsP - 1) % 255;
#pragma unroll 8
      for (int j = kEdiRsK; j < kEdiRsN; ++j) {
        const uint32_t lr = sh.lword[j], v = sh.exp[lr + e];
        s ^= lr == kLogZero ? 0 : v;
        e -= i;
        if (e < 0) e += 255;
      }
    }
    // the locator: lane i holds coefficient i
    uint32_t lam = l == 0;
    for (int e = 0; e < ne; ++e) {
      const uint32_t up = __shfl_up(lam, 1);
      if (l > 0 && up) lam ^= sh.exp[sh.log[up] + sh.elog[e]];
    }
    if (l < kEdiRsP) sh.lsyn[l] = static_cast<uint8_t>(s ? sh.log[s] : kLogZero);
    if (l <= kEdiRsP) sh.llam[l] = static_cast<uint8_t>(lam ? sh.log[lam] : kLogZero);
    __syncthreads();
    // the evaluator: coefficient i of S(x) lambda(x), i below the erasures' number
    uint32_t om = 0;
    for (int j = 0; j < ne; ++j) {
      const uint32_t a = sh.llam[j], b = sh.lsyn[j <= i ? i - j : 0], v = sh.exp[a + b];
      om ^= (j > i || a == kLogZero || b == kLogZero) ? 0 : v;
    }
    if (l < kEdiRsP) sh.lom[l] = static_cast<uint8_t>(l < ne && om ? sh.log[om] : kLogZero);
    __syncthreads();
    // Forney, a lane per erasure: e = X omega(1 / X) / lambda'(1 / X)
    uint32_t val = 0;
    const int xl = l < ne ? sh.elog[l] : 0;
    {
      const int inv = (255 - xl) % 255;
      uint32_t num = 0, den = 0;
      int pw = 0;                                      // log of (1 / X)^j
      for (int j = 0; j < ne; ++j) {
        const uint32_t a = sh.lom[j], va = sh.exp[a + pw];
        num ^= a == kLogZero ? 0 : va;
        const uint32_t b = sh.llam[j + 1], vb = sh.exp[b + pw];              // the derivative's term j, of the odd coefficient j + 1
        den ^= ((j & 1) || b == kLogZero) ? 0 : vb;
        pw += inv;
        if (pw >= 255) pw -= 255;
      }
      if (l < ne && num && den) val = sh.exp[(sh.log[num] + xl + 255 - sh.log[den]) % 255];
    }
    if (l < ne) {
      block[sh.eat[l]] = static_cast<uint8_t>(val);
      sh.lval[l] = static_cast<uint8_t>(val ? sh.log[val] : kLogZero);
    }
    __syncthreads();
    // the filled word's syndromes, by linearity: syndrome i + sum of e X^i
    for (int e = 0; e < ne; ++e) {
      const uint32_t a = sh.lval[e], v = sh.exp[a + i * sh.elog[e] % 255];
      s ^= a == kLogZero ? 0 : v;
    }
    if (__ballot(l < kEdiRsP && s != 0) != 0 && l == 0) rsfail[c] = 1;
  }
}

// ---- the frame ---------------------------------------------------------------------------------------------------------------------------------
__device__ inline uint32_t crc_step(const uint16_t* table, uint32_t reg, uint32_t b) { return ((reg << 8) & 0xFFFF) ^ table[(reg >> 8) ^ b]; }

// The complemented CRC-16 of n bytes (n >= 0) by one wave, the same value in every lane: lane i runs piece i from 0 through the table, the 64
// pieces of ceil(n / 64) bytes lying so that the last one ends at n; a prefix scan combines them (edi_plan.hpp); the start value 0xFFFF is
// shifted over all n bytes.
__device__ inline uint32_t wave_crc(const uint16_t* table, const uint8_t* p, int n, int l)
{
  const int piece = edi_crc_piece(n);
  const int e = n - (63 - l) * piece, a = e - piece > 0 ? e - piece : 0;
  uint32_t v = 0, mult = 1;
  for (int i = a; i < e; ++i) v = crc_step(table, v, p[i]);
  for (int i = 0; i < piece; ++i) mult = crc_step(table, mult, 0);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(v, d);
    if (l >= d) v ^= edi_crc_mulmod(static_cast<uint16_t>(up), static_cast<uint16_t>(mult));
    mult = edi_crc_mulmod(static_cast<uint16_t>(mult), static_cast<uint16_t>(mult));
  }
  v = __shfl(v, 63) ^ edi_crc_shift(0xFFFF, n);
  return ~v & 0xFFFF;
}

__global__ void __launch_bounds__(256) edirx_frame_kernel(const EdirxMeta* meta, const EdirxCand* cands, const uint8_t* ers, const int32_t* rsfail, const uint8_t* work,
                                                          uint8_t* candframes, EdirxVerdict* verdict)
{
  __shared__ alignas(16) uint8_t pk[kEdirxTail];
  __shared__ alignas(16) uint8_t fr[kEti];
  __shared__ uint16_t crc_t[256];
  __shared__ EdirxLayout lay;
  __shared__ int dst_at[kEdiMaxNst];
  __shared__ int status, mst_end;
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const EdirxCand cand = cands[c];
  const EdirxGroup& g = meta[cand.slot].g;
  const int kind = g.kind, f = g.fcount, plen = g.plen, k = g.rsk;
  EdirxVerdict v = {};
  if (kind == kEdirxPfFec) {
    const int nw = f * plen / (k + kEdiRsP);
    for (int i = 0; i < nw; ++i) {
      const int n = ers[c * 32 + i];
      v.words += n > 0;
      v.erasures += n;
    }
    if (rsfail[c]) {                                   // the whole workgroup
      v.status = 1;
      if (t == 0) verdict[c] = v;
      return;
    }
  }
  crc_t[t] = edi_crc_byte(0, static_cast<uint8_t>(t));
  const int len = edirx_af_bytes(g);                   // 1 .. kEdirxMaxPayload
  const uint8_t* block = work + static_cast<int64_t>(cand.work) * kEdirxStride;
  const int body = (f - 1) * plen;                     // PFT: what lies in front of the last fragment
  for (int i = t; i < len; i += 256) {
    int at = i;
    if (kind == kEdirxPfFec) at = i / k * (k + kEdiRsP) + i % k;
    else if (kind == kEdirxPf && f > 1 && i >= body) at = kEdirxTail + i - body;
    pk[i] = block[at];
  }
  __syncthreads();
  if (w == 0) {
    bool good = len >= kEdiAfOver && pk[0] == 'A' && pk[1] == 'F' && static_cast<int64_t>(edirx_get32(pk + 2)) + kEdiAfOver == len && (pk[8] & 0xF0) == 0x90 && pk[9] == 'T';
    if (good) good = wave_crc(crc_t, pk, len - 2, l) == edirx_get16(pk + len - 2);
    if (l == 0) {
      int st = good ? 0 : 2;
      if (good && edirx_walk(pk, len, lay)) st = 3;
      if (st == 0) {
        int at = edirx_eti_header(pk, lay, fr) + kEdiFic * lay.ficf;
        for (int e = 0; e < lay.nst; ++e) {
          dst_at[e] = at;
          at += 8 * lay.est_stl[e];
        }
        mst_end = at;
      }
      status = st;
    }
  }
  __syncthreads();
  v.status = status;
  if (status) {
    if (t == 0) verdict[c] = v;
    return;
  }
  const int mst0 = 12 + 4 * lay.nst;
  if (lay.ficf && t < kEdiFic) fr[mst0 + t] = pk[lay.fic_at + t];
  for (int e = w; e < lay.nst; e += 4) {
    const uint8_t* src = pk + lay.est_at[e] + 3;
    uint8_t* dst = fr + dst_at[e];
    for (int b = l; b < 8 * lay.est_stl[e]; b += 64) dst[b] = src[b];
  }
  for (int i = mst_end + 2 + t; i < kEti; i += 256) fr[i] = i < mst_end + 8 ? 0xFF : 0x55;
  __syncthreads();
  if (w == 0) {
    const uint32_t crc = wave_crc(crc_t, fr + mst0, mst_end - mst0, l);
    if (l == 0) edi_put16(fr + mst_end, crc);
  }
  __syncthreads();
  uint4* dst = reinterpret_cast<uint4*>(candframes + c * kEti);
  const uint4* src = reinterpret_cast<const uint4*>(fr);
  for (int i = t; i < kEti / 16; i += 256) dst[i] = src[i];
  if (t == 0) {
    v.items_ignored = lay.items_ignored;
    v.with_atst = lay.atstf;
    v.fcth = lay.fcth;
    v.fct = lay.fct;
    verdict[c] = v;
  }
}

__global__ void __launch_bounds__(64) edirx_rank_kernel(EdirxPush p, const EdirxMeta* meta, const EdirxCand* cands, const EdirxVerdict* verdict, const int64_t* bases,
                                                        int64_t* counters, int32_t* outmap, int32_t* nframes, dabhip_edirx_rec* recs)
{
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= p.nstreams) return;
  int64_t* cnt = counters + static_cast<int64_t>(s) * kEdirxCntN;
  const int64_t a = bases[2 * s + 1], b = bases[2 * s + 3];
  int64_t r = 0;
  for (int64_t c = a; c < b; ++c) {
    const EdirxVerdict v = verdict[c];
    if (v.status == 1) { ++cnt[kEdirxCntRsFailed]; continue; }
    cnt[kEdirxCntWordsFilled] += v.words;
    cnt[kEdirxCntErasuresFilled] += v.erasures;
    if (v.status == 2) { ++cnt[kEdirxCntCrcFailed]; continue; }
    if (v.status == 3) { ++cnt[kEdirxCntRefused]; continue; }
    const EdirxGroup& g = meta[cands[c].slot].g;
    dabhip_edirx_rec rec = {};
    rec.frame = cnt[kEdirxCntFrames] + r;
    rec.received = g.nrecv;
    rec.expected = g.fcount;
    rec.words_filled = v.words;
    rec.erasures_filled = v.erasures;
    rec.seq = static_cast<uint16_t>(g.seq);
    rec.fcth = static_cast<uint8_t>(v.fcth);
    rec.fct = static_cast<uint8_t>(v.fct);
    recs[a + r] = rec;
    outmap[a + r] = static_cast<int32_t>(c);
    cnt[kEdirxCntItemsIgnored] += v.items_ignored;
    cnt[kEdirxCntWithAtst] += v.with_atst;
    ++r;
  }
  cnt[kEdirxCntFrames] += r;
  nframes[s] = static_cast<int32_t>(r);
  for (int64_t o = a + r; o < b; ++o) outmap[o] = -1;
}

__global__ void __launch_bounds__(256) edirx_place_kernel(const int32_t* outmap, const uint8_t* candframes, uint8_t* out)
{
  const int64_t o = blockIdx.x;
  const int c = outmap[o];
  if (c < 0) return;
  const uint4* src = reinterpret_cast<const uint4*>(candframes + static_cast<int64_t>(c) * kEti);
  uint4* dst = reinterpret_cast<uint4*>(out + o * kEti);
  for (int i = threadIdx.x; i < kEti / 16; i += 256) dst[i] = src[i];
}

__global__ void __launch_bounds__(256) edirx_carry_out_kernel(EdirxPush p, const EdirxMeta* meta, const int64_t* bases, const uint8_t* work, uint8_t* carry)
{
  const int64_t x = blockIdx.x;
  const EdirxMeta& m = meta[touched_slot(p, bases, x)];
  if (m.status != 0) return;
  const uint4* src = reinterpret_cast<const uint4*>(work + x * kEdirxStride);
  uint4* dst = reinterpret_cast<uint4*>(carry + (static_cast<int64_t>(m.stream) * p.depth + m.entry) * kEdirxStride);
  for (int i = threadIdx.x; i < kEdirxStride / 16; i += 256) dst[i] = src[i];
}

}  // namespace

hipError_t launch_edirx_parse(const EdirxPush& p, EdirxHdr* hdr, hipStream_t stream)
{
  if (p.npackets > 0) edirx_parse_kernel<<<(p.npackets + 255) / 256, 256, 0, stream>>>(p, hdr);
  return hipGetLastError();
}

hipError_t launch_edirx_window(const EdirxPush& p, const EdirxHdr* hdr, EdirxStream* state, int64_t* counters, EdirxMeta* meta, int32_t* fin, int32_t* joined,
                               int64_t* sums, int64_t* bases, hipStream_t stream)
{
  edirx_window_kernel<<<(p.nstreams + kEdirxWindowLanes - 1) / kEdirxWindowLanes, kEdirxWindowLanes, 0, stream>>>(p, hdr, state, counters, meta, fin, joined, sums);
  edirx_bases_kernel<<<1, 1024, 0, stream>>>(p.nstreams, sums, bases);
  return hipGetLastError();
}

hipError_t launch_edirx_gather(const EdirxPush& p, int64_t ntouched, const EdirxHdr* hdr, const EdirxMeta* meta, const int32_t* joined, const int64_t* bases,
                               const uint8_t* carry, uint8_t* work, hipStream_t stream)
{
  if (ntouched <= 0) return hipGetLastError();
  const hipError_t e = hipMemsetAsync(work, 0, static_cast<size_t>(ntouched) * kEdirxStride, stream);
  if (e != hipSuccess) return e;
  edirx_carry_in_kernel<<<static_cast<unsigned>(ntouched), 256, 0, stream>>>(p, meta, bases, carry, work);
  if (p.npackets > 0) edirx_scatter_kernel<<<(p.npackets + 3) / 4, 256, 0, stream>>>(p, hdr, meta, joined, bases, work);
  return hipGetLastError();
}

hipError_t launch_edirx_rs(const EdirxPush& p, int64_t ncand, const EdirxMeta* meta, const int32_t* fin, const int64_t* bases, const uint8_t* gf, EdirxCand* cands,
                           uint8_t* ers, int32_t* list, int32_t* nlist, int32_t* rsfail, uint8_t* work, hipStream_t stream)
{
  if (ncand <= 0) return hipGetLastError();
  hipError_t e = hipMemsetAsync(nlist, 0, sizeof(int32_t), stream);
  if (e == hipSuccess) e = hipMemsetAsync(rsfail, 0, sizeof(int32_t) * static_cast<size_t>(ncand), stream);
  if (e != hipSuccess) return e;
  const int64_t words = ncand * kEdirxMaxWords;
  edirx_cand_kernel<<<static_cast<unsigned>((words + 255) / 256), 256, 0, stream>>>(p, ncand, meta, fin, bases, cands, ers, list, nlist);
  // workgroups that stay: each loads the tables once and goes round over the list
  const unsigned grid = static_cast<unsigned>(words < 16384 ? words : 16384);
  edirx_rs_kernel<<<grid, 64, 0, stream>>>(meta, cands, gf, list, nlist, rsfail, work);
  return hipGetLastError();
}

hipError_t launch_edirx_frame(int64_t ncand, const EdirxMeta* meta, const EdirxCand* cands, const uint8_t* ers, const int32_t* rsfail, const uint8_t* work,
                              uint8_t* candframes, EdirxVerdict* verdict, hipStream_t stream)
{
  if (ncand > 0) edirx_frame_kernel<<<static_cast<unsigned>(ncand), 256, 0, stream>>>(meta, cands, ers, rsfail, work, candframes, verdict);
  return hipGetLastError();
}

hipError_t launch_edirx_emit(const EdirxPush& p, int64_t ncand, const EdirxMeta* meta, const EdirxCand* cands, const EdirxVerdict* verdict, const int64_t* bases,
                             const uint8_t* candframes, int64_t* counters, int32_t* outmap, int32_t* nframes, dabhip_edirx_rec* recs, uint8_t* out, hipStream_t stream)
{
  edirx_rank_kernel<<<(p.nstreams + 63) / 64, 64, 0, stream>>>(p, meta, cands, verdict, bases, counters, outmap, nframes, recs);
  if (ncand > 0) edirx_place_kernel<<<static_cast<unsigned>(ncand), 256, 0, stream>>>(outmap, candframes, out);
  return hipGetLastError();
}

hipError_t launch_edirx_carry(const EdirxPush& p, int64_t ntouched, const EdirxMeta* meta, const int64_t* bases, const uint8_t* work, uint8_t* carry, hipStream_t stream)
{
  if (ntouched > 0) edirx_carry_out_kernel<<<static_cast<unsigned>(ntouched), 256, 0, stream>>>(p, meta, bases, work, carry);
  return hipGetLastError();
}

}  // namespace dabhip
