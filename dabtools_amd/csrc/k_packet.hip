// k_packet.hip — packet-mode data out of ETI frames in device memory (ETSI EN 300 401 clauses 5.3.2, 5.3.5), for many streams and sub-channels
// at once.  dabhip.h (dabhip_packet) has the rules; packet.hpp the sizes, the types and the sync rule's text.
//
//   locate   one thread per (stream, new frame): FC / STC header, where each requested SubChId sits and its STL
//   sync     one lane per (stream, sub-channel), taking that lane's new cells in order from the state of the previous push: the lane's virtual
//            cell numbering (carried cells, then the frames' cells), the FEC frame sync, and the units (FEC frames, or ETI frames without FEC)
//            into fixed slots per lane, so the order is deterministic without atomics
//   scan     one workgroup: prefix sums over the lanes' unit and buffer-cell counts; jobs: one thread per slot -> the push's unit list
//   gather   one thread per cell of every unit: its 24 bytes into the contiguous cell buffer (103 cells per FEC frame)
//   rs       one lane per code word, 12 per FEC frame side by side: the 16 syndromes by Horner through LDS tables (the hot path); then, for the
//            code words with errors only, Berlekamp-Massey, Chien search, Forney and the check by syndromes in a second kernel, which
//            corrects the cell buffer in place.  The code's tables, its Horner step and its solver are rs_code.hpp's, shared with
//            k_dabplus.hip and k_ts.hip; the addressing (fec_byte_offset) is this stage's
//   cand     one lane per data cell: header check and CRC of the packet that would start there
//   walk     one lane per unit over the candidates' flags: a record per cell (length 0: no packet starts here), the counters
//   carry    one workgroup per lane: its unconsumed cells (at most 102), for the next push
//
// No scalar-memory writes anywhere.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "eti_locate.hpp"
#include "kernels.hpp"
#include "packet.hpp"
#include "rs_code.hpp"

namespace dabhip {
namespace {

constexpr int kEti = DABHIP_ETI_BYTES;
constexpr int kCarryBytes = kPkCarry * kPkCell;

__global__ void __launch_bounds__(256) packet_locate_kernel(EtiFrames fr, const int32_t* subch, int nsub, int nstreams, int maxv, PacketLoc* loc)
{
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(nstreams) * maxv) return;
  const int s = static_cast<int>(t / maxv), v = static_cast<int>(t % maxv);
  if (v >= fr.nnew[s]) return;
  const uint8_t* f = fr.frames + (fr.base[s] + v) * kEti;
  PacketLoc* out = loc + t * nsub;
  for (int q = 0; q < nsub; ++q) out[q] = PacketLoc{nullptr, 0, 0};
  eti_stc_walk(f, subch, nsub, [out](int q, int stl, bool fits, const uint8_t* p) {
    out[q].stl = stl;
    if (fits && stl > 0 && stl % 3 == 0) out[q].ptr = p;
  });
}

__device__ inline PacketLoc& loc_at(PacketLoc* loc, int stream, int v, int sub, int maxv, int nsub)
{
  return loc[(static_cast<int64_t>(stream) * maxv + v) * nsub + sub];
}

// virtual cell u of a lane: a carried cell (u < ncar), else a cell of the last frame whose cell0 is at or below u (frames that gave no cells
// share the cell0 of the frame after them, so the last one is the one that has the cell)
__device__ inline const uint8_t* cell_ptr(const PacketLoc* loc, int stream, int sub, int maxv, int nsub, int nnew, const uint8_t* carry, int lane, int ncar, int u)
{
  if (u < ncar) return carry + static_cast<int64_t>(lane) * kCarryBytes + u * kPkCell;
  int lo = 0, hi = nnew - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (loc[(static_cast<int64_t>(stream) * maxv + mid) * nsub + sub].cell0 <= u) lo = mid; else hi = mid - 1;
  }
  const PacketLoc& l = loc[(static_cast<int64_t>(stream) * maxv + lo) * nsub + sub];
  return l.ptr + (u - l.cell0) * kPkCell;
}

__global__ void __launch_bounds__(64) packet_sync_kernel(EtiFrames fr, int nstreams, int nsub, int maxv, const uint8_t* fec, PacketLoc* loc, PacketSync* sync,
                                                         const uint8_t* carry, PacketSlot* slots, int cap, int* nunits, int* lane_buf, int* ncar_in, int* ncar_out,
                                                         int* lo_out, int64_t* counters, int* totals)
{
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nstreams * nsub) return;
  const int s = lane / nsub, q = lane % nsub;
  const bool with_fec = fec[q] != 0;
  const int nnew = fr.nnew[s];
  PacketWalkState w;
  w.st = sync[lane];
  w.lo = 0;
  w.skipped = w.frames = w.misses = w.losses = 0;
  const int ncar = w.st.ncar;
  const int64_t cell_base = w.st.next_cell - ncar;   // the index since creation of virtual cell 0
  ncar_in[lane] = ncar;
  int n = 0, nbuf = 0;
  PacketSlot* mine = slots + static_cast<int64_t>(lane) * cap;
  const auto emit = [&](int32_t u0, int flags) {
    if (n < cap) mine[n] = PacketSlot{u0, static_cast<int16_t>(kPkDataCells), static_cast<int16_t>(flags), cell_base + u0};
    ++n;
    nbuf += kPkFrameCells;
  };
  int nv = ncar;
  for (int v = 0; v < nnew; ++v) {
    PacketLoc& l = loc_at(loc, s, v, q, maxv, nsub);
    const bool valid = l.ptr != nullptr;
    if (!valid || (w.st.stl != 0 && l.stl != w.st.stl)) packet_break(w, nv);
    l.cell0 = nv;
    if (!valid) continue;
    w.st.stl = l.stl;
    const int cells = l.stl / 3;
    if (!with_fec) {                                 // the unit is this frame; nothing is carried
      if (n < cap) mine[n] = PacketSlot{nv, static_cast<int16_t>(cells), 0, cell_base + nv};
      ++n;
      ++w.frames;
      nbuf += cells;
      nv += cells;
      w.lo = nv;
      continue;
    }
    const uint8_t* p = l.ptr;
    for (int c0 = 0; c0 < cells; c0 += 8) {          // the headers of 8 cells at a time: their loads are in flight together
      int hdr[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = c0 + i < cells ? c0 + i : cells - 1;
        hdr[i] = fec_counter(p[c * kPkCell], p[c * kPkCell + 1]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (c0 + i >= cells) break;
        if (packet_feed(w, nv, hdr[i], emit)) {
          // the third miss: search again from the cell after the frame's first (rare: these cells are found the slow way)
          for (int u = w.lo + 1; u <= nv; ++u) {
            const uint8_t* h = u >= l.cell0 ? p + (u - l.cell0) * kPkCell : cell_ptr(loc, s, q, maxv, nsub, v + 1, carry, lane, ncar, u);
            packet_feed(w, u, fec_counter(h[0], h[1]), emit);
          }
        }
        ++nv;
      }
    }
  }
  packet_push_end(w, nv);
  w.st.next_cell = cell_base + nv;
  sync[lane] = w.st;
  ncar_out[lane] = w.st.ncar;
  lo_out[lane] = w.lo;
  nunits[lane] = n <= cap ? n : 0;                   // (cap holds every unit a push can give: packet.cpp)
  lane_buf[lane] = n <= cap ? nbuf : 0;
  if (n > cap) totals[3] = 1;                        // never, by that bound; if ever, the push fails instead of losing the lane's units
  int64_t* cnt = counters + static_cast<int64_t>(lane) * kPkCntN;
  cnt[kPkCntFrames] += w.frames;
  cnt[kPkCntMisses] += w.misses;
  cnt[kPkCntSyncLosses] += w.losses;
  cnt[kPkCntSkipped] += w.skipped;
}

// one workgroup of 1024: lanes split in contiguous chunks, a block scan of (units, buffer cells) per lane -> the lanes' bases
__global__ void __launch_bounds__(1024) packet_scan_kernel(int nlanes, const int* nunits, const int* lane_buf, int* lane_unit_base, int* lane_buf_base, int* totals)
{
  __shared__ int sh_u[1024], sh_c[1024];
  const int t = threadIdx.x;
  const int chunk = (nlanes + 1023) / 1024;
  const int a = t * chunk < nlanes ? t * chunk : nlanes, b = a + chunk < nlanes ? a + chunk : nlanes;
  int nu = 0, nc = 0;
  for (int l = a; l < b; ++l) {
    nu += nunits[l];
    nc += lane_buf[l];
  }
  sh_u[t] = nu;
  sh_c[t] = nc;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {               // inclusive Hillis-Steele scan
    const int x = t >= d ? sh_u[t - d] : 0, y = t >= d ? sh_c[t - d] : 0;
    __syncthreads();
    sh_u[t] += x;
    sh_c[t] += y;
    __syncthreads();
  }
  int u = sh_u[t] - nu, c = sh_c[t] - nc;
  for (int l = a; l < b; ++l) {
    lane_unit_base[l] = u;
    lane_buf_base[l] = c;
    u += nunits[l];
    c += lane_buf[l];
  }
  if (t == 1023) {
    lane_unit_base[nlanes] = sh_u[1023];
    lane_buf_base[nlanes] = sh_c[1023];
    totals[0] = sh_u[1023];
    totals[1] = sh_c[1023];
  }
}

// one lane per (stream, sub-channel): its slots into the push's unit list, in (stream, sub-channel, time) order, with their places in the cell buffer
__global__ void __launch_bounds__(64) packet_jobs_kernel(int nlanes, const PacketSlot* slots, int cap, const int* nunits, const int* lane_unit_base,
                                                         const int* lane_buf_base, PacketUnit* units)
{
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= nlanes) return;
  int buf = lane_buf_base[lane];
  PacketUnit* out = units + lane_unit_base[lane];
  const int n = nunits[lane];
  for (int i = 0; i < n; ++i) {
    const PacketSlot sl = slots[static_cast<int64_t>(lane) * cap + i];
    const int nb = (sl.flags & (DABHIP_PACKET_FROM_FEC | DABHIP_PACKET_FROM_MISS)) ? kPkFrameCells : sl.ncells;
    out[i] = PacketUnit{lane, sl.u0, sl.ncells, nb, sl.flags, buf, sl.cell_index};
    buf += nb;
  }
}

// the unit of buffer cell c: the last with buf0 <= c (no unit is empty)
__device__ inline int unit_of(const PacketUnit* units, int nunits, int c)
{
  int lo = 0, hi = nunits - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (units[mid].buf0 <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(256) packet_gather_kernel(EtiFrames fr, const PacketUnit* units, const int* totals, const PacketLoc* loc, int maxv, int nsub,
                                                           const uint8_t* carry, const int* ncar_in, uint8_t* cells)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= totals[1]) return;
  const PacketUnit un = units[unit_of(units, totals[0], c)];
  const int s = un.lane / nsub, q = un.lane % nsub;
  const uint8_t* src = cell_ptr(loc, s, q, maxv, nsub, fr.nnew[s], carry, un.lane, ncar_in[un.lane], un.u0 + (c - un.buf0));
  uint32_t* dst = reinterpret_cast<uint32_t*>(cells + static_cast<int64_t>(c) * kPkCell);
  if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
#pragma unroll
    for (int i = 0; i < kPkCell / 4; ++i) dst[i] = reinterpret_cast<const uint32_t*>(src)[i];
  } else {
#pragma unroll
    for (int i = 0; i < kPkCell / 4; ++i) dst[i] = src[4 * i] | (src[4 * i + 1] << 8) | (src[4 * i + 2] << 16) | (static_cast<uint32_t>(src[4 * i + 3]) << 24);
  }
}

// The hot path: syndromes S_i = r(alpha^i) by Horner, byte 0 first.  Thread t is code word t % 12 of unit t / 12, so the 12 lanes of a frame read
// 12 contiguous bytes per column.  A clean code word (all syndromes zero) is done here; the others leave their syndromes for the decode kernel,
// which keeps this loop's register count low.  Units that are not RS-decoded frames get status 0.
__global__ void __launch_bounds__(256) packet_syndrome_kernel(const PacketUnit* units, const int* totals, const uint8_t* gf_global, const uint8_t* cells,
                                                             uint8_t* cw_status, uint32_t* syn)
{
  __shared__ uint32_t mul_w[kPkRoots * 64];          // GfRs::mul
  const uint32_t* src = reinterpret_cast<const uint32_t*>(gf_global);
  for (int i = threadIdx.x; i < kPkRoots * 64; i += blockDim.x) mul_w[i] = src[i];
  __syncthreads();
  const uint8_t* mul = reinterpret_cast<const uint8_t*>(mul_w);
  const int cw = blockIdx.x * blockDim.x + threadIdx.x;
  if (cw >= totals[0] * kPkRows) return;
  const PacketUnit un = units[cw / kPkRows];
  if (!(un.flags & DABHIP_PACKET_FROM_FEC)) {
    cw_status[cw] = 0;
    return;
  }
  const int r = cw % kPkRows;
  const uint8_t* z = cells + static_cast<int64_t>(un.buf0) * kPkCell;
  uint32_t S[kPkRoots] = {0};
#pragma unroll 4
  for (int c = 0; c < kPkN; ++c) {
    const uint8_t b = z[fec_byte_offset(r, c)];
    rs_horner(mul, S, b);
  }
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < kPkRoots; ++i) any |= S[i];
  cw_status[cw] = any ? 0xfe : 0;
  if (any) rs_pack(S, syn + static_cast<int64_t>(cw) * 4);
}

// The error path of the code words the syndrome kernel left (status 0xfe): the table bytes corrected in place in the cell buffer, status = symbols
// corrected or 0xff.  A workgroup without such a code word returns before it loads the tables.
__global__ void __launch_bounds__(256) packet_decode_kernel(const PacketUnit* units, const int* totals, const uint8_t* gf_global, uint8_t* cells,
                                                           uint8_t* cw_status, const uint32_t* syn)
{
  __shared__ GfRs<kPkRoots> g;
  const int cw = blockIdx.x * blockDim.x + threadIdx.x;
  const bool need = cw < totals[0] * kPkRows && cw_status[cw] == 0xfe;
  if (!__syncthreads_or(need)) return;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(gf_global);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&g);
    for (int i = threadIdx.x; i < static_cast<int>(sizeof(g) / 4); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  if (!need) return;
  const PacketUnit un = units[cw / kPkRows];
  const int r = cw % kPkRows;
  uint8_t S8[kPkRoots];
  const uint32_t* o = syn + static_cast<int64_t>(cw) * 4;
#pragma unroll
  for (int i = 0; i < kPkRoots; ++i) S8[i] = static_cast<uint8_t>(o[i >> 2] >> (8 * (i & 3)));
  int pos[kPkT] = {0};
  uint8_t val[kPkT] = {0};
  const int n = rs_solve<kPkN, kPkRoots, kPkT>(g, S8, pos, val);
  if (n < 0) {
    cw_status[cw] = 0xff;
    return;
  }
  uint8_t* z = cells + static_cast<int64_t>(un.buf0) * kPkCell;
  for (int i = 0; i < n; ++i)
    if (pos[i] < kPkK) z[fec_byte_offset(r, pos[i])] ^= val[i];
  cw_status[cw] = static_cast<uint8_t>(n);
}

// One lane per buffer cell: the length (1..4) of the packet that would start there if the walk may take it, else 0.
__global__ void __launch_bounds__(256) packet_cand_kernel(const PacketUnit* units, const int* totals, const uint16_t* crc_tab_global, const uint8_t* cells, uint8_t* cand)
{
  __shared__ uint16_t crc_tab[256];
  crc_tab[threadIdx.x] = crc_tab_global[threadIdx.x];
  __syncthreads();
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= totals[1]) return;
  const PacketUnit un = units[unit_of(units, totals[0], c)];
  const int k = c - un.buf0;
  const uint8_t* p = cells + static_cast<int64_t>(c) * kPkCell;
  const int L = (p[0] >> 6) + 1;
  uint8_t out = 0;
  if (k + L <= un.ncells && (p[2] & 0x7f) <= kPkCell * L - 5) {
    const int len = kPkCell * L - 2;
    uint32_t crc = 0xffff;
    for (int i = 0; i < len; ++i) crc = (crc_tab[(p[i] ^ (crc >> 8)) & 0xff] ^ (crc << 8)) & 0xffff;
    if ((crc ^ 0xffff) == static_cast<uint32_t>((p[len] << 8) | p[len + 1])) out = static_cast<uint8_t>(L);
  }
  cand[c] = out;
}

// One lane per unit: the walk over the candidates, a record for every cell the unit holds, the unit's counters to its lane.
__global__ void __launch_bounds__(64) packet_walk_kernel(const PacketUnit* units, const int* totals, const uint8_t* cells, const uint8_t* cand, const uint8_t* cw_status,
                                                        dabhip_packet_rec* recs, int64_t* counters, int* npackets)
{
  const int ui = blockIdx.x * blockDim.x + threadIdx.x;
  if (ui >= totals[0]) return;
  const PacketUnit un = units[ui];
  int bad = 0, taken = 0;
  int k = 0;
  while (k < un.ncells) {
    const int c = un.buf0 + k;
    const int L = cand[c];
    dabhip_packet_rec r = {};
    if (!L) {
      ++bad;
      recs[c] = r;
      ++k;
      continue;
    }
    const uint8_t* p = cells + static_cast<int64_t>(c) * kPkCell;
    r.cell = un.cell_index + k;
    r.address = static_cast<uint16_t>(((p[0] & 3) << 8) | p[1]);
    r.length = static_cast<uint8_t>(L);
    r.continuity = (p[0] >> 4) & 3;
    r.first_last = (p[0] >> 2) & 3;
    r.command = p[2] >> 7;
    r.useful_length = p[2] & 0x7f;
    r.flags = static_cast<uint8_t>(un.flags);
    recs[c] = r;
    const dabhip_packet_rec none = {};
    for (int i = 1; i < L; ++i) recs[c + i] = none;
    ++taken;
    k += L;
  }
  const dabhip_packet_rec none = {};
  for (; k < un.nbuf; ++k) recs[un.buf0 + k] = none;
  int fixed = 0, failed = 0;
  if (un.flags & DABHIP_PACKET_FROM_FEC)
    for (int r = 0; r < kPkRows; ++r) {
      const uint8_t st = cw_status[ui * kPkRows + r];
      if (st == 0xff) ++failed; else fixed += st;
    }
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters + static_cast<int64_t>(un.lane) * kPkCntN);
  atomicAdd(cnt + kPkCntBadCells, static_cast<unsigned long long>(bad));
  atomicAdd(cnt + kPkCntPackets, static_cast<unsigned long long>(taken));
  atomicAdd(cnt + kPkCntRsCorrected, static_cast<unsigned long long>(fixed));
  atomicAdd(cnt + kPkCntRsFailed, static_cast<unsigned long long>(failed));
  atomicAdd(npackets, taken);
}

// a lane's unconsumed cells (virtual cells lo .. lo + ncar_out - 1) into the other carry buffer
__global__ void __launch_bounds__(128) packet_carry_kernel(EtiFrames fr, const PacketLoc* loc, int maxv, int nsub, const uint8_t* carry, const int* ncar_in,
                                                          const int* ncar_out, const int* lo, uint8_t* carry_next)
{
  const int lane = blockIdx.x, i = threadIdx.x;
  if (i >= ncar_out[lane]) return;
  const int s = lane / nsub, q = lane % nsub;
  const uint8_t* src = cell_ptr(loc, s, q, maxv, nsub, fr.nnew[s], carry, lane, ncar_in[lane], lo[lane] + i);
  uint8_t* dst = carry_next + static_cast<int64_t>(lane) * kCarryBytes + i * kPkCell;
  for (int b = 0; b < kPkCell; ++b) dst[b] = src[b];
}

}  // namespace

hipError_t launch_packet_locate(const EtiFrames& fr, const int32_t* subch, int nsub, int nstreams, int maxv, PacketLoc* loc, hipStream_t stream)
{
  const int64_t n = static_cast<int64_t>(nstreams) * maxv;
  if (n > 0) packet_locate_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, stream>>>(fr, subch, nsub, nstreams, maxv, loc);
  return hipGetLastError();
}

hipError_t launch_packet_sync(const EtiFrames& fr, int nstreams, int nsub, int maxv, const uint8_t* fec, PacketLoc* loc, PacketSync* sync, const uint8_t* carry,
                              PacketSlot* slots, int cap, int* nunits, int* lane_buf, int* ncar_in, int* ncar_out, int* lo, int64_t* counters, PacketUnit* units,
                              int* lane_unit_base, int* lane_buf_base, int* totals, hipStream_t stream)
{
  const int nlanes = nstreams * nsub;
  packet_sync_kernel<<<(nlanes + 63) / 64, 64, 0, stream>>>(fr, nstreams, nsub, maxv, fec, loc, sync, carry, slots, cap, nunits, lane_buf, ncar_in, ncar_out, lo, counters, totals);
  packet_scan_kernel<<<1, 1024, 0, stream>>>(nlanes, nunits, lane_buf, lane_unit_base, lane_buf_base, totals);
  packet_jobs_kernel<<<(nlanes + 63) / 64, 64, 0, stream>>>(nlanes, slots, cap, nunits, lane_unit_base, lane_buf_base, units);
  return hipGetLastError();
}

hipError_t launch_packet_gather(const EtiFrames& fr, const PacketUnit* units, const int* totals, int ncells, const PacketLoc* loc, int maxv, int nsub,
                                const uint8_t* carry, const int* ncar_in, uint8_t* cells, hipStream_t stream)
{
  if (ncells > 0) packet_gather_kernel<<<(ncells + 255) / 256, 256, 0, stream>>>(fr, units, totals, loc, maxv, nsub, carry, ncar_in, cells);
  return hipGetLastError();
}

hipError_t launch_packet_rs(const PacketUnit* units, const int* totals, int nunits, const uint8_t* gf_tables, uint8_t* cells, uint8_t* cw_status, uint32_t* syn,
                            hipStream_t stream)
{
  const int64_t ncw = static_cast<int64_t>(nunits) * kPkRows;
  if (ncw <= 0) return hipSuccess;
  const unsigned blocks = static_cast<unsigned>((ncw + 255) / 256);
  packet_syndrome_kernel<<<blocks, 256, 0, stream>>>(units, totals, gf_tables, cells, cw_status, syn);
  packet_decode_kernel<<<blocks, 256, 0, stream>>>(units, totals, gf_tables, cells, cw_status, syn);
  return hipGetLastError();
}

hipError_t launch_packet_cand(const PacketUnit* units, const int* totals, int ncells, const uint16_t* crc_tab, const uint8_t* cells, uint8_t* cand, hipStream_t stream)
{
  if (ncells > 0) packet_cand_kernel<<<(ncells + 255) / 256, 256, 0, stream>>>(units, totals, crc_tab, cells, cand);
  return hipGetLastError();
}

hipError_t launch_packet_walk(const PacketUnit* units, const int* totals, int nunits, const uint8_t* cells, const uint8_t* cand, const uint8_t* cw_status,
                              dabhip_packet_rec* recs, int64_t* counters, int* npackets, hipStream_t stream)
{
  if (nunits > 0) packet_walk_kernel<<<(nunits + 63) / 64, 64, 0, stream>>>(units, totals, cells, cand, cw_status, recs, counters, npackets);
  return hipGetLastError();
}

hipError_t launch_packet_carry(const EtiFrames& fr, int nlanes, const PacketLoc* loc, int maxv, int nsub, const uint8_t* carry, const int* ncar_in,
                               const int* ncar_out, const int* lo, uint8_t* carry_next, hipStream_t stream)
{
  if (nlanes > 0) packet_carry_kernel<<<nlanes, 128, 0, stream>>>(fr, loc, maxv, nsub, carry, ncar_in, ncar_out, lo, carry_next);
  return hipGetLastError();
}

}  // namespace dabhip
