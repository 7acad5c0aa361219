// vit_soft_lanes.hpp — the SOFT-decision decoder with 2^NL lanes per code word (NL = 2: four lanes; NL = 1: two lanes), opt-in (decoder_form.hpp: soft_lanes).
//
// Included by k_decode.hip inside its anonymous namespace, after vit_common.hpp and vit_four_lanes.hpp, whose lane-bit rotation, compaction numbering, exchange through
// quad_perm and re-pairing it reuses unchanged (namespace multi).  What soft values change, all of it run on the CPU first
// (tools/models/multilane_soft_model.py, held against oracle/or_soft.c by the CPU suite):
//   * the lane form's soft scale: metrics x16 with FOUR tag bits (MetricScale<4>: kBase 8192, re-base every 32 steps), so a block is 4 steps, every
//     re-pairing clears the tags, and the rotation (period 6 steps against 4) has THREE variants of a block, v = block index mod 3: lane places
//     (3, 5), (1, 3), (5, 1) at its start.  Two blocks make one unit of 8 steps -- the de-puncturing's unit -- in three variants as well.
//   * records: a block leaves one tag nibble per state, 2^(3 - NL) words per lane (register R -> word R >> 2, byte 2 (R & 1) + half, high nibble for
//     R & 2: survivor_record's packing inside the lane); the two half-records of a unit go out together, one 16-byte store per lane and 8 steps at
//     NL = 2 (words: half 0, half 0, half 1, half 1), two at NL = 1 (store j = half j) -- the hard form's volume and dec_base layout
//     (worklist.hpp sizes the buffer by steps alone, whatever the form).
//   * branch metrics without per-lane tables: the eight packed words W(c) (c < 4: the sum of the two SoftLut rows; W(c ^ 7) = kAll - W(c)) are
//     INDEXED by c ^ g, g = the lane's code offset, with one v_cndmask per word and lane bit below place 5 (the id bits are wave-constant masks).
//     The other way, flipping the signs of the received values on the bits of cw4(g) before the table read, is no XOR on 4-bit two's complement:
//     it takes a clamp of -8 to -7 (which build_soft_lut does inside the table, so a flipped -8 would read the -7 row where +7 is needed), a
//     nibble-wise negate with blocked carries and the split of the index again, ~10 VALU per step and a special case; the selects are at most 8 per
//     lane bit, 0 for the bit at place 5, and exact by construction: every lane reads the lane form's rows for the values as received.
//   * at an exchange step over id bit i the lanes with that bit set own the HIGH predecessor: their own operand takes the untagged words and the
//     partner's the tagged ones (the hard form's address ^ 1024; here the tag is added after the select, to A or to B).
// Input: each lane of a code word repeats the lane form's fifo arithmetic on the code word's row (RowInput<4>::take_soft).
// Per step and lane at NL = 2: 24 add / max (butterflies) + 8 (words) + 8 (tags) + at most 16 selects.
// Resources and occupancy: the kernel's comment below.

namespace softmulti {

using multi::Lane;
constexpr uint32_t kAll = static_cast<uint32_t>(56 << kMetricShift) * 0x00010001u;
__host__ __device__ constexpr int hard_variant(int v) { return (2 * v) % 3; }      // multi's helpers count t = 8 kV + kS: the same t mod 6 as 4 v + kS

// W(c) <- W(c ^ kG) in the lanes where `set` holds.  (A pack, not a loop over c: with a loop the optimiser folds the selects of two array elements into
// one load at a selected index before it unrolls, and every word becomes an eight-way compare-and-select chain.)
template <int kG, int... kC>
__device__ __forceinline__ void offset_words(bool set, uint32_t (&W)[8], std::integer_sequence<int, kC...>)
{
  const uint32_t X[8] = {(set ? W[kC ^ kG] : W[kC])...};
  ((W[kC] = X[kC]), ...);
}
template <int kG>
__device__ __forceinline__ void offset_words(bool set, uint32_t (&W)[8])
{
  offset_words<kG>(set, W, std::make_integer_sequence<int, 8>{});
}

template <int NL, int kVar, int kS, int... kQ>
__device__ __forceinline__ void butterflies(const uint32_t (&A)[8], const uint32_t (&B)[8], const pk16 (&p)[Lane<NL>::kRegs], pk16 (&n)[Lane<NL>::kRegs],
                                            std::integer_sequence<int, kQ...>)
{
  (multi::one_butterfly<NL, hard_variant(kVar), kS, kQ>(p, n, A, B), ...);
}

// one step of block variant kVar: nib16 = the step's four received 4-bit values (not received: zero nibbles)
template <int NL, int kVar, int kS>
__device__ __forceinline__ void step(uint32_t nib16, const SoftLut* lut, unsigned id, const pk16 (&p)[Lane<NL>::kRegs], pk16 (&n)[Lane<NL>::kRegs])
{
  constexpr int t = 4 * kVar + kS, i5 = multi::at_five<NL>(t);
  constexpr uint32_t tag = 0x00010001u << kS;
  const uint4 ta = lut->a[kS][(nib16 & 15u) | ((nib16 >> 8) & 0xf0u)], tb = lut->b[kS][(nib16 >> 4) & 0xffu];
  uint32_t W[8];
  W[0] = ta.x + tb.x;
  W[1] = ta.y + tb.y;
  W[2] = ta.z + tb.z;
  W[3] = ta.w + tb.w;
#pragma unroll
  for (int c = 0; c < 4; ++c) W[c ^ 7] = kAll - W[c];
  constexpr int L0 = multi::place(0, t), L1 = multi::place(1, t);
  if constexpr (L0 < 5) offset_words<branch_code3(2u << L0)>((id & 1u) != 0, W);
  if constexpr (NL > 1 && L1 < 5) offset_words<branch_code3(2u << L1)>((id & 2u) != 0, W);
  uint32_t A[8], B[8];
  if constexpr (i5 >= 0) {
    const bool high = ((id >> i5) & 1u) != 0;
    const uint32_t tag_a = high ? 0u : tag, tag_b = high ? tag : 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      A[c] = W[c] + tag_a;
      B[c] = W[c] + tag_b;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      A[c] = W[c] + tag;
      B[c] = W[c];
    }
  }
  constexpr int count = i5 >= 0 ? Lane<NL>::kRegs : Lane<NL>::kRegs / 2;
  butterflies<NL, kVar, kS>(A, B, p, n, std::make_integer_sequence<int, count>{});
}

// parked pairs -> pairs (k, k ^ 1) in the layout after block variant kVar, tag nibbles cleared
template <int NL, int kVar>
__device__ __forceinline__ void repair(const pk16 (&n)[Lane<NL>::kRegs], pk16 (&p)[Lane<NL>::kRegs])
{
  multi::repair<NL, false, 4 * (kVar + 1)>(n, p);
#pragma unroll
  for (int r = 0; r < Lane<NL>::kRegs; ++r) p[r] = as_pk(as_u32(p[r]) & 0xfff0fff0u);
}

// a lane's half-record: the tag nibbles of its registers
template <int NL>
__device__ __forceinline__ void pack(const pk16 (&n)[Lane<NL>::kRegs], uint32_t (&d)[Lane<NL>::kRegs / 4])
{
#pragma unroll
  for (int i = 0; i < Lane<NL>::kRegs / 4; ++i) {
    const uint32_t pa = __builtin_amdgcn_perm(as_u32(n[4 * i + 1]), as_u32(n[4 * i]), 0x06040200u);
    const uint32_t pb = __builtin_amdgcn_perm(as_u32(n[4 * i + 3]), as_u32(n[4 * i + 2]), 0x06040200u);
    d[i] = (pa & 0x0f0f0f0fu) | ((pb << 4) & 0xf0f0f0f0u);
  }
}

template <int NL, int kVar>
__device__ __forceinline__ void block(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, const SoftLut* lut, unsigned id, pk16 (&pm)[Lane<NL>::kRegs],
                                      pk16 (&pn)[Lane<NL>::kRegs], pk16 (&pl4)[Lane<NL>::kRegs], uint32_t (&d)[Lane<NL>::kRegs / 4])
{
  step<NL, kVar, 0>(x0, lut, id, pm, pn);
  step<NL, kVar, 1>(x1, lut, id, pn, pm);
  step<NL, kVar, 2>(x2, lut, id, pm, pn);
  step<NL, kVar, 3>(x3, lut, id, pn, pl4);
  pack<NL>(pl4, d);
  repair<NL, kVar>(pl4, pm);
}
// the last r = 1..3 steps of a code word: the half-record is only read for state 0 (lane 0, low half of register 0 in every layout)
template <int NL, int kVar>
__device__ __forceinline__ void block_tail(uint32_t x0, uint32_t x1, uint32_t x2, int r, const SoftLut* lut, unsigned id, pk16 (&pm)[Lane<NL>::kRegs],
                                           pk16 (&pn)[Lane<NL>::kRegs], uint32_t (&d)[Lane<NL>::kRegs / 4])
{
  step<NL, kVar, 0>(x0, lut, id, pm, pn);
  if (r == 1) { pack<NL>(pn, d); return; }
  step<NL, kVar, 1>(x1, lut, id, pn, pm);
  if (r == 2) { pack<NL>(pm, d); return; }
  step<NL, kVar, 2>(x2, lut, id, pm, pn);
  pack<NL>(pn, d);
}

// a unit of 8 steps = blocks 2 u, 2 u + 1 (variants (2 kU) % 3 and (2 kU + 1) % 3); left = steps of the code word from the unit's first on.  As in the lane
// form a code word ends in the unit's second block or at a block's end (every plan: 32 x blocks + 6 steps).
template <int NL, int kU>
__device__ __forceinline__ void unit(const uint32_t (&x)[8], int left, const SoftLut* lut, unsigned id, pk16 (&pm)[Lane<NL>::kRegs], pk16 (&pn)[Lane<NL>::kRegs],
                                     pk16 (&pl4)[Lane<NL>::kRegs], uint32_t (&h0)[Lane<NL>::kRegs / 4], uint32_t (&h1)[Lane<NL>::kRegs / 4])
{
  constexpr int v0 = (2 * kU) % 3, v1 = (2 * kU + 1) % 3;
  // left = 1..3 here would run no step and leave a tail nibble that chain_back reads at zero: no plan gets there.
  // make_codeword_plan (worklist.hpp) makes whole output bytes, out_bytes = (nsteps - 6) / 8, from 32 x blocks + 6 steps, so a code word's last unit
  // starts with 6 steps left; a plan of another length needs a block_tail for the first half here (tools/models/multilane_soft_model.py asserts
  // nsteps % 8 in {0, 4, 5, 6, 7} for the same reason)
  if (left >= 4) block<NL, v0>(x[0], x[1], x[2], x[3], lut, id, pm, pn, pl4, h0);
  if (left >= 8) block<NL, v1>(x[4], x[5], x[6], x[7], lut, id, pm, pn, pl4, h1);
  else if (left > 4) block_tail<NL, v1>(x[4], x[5], x[6], left - 4, lut, id, pm, pn, h1);
}

// dword idx (0..15) of four fetched 16-byte parts: uint4 idx >> 2, component idx & 3 (the barriers keep the selects in registers, see in_vgpr)
__device__ __forceinline__ uint32_t pick_word(const uint4 (&q)[4], unsigned idx)
{
  uint32_t d[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t lo = (idx & 1u) ? in_vgpr(q[u].y) : in_vgpr(q[u].x), hi = (idx & 1u) ? in_vgpr(q[u].w) : in_vgpr(q[u].z);
    d[u] = (idx & 2u) ? hi : lo;
  }
  return (idx & 8u) ? ((idx & 4u) ? d[3] : d[2]) : ((idx & 4u) ? d[1] : d[0]);
}

// chain back over the lanes' half-records, in one lane per code word (multi::chain_back's scheme: the whole records of four units per memory round
// trip).  cw_rec = the record base of the code word's lane 0; lane l's store j of unit u at cw_rec[256 u + 64 j + l].  The state's nibble is found by
// inverting the compaction numbering of the layout at the block's end: lane places (3, 5), (1, 3), (5, 1) for (block + 1) mod 3 = 0, 1, 2, pair bit 4.
template <int NL>
__device__ __forceinline__ void chain_back(const uint4* cw_rec, int nsteps, const uint32_t* __restrict__ prbs_words, uint32_t* dst)
{
  constexpr int kLanes = 1 << NL, kVec = Lane<NL>::kRegs / 8, kHalfWords = Lane<NL>::kRegs / 4;
  ChainOut o{prbs_words, dst};
  const int nfull = nsteps >> 2, r = nsteps & 3;           // whole blocks of 4 steps; block b = half b & 1 of unit b >> 1
  if (r) {                                                 // state 0's nibble: lane 0, word 0 of the half-record, nibble 0
    const uint4 q = rec_load(cw_rec + static_cast<size_t>(nfull >> 1) * 256 + (NL == 1 ? 64 * (nfull & 1) : 0));
    o.consume<4>((NL == 2 && (nfull & 1) ? q.z : q.x) & 15u, 4 * nfull, r - 1);
  }
  int m3 = nfull % 3;                                      // (block + 1) mod 3 of the block in hand
  for (int top = (nfull - 1) >> 1; top >= 0; top -= 4) {
    uint4 q[4][4];                                         // [unit top - k][lane * kVec + j]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint4* at = cw_rec + static_cast<size_t>(max(top - k, 0)) * 256;
#pragma unroll
      for (int l = 0; l < kLanes; ++l)
#pragma unroll
        for (int j = 0; j < kVec; ++j) q[k][l * kVec + j] = rec_load(at + 64 * j + l);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int u = top - k;
      if (u < 0) break;
#pragma unroll
      for (int h = 1; h >= 0; --h) {
        const int b = 2 * u + h;
        if (b >= nfull || b < 1) continue;                 // block 0 (steps 0..3) only flushes the encoder's initial zeros
        using multi::place;
        const unsigned L0 = m3 == 0 ? place(0, 0) : m3 == 1 ? place(0, 4) : place(0, 8), L1 = m3 == 0 ? place(1, 0) : m3 == 1 ? place(1, 4) : place(1, 8);
        unsigned removed = (1u << 4) | (1u << L0), lane = (o.state >> L0) & 1u;
        if (NL == 2) {
          removed |= 1u << L1;
          lane |= ((o.state >> L1) & 1u) << 1;
        }
        const unsigned P = register_of(o.state, removed), half = (o.state >> 4) & 1u, shift = 8u * (2u * (P & 1u) + half) + 4u * ((P >> 1) & 1u);
        const unsigned idx = lane * (2 * kHalfWords) + static_cast<unsigned>(h) * kHalfWords + (P >> 2);      // word of the unit's 16
        o.consume<4>((pick_word(q[k], idx) >> shift) & 15u, 4 * b, 3);
        m3 = m3 == 0 ? 2 : m3 - 1;
      }
    }
  }
}

}  // namespace softmulti

// the fused soft decoder (vit_common.hpp's front and output) with 2^NL lanes per code word: 2^NL waves per group of 64 code words.
// LDS: the lane form's SoftLut, 32 KB per workgroup.  As compiled for gfx950 (-Rpass-analysis=kernel-resource-usage): NL = 2: 83 VGPRs, no scratch, no
// spills, occupancy 5 waves per SIMD -- five workgroups per CU, which is also what 5 x 32 KB = 160 KB of LDS admits (the launch bound asks for four);
// NL = 1: 115 VGPRs, no scratch, no spills, occupancy 4 waves per SIMD (registers: 512 / 115), four workgroups = 128 KB of LDS.
template <int NL>
__global__ __launch_bounds__(256, NL == 2 ? 4 : 2) void viterbi_soft_lanes_kernel(const WaveGroup* __restrict__ groups, int ngroups, const int* __restrict__ job_ids,
                                                                                  const CodewordPlan* __restrict__ plans, const uint32_t* __restrict__ grouped,
                                                                                  int row_words, uint2* __restrict__ decisions,
                                                                                  const uint32_t* __restrict__ prbs_words, uint8_t* __restrict__ out,
                                                                                  int record_stride)
{
  constexpr int kRegs = multi::Lane<NL>::kRegs, kLanes = 1 << NL, kVec = kRegs / 8, kHalfWords = kRegs / 4;
  __shared__ __attribute__((aligned(16))) unsigned char lut_raw[sizeof(SoftLut)];
  SoftLut* lut = reinterpret_cast<SoftLut*>(lut_raw);
  build_soft_lut(lut);
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(4 * blockIdx.x + (threadIdx.x >> 6));
  const int g = w >> NL, part = w & (kLanes - 1);
  if (g >= ngroups) return;
  const WaveGroup grp = groups[g];
  const CodewordPlan* plan = plans + grp.plan;
  const int nsteps = grp.nsteps;
  const unsigned id = lane & (kLanes - 1);
  const int cw = (64 >> NL) * part + (lane >> NL);           // this lane's code word within the group
  uint4* my_rec = reinterpret_cast<uint4*>(decisions + grp.dec_base * 64) + 64 * kVec * part + lane;
  RowInput<4> in(grouped, row_words, grp.first >> 6, plan->start_bit, cw);
  pk16 pm[kRegs], pn[kRegs], pl4[kRegs];
#pragma unroll
  for (int r = 0; r < kRegs; ++r) pm[r] = as_pk(0u);         // (init_metrics, written out: through the function the NL = 1 kernel takes 116 VGPRs, not 115)
  pm[0] = as_pk(id ? 0u : MetricScale<4>::kBase);            // state 0: lane 0, register 0, low half
  int t = 0, v = 0;                                          // v = unit index mod 3: the unit's variant
  for (int seg = 0; seg < 5; ++seg) {
    const Segment s(*plan, seg);
    for (int u = 0; u < s.units; ++u) {
      uint32_t x[8];
      in.take_soft(s.counts, x);
      if (t < nsteps) {
        uint32_t h0[kHalfWords] = {}, h1[kHalfWords] = {};
        const int left = nsteps - t;
        if (v == 0) softmulti::unit<NL, 0>(x, left, lut, id, pm, pn, pl4, h0, h1);
        else if (v == 1) softmulti::unit<NL, 1>(x, left, lut, id, pm, pn, pl4, h0, h1);
        else softmulti::unit<NL, 2>(x, left, lut, id, pm, pn, pl4, h0, h1);
        uint4* rec = my_rec + static_cast<size_t>(t >> 3) * 256;
        if constexpr (NL == 2) {
          rec_store(rec, h0[0], h0[1], h1[0], h1[1]);
        } else {
          rec_store(rec, h0[0], h0[1], h0[2], h0[3]);
          rec_store(rec + 64, h1[0], h1[1], h1[2], h1[3]);
        }
      }
      t += 8;
      v = v == 2 ? 0 : v + 1;
      if ((t & (MetricScale<4>::kRebaseSteps - 1)) == 0 && t < nsteps) rebase<kLanes>(pm, MetricScale<4>::kBase);
    }
  }
  if (id == 0 && cw < grp.count)
    softmulti::chain_back<NL>(my_rec, nsteps, prbs_words, output_words(job_ids, grp.first + cw, out, record_stride, plan->out_offset));
}
