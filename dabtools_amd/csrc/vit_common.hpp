// vit_common.hpp — what the lane forms of the fused decoder share: the front of a code word (its received words, the walk over its puncturing
// segments, its output record), the chain-back's walk and output, and start and re-base of the metrics.
//
// Included by k_decode.hip inside its anonymous namespace, ahead of the first decoder and of vit_two_lanes.hpp / vit_four_lanes.hpp /
// vit_soft_lanes.hpp; it uses that file's packed-metric types and in_vgpr.  Not a header of its own.  Users: viterbi_kernel, viterbi_fused_kernel<1 | 4>
// and viterbi_soft_lanes_kernel<1 | 2>.  The hard forms of two and four lanes per code word (vit_two_lanes.hpp, vit_four_lanes.hpp) keep copies of their
// own, measured (profiles/r17_viterbi_shared_front_ab.json): with this front their decoder stage was 2 % slower at 8 .. 40 streams, where a lone wave per
// SIMD pays for every instruction, and with this chain-back walk just outside the parent's spread.  So not everything here is shared yet: the front,
// ChainOut::consume, re-base and the output record replace two or three copies each; ChainOut::block8, take_rows and register_of have ONE caller at run
// time (chain_back8, viterbi_fused_kernel<1>, softmulti::chain_back) and stand here for the forms that may join -- a move, not a saving.  The hard
// multi-lane chain-backs still carry their own consume lambda, whole-block step, select ladder and inverse compaction.
// What differs between the forms stays with them: the add-compare-select and the record layout (which word and byte or nibble holds a state's tags).

// ---- the received words of one code word --------------------------------------------------------
// Row `tile` of the lane-interleaved input (regroup_kernel / fic_group_kernel), column = the code word's place in its tile, kBits per received value.
// Every member is wave-uniform but nextw, and has to stay so: see viterbi_fused_kernel on SGPR residency.
template <int kBits>
struct RowInput {
  const uint32_t* src;
  int last_word;
  uint64_t fifo = 0;
  int have = 0;                              // wave-uniform number of valid bits in fifo
  uint32_t nextw;
  int widx = 1;
  // (a plan whose first word lies outside the row cannot arrive any more: the control plane drops such multiplexes, control_plane.hpp StreamFault;
  // the clamp keeps even a corrupted plan inside the tile's rows)
  __device__ __forceinline__ RowInput(const uint32_t* grouped, int row_words, int tile, int start_bit, int column)
  {
    const int word0 = min((start_bit * kBits) >> 5, row_words - 1);
    src = grouped + (static_cast<size_t>(tile) * row_words + word0) * 64 + column;
    last_word = row_words - 1 - word0;
    nextw = src[0];
  }
  // (one word ahead; two -- hard -- and six -- soft -- words ahead measured slower, 5.04 against 4.88 and 6.78 against 6.63 ms)
  __device__ __forceinline__ void refill()
  {
    fifo |= static_cast<uint64_t>(nextw) << have;
    have += 32;
    nextw = src[static_cast<size_t>(min(widx, last_word)) * 64];
    ++widx;
  }
  // hard bits of a unit's eight steps, one byte per step: the step's n received bits (n from counts, wave-uniform) as the row of the lane form's
  // metric table.  The caller has topped up to `need` bits.
  __device__ __forceinline__ void take_rows(uint32_t counts, int need, uint32_t (&ww)[2])
  {
    ww[0] = ww[1] = 0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int n = (counts >> (3 * g)) & 7;
      const uint32_t row = (static_cast<uint32_t>(fifo) & ((1u << n) - 1u)) + lut_row_base(n);     // table row of (value, mask)
      fifo >>= n;
      ww[g >> 2] |= row << (8 * (g & 3));
    }
    have -= need;
  }
  // soft values of a unit's eight steps straight out of the fifo's low word (4 n <= 16 bits; n wave-uniform): one 32-bit and, one 64-bit shift per
  // step -- collecting them in 64-bit words first, to be taken apart again by the steps, cost seven instructions more per step (161 -> 150 per step)
  __device__ __forceinline__ void take_soft(uint32_t counts, uint32_t (&x)[8])
  {
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const int nb = 4 * ((counts >> (3 * g)) & 7);        // bits of this step: 4 per received value
      if (have < nb) refill();
      x[g] = static_cast<uint32_t>(fifo) & ((1u << nb) - 1u);
      fifo >>= nb;
      have -= nb;
    }
  }
};

// ---- the segment walk ---------------------------------------------------------------------------
// A code word is four segments of pl.blocks[seg] x 4 units under pl.mask[seg], then the tail: one unit under puncturing vector 8, 24 mother-code bits.
// A unit is 8 trellis steps = 32 mother-code bits, of which the mask keeps `need`.
__device__ __forceinline__ uint32_t step_counts(uint32_t mask)      // values taken by each of the 8 steps of a unit, 3 bits per step
{
  uint32_t counts = 0;
  for (int g = 0; g < 8; ++g) counts |= static_cast<uint32_t>(__popc((mask >> (4 * g)) & 15u)) << (3 * g);
  return counts;
}
struct Segment {
  int units, need;
  uint32_t counts;
  __device__ __forceinline__ Segment(const CodewordPlan& pl, int seg)
  {
    const uint32_t mask = seg < 4 ? pl.mask[seg] : (puncture_mask(8) & 0x00ffffffu);
    units = seg < 4 ? 4 * pl.blocks[seg] : 1;
    need = __popc(mask);
    counts = step_counts(mask);
  }
};

// ---- the output record --------------------------------------------------------------------------
__device__ __forceinline__ uint32_t* output_words(const int* job_ids, int index, uint8_t* out, int record_stride, int out_offset)
{
  const int record = job_ids ? job_ids[index] : index;
  return reinterpret_cast<uint32_t*>(out + static_cast<size_t>(record) * record_stride + out_offset);
}

// ---- the chain-back's walk ----------------------------------------------------------------------
// From state 0 (viterbi.c:438-450), newest step first; decisions are descrambled (misc.c:41-58) and packed MSB first, a word at a time.
struct ChainOut {
  const uint32_t* __restrict__ prbs_words;
  uint32_t* dst;
  unsigned state = 0;
  uint32_t acc = 0;
  // steps t0 + k_hi .. t0 from the tags of a block of kSteps (4: nibble tags, 8: byte tags)
  template <int kSteps>
  __device__ __forceinline__ void consume(unsigned tags, int t0, int k_hi)
  {
#pragma unroll
    for (int k = kSteps - 1; k >= 0; --k) {
      const int t = t0 + k;
      if (k <= k_hi && t >= 6) {                           // steps 0..5 only flush the encoder's initial zeros
        const unsigned bit = ((tags >> k) & 1u) ^ 1u;      // tag set = low predecessor survived = decision 0
        state = (state | (bit << 6)) >> 1;
        const int i = t - 6;                               // data bit index
        acc |= bit << (8 * ((i >> 3) & 3) + (7 - (i & 7)));
        if ((i & 31) == 0) {
          dst[i >> 5] = acc ^ prbs_words[i >> 5];
          acc = 0;
        }
      }
    }
  }
  // A whole block of byte tags per step: its decisions d_k = !tag_k (k = 0 .. 7, step 8 b + k), bit-reversed: r8 = d_0 .. d_7 from the top.  Walking
  // back from step 8 b + 7 to 8 b leaves state (d_0 .. d_5) = r8 >> 2; data bit i = step - 6 goes MSB-first into byte i >> 3: d_6, d_7
  // are the top two bits of byte b, d_0 .. d_5 the low six bits of byte b - 1 -- the new state itself.
  __device__ __forceinline__ void block8(unsigned tags, int b)
  {
    if (b >= 1) {
      const unsigned r8 = __brev(~tags & 0xffu) >> 24;
      state = r8 >> 2;
      acc |= ((r8 & 3u) << 6) << (8 * (b & 3));
      if ((b & 3) == 0) {
        dst[b >> 2] = acc ^ prbs_words[b >> 2];
        acc = 0;
      }
      acc |= state << (8 * ((b - 1) & 3));
    } else {
      consume<8>(tags, 0, 7);                              // steps 0..5 only flush the encoder's initial zeros
    }
  }
};

// The register of `state` inside its lane where the lanes' registers are numbered by compaction (vit_four_lanes.hpp): the state's bits in place order
// with the places of `removed` -- the pair bit and the lane bits -- taken out.  Branch-free, for a run-time mask.  vit_four_lanes.hpp holds it against the
// forward numberings (multi::compact / expand, two::phys_of) at compile time; the inverses written out in multi::chain_back and two::chain_back8_two are
// NOT covered by that assertion, only by the GPU suite.
__host__ __device__ constexpr unsigned register_of(unsigned state, unsigned removed)
{
  unsigned P = 0, pos = 0;
  for (unsigned bit = 0; bit < 6; ++bit) {
    const unsigned keep = ((removed >> bit) & 1u) ^ 1u;
    P |= (((state >> bit) & 1u) & keep) << pos;
    pos += keep;
  }
  return P;
}

// ---- metrics of a code word spread over kLanes = 1, 2, 4 neighbouring lanes ---------------------
// State 0 is the low half of register 0 in lane 0 of the code word, in every layout of every form.
// start: state 0 at kBase, the others far below (MetricScale).  reg0 = kBase in lane 0 of the code word, 0 in its other lanes.
// (viterbi_soft_lanes_kernel keeps these lines written out: see there)
template <int kRegs>
__device__ __forceinline__ void init_metrics(pk16 (&pm)[kRegs], uint32_t reg0)
{
#pragma unroll
  for (int r = 0; r < kRegs; ++r) pm[r] = as_pk(0u);
  pm[0] = as_pk(reg0);
}
// re-base: state 0 back to kBase, in all of the code word's lanes
template <int kLanes>
__device__ __forceinline__ void rebase(pk16 (&pm)[32 / kLanes], uint32_t kBase)
{
  uint32_t r0 = as_u32(pm[0]);
  if constexpr (kLanes == 2) r0 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(r0), 0xA0 /* quad_perm [0,0,2,2]: the even lane's */, 0xf, 0xf, true));
  if constexpr (kLanes == 4) r0 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(r0), 0x00 /* quad_perm [0,0,0,0] */, 0xf, 0xf, true));
  const uint32_t s0 = (r0 & 0xffffu) - kBase;
  const uint32_t base = s0 | (s0 << 16);                  // every half is >= s0: no borrow crosses
#pragma unroll
  for (int r = 0; r < 32 / kLanes; ++r) pm[r] = as_pk(as_u32(pm[r]) - base);
}
