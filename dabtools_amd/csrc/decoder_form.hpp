// decoder_form.hpp — which form of the Viterbi decoder (include/dabhip.h: DABHIP_FORM_*) an MSC or FIC launch runs: the knobs, their defaults and
// the rule.  Host-only, no GPU call (tests/host_sanitize pins the rule at every documented crossover); kernels.hpp's launch_viterbi_form runs the form.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/dabhip.h"

namespace dabhip {

struct FormKnobs {
  // Decodes of at most this many code words (MSC: ETI frames x sub-channels; FIC: 4 per TF) run one WAVE per code word (k_vitwave.hip: latency
  // of a code word 0.1 instead of 1.4 ms) instead of one lane per code word (viterbi_fused_kernel: a sixth of the lane-ops).  DABHIP_VIT_WAVE_MAX
  // (both), DABHIP_FIC_WAVE_MAX.
  int wave_max_codewords = 12288, wave_max_fic_blocks = 3072;     // measured crossovers (tools/gpu/wavesweep.sh): MSC 5..6 streams x 64 TF, FIC 12..16
  // Above that, hard-decision decodes of at most this many groups of 64 code words run TWO LANES per code word (vit_two_lanes.hpp): while the lane form
  // would leave the SIMDs at one or two waves (8 .. 40 streams x 64 TF: decoder stage 1.45 -> 0.96 ms at 16 streams).  Measured crossover between 32 and
  // 64 streams (1,176 and 2,352 groups; profiles/r06_two_lanes_curve.txt).  DABHIP_VIT_TWO_LANES = 0 / 1 / N: never / always / at most N groups.
  int two_lanes_max_groups = 1536;
  // ... and of at most this many groups FOUR lanes per code word (vit_four_lanes.hpp): decoder stage 0.96 -> 0.82 ms at 8 and 16 streams, the same as
  // two lanes at 32 (1,176 groups; profiles/r06_lanes_curve.txt).  DABHIP_VIT_FOUR_LANES = 0 / 1 / N likewise;
  // DABHIP_VIT_LANES_PLAIN=1 (measurement) runs the two-lane decodes through that file's table-free two-lane form instead of vit_two_lanes.hpp's.
  int four_lanes_max_groups = 800;
  bool two_lanes_plain = false;
  // FIC decodes of at most this many tiles of 64 blocks (above the wave form's range: 12 .. 32 streams x 64 TF) run four lanes per block: FIC stage 0.32 -> 0.24 ms
  // at 16 streams, 0.58 -> 0.50 at 32, nothing from 64 streams (256 tiles) on.  DABHIP_FIC_FOUR_LANES = 0 / 1 / N
  int fic_four_lanes_max_tiles = 128;
  // SOFT decisions through the multi-lane forms (vit_soft_lanes.hpp): opt-in.  With soft_lanes off (the default) a soft launch outside the wave form runs
  // the lane form whatever is forced, as it always has.  With it on (set_soft_lanes, DABHIP_SOFT_LANES=1) a forced FOUR or TWO_PLAIN (FIC: FOUR) is
  // honoured, a forced TWO (per-lane tables of hard metrics) still runs the lane form, and under AUTO the two knobs below choose between FOUR and LANE:
  // soft MSC decodes of at most soft_four_lanes_max_groups groups, soft FIC decodes of at most soft_fic_four_lanes_max_tiles tiles, run four lanes.
  // DABHIP_VIT_SOFT_FOUR_LANES, DABHIP_FIC_SOFT_FOUR_LANES = 0 / 1 / N.  profiles/r08_soft_lanes_curve.json (tools/soft_lanes_curve.py: 5 dB, 64 TF,
  // rounds interleaved on one box, the same build's lane form as baseline): the MSC stage 2.26 -> 1.78 ms at 8 streams, 2.28 -> 1.66 at 16, 2.40 -> 1.95
  // at 32 (1176 groups) and the whole decode with it by more than the spread between rounds, 2.79 -> 3.25 at 64 (2352 groups): 1176.  The FIC stage
  // gains 0.10 .. 0.13 ms at every size (31 .. 248 tiles), which the whole decode's spread between rounds (0.3 .. 1.0 ms) swallows: four wins nowhere by
  // the rule, 0 = never.
  bool soft_lanes = false;
  int soft_four_lanes_max_groups = 1176, soft_fic_four_lanes_max_tiles = 0;

  void from_env()
  {
    auto knob = [](const char* name, int* v) { if (const char* env = std::getenv(name)) *v = std::max(0, std::atoi(env)); };
    knob("DABHIP_VIT_WAVE_MAX", &wave_max_codewords);
    knob("DABHIP_VIT_WAVE_MAX", &wave_max_fic_blocks);
    knob("DABHIP_VIT_TWO_LANES", &two_lanes_max_groups);
    knob("DABHIP_VIT_FOUR_LANES", &four_lanes_max_groups);
    knob("DABHIP_FIC_FOUR_LANES", &fic_four_lanes_max_tiles);
    if (const char* env = std::getenv("DABHIP_VIT_LANES_PLAIN")) two_lanes_plain = std::atoi(env) != 0;
    knob("DABHIP_FIC_WAVE_MAX", &wave_max_fic_blocks);
    if (const char* env = std::getenv("DABHIP_SOFT_LANES")) soft_lanes = std::atoi(env) != 0;
    knob("DABHIP_VIT_SOFT_FOUR_LANES", &soft_four_lanes_max_groups);
    knob("DABHIP_FIC_SOFT_FOUR_LANES", &soft_fic_four_lanes_max_tiles);
  }
};

inline bool knob_admits(int knob, int n) { return knob > 0 && (knob == 1 || n <= knob); }      // 0 / 1 / N = never / always / at most N

inline bool msc_form_valid(int form) { return form >= DABHIP_FORM_AUTO && form <= DABHIP_FORM_FOUR; }
inline bool fic_form_valid(int form) { return form == DABHIP_FORM_AUTO || form == DABHIP_FORM_WAVE || form == DABHIP_FORM_LANE || form == DABHIP_FORM_FOUR; }

// the work-list build's bound (worklist.hpp: plan_decode_batch): a forced form puts every batch, or none, in the wave form
inline int64_t msc_wave_max(const FormKnobs& k, int forced) { return forced == DABHIP_FORM_AUTO ? k.wave_max_codewords : forced == DABHIP_FORM_WAVE ? INT64_MAX : 0; }

// MSC launch over `ngroups` groups of 64 code words of a batch that is (wave_batch) or is not laid out for the wave form.  A form set by
// set_decoder_forms (forced != AUTO) replaces the rule.  Soft decisions: the lane form, forced or not, unless k.soft_lanes is on (see FormKnobs).
inline int msc_form(const FormKnobs& k, int forced, bool soft, bool wave_batch, int ngroups)
{
  if (wave_batch) return DABHIP_FORM_WAVE;
  if (soft) {
    if (!k.soft_lanes) return DABHIP_FORM_LANE;
    if (forced != DABHIP_FORM_AUTO) return forced == DABHIP_FORM_TWO_PLAIN || forced == DABHIP_FORM_FOUR ? forced : DABHIP_FORM_LANE;
    return knob_admits(k.soft_four_lanes_max_groups, ngroups) ? DABHIP_FORM_FOUR : DABHIP_FORM_LANE;
  }
  if (forced != DABHIP_FORM_AUTO) return forced == DABHIP_FORM_TWO || forced == DABHIP_FORM_TWO_PLAIN || forced == DABHIP_FORM_FOUR ? forced : DABHIP_FORM_LANE;
  if (knob_admits(k.four_lanes_max_groups, ngroups)) return DABHIP_FORM_FOUR;
  if (knob_admits(k.two_lanes_max_groups, ngroups)) return k.two_lanes_plain ? DABHIP_FORM_TWO_PLAIN : DABHIP_FORM_TWO;
  return DABHIP_FORM_LANE;
}

// FIC launch over nblocks blocks in ntiles tiles of 64.  Few blocks: one wave per block; more, but not enough to fill the device with one lane per block
// (774 dependent steps in front of the control plane): four lanes per block, up to 128 tiles = 32 streams x 64 TF (measured: nothing to gain above).
inline int fic_form(const FormKnobs& k, int forced, bool soft, int nblocks, int ntiles)
{
  const bool is_forced = forced != DABHIP_FORM_AUTO;
  if (is_forced ? forced == DABHIP_FORM_WAVE : nblocks <= k.wave_max_fic_blocks) return DABHIP_FORM_WAVE;
  if (soft && !k.soft_lanes) return DABHIP_FORM_LANE;
  const int four_max = soft ? k.soft_fic_four_lanes_max_tiles : k.fic_four_lanes_max_tiles;
  if (is_forced ? forced == DABHIP_FORM_FOUR : knob_admits(four_max, ntiles)) return DABHIP_FORM_FOUR;
  return DABHIP_FORM_LANE;
}

}  // namespace dabhip
