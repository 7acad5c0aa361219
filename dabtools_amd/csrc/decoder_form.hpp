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
  }
};

inline bool knob_admits(int knob, int n) { return knob > 0 && (knob == 1 || n <= knob); }      // 0 / 1 / N = never / always / at most N

inline bool msc_form_valid(int form) { return form >= DABHIP_FORM_AUTO && form <= DABHIP_FORM_FOUR; }
inline bool fic_form_valid(int form) { return form == DABHIP_FORM_AUTO || form == DABHIP_FORM_WAVE || form == DABHIP_FORM_LANE || form == DABHIP_FORM_FOUR; }

// the work-list build's bound (worklist.hpp: plan_decode_batch): a forced form puts every batch, or none, in the wave form
inline int64_t msc_wave_max(const FormKnobs& k, int forced) { return forced == DABHIP_FORM_AUTO ? k.wave_max_codewords : forced == DABHIP_FORM_WAVE ? INT64_MAX : 0; }

// MSC launch over `ngroups` groups of 64 code words of a batch that is (wave_batch) or is not laid out for the wave form.  A form set by
// set_decoder_forms (forced != AUTO) replaces the rule; multi-lane forms are hard-only: a soft engine runs, and reports, the lane form.
inline int msc_form(const FormKnobs& k, int forced, bool soft, bool wave_batch, int ngroups)
{
  if (wave_batch) return DABHIP_FORM_WAVE;
  if (soft) return DABHIP_FORM_LANE;
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
  if (!soft && (is_forced ? forced == DABHIP_FORM_FOUR : knob_admits(k.fic_four_lanes_max_tiles, ntiles))) return DABHIP_FORM_FOUR;
  return DABHIP_FORM_LANE;
}

}  // namespace dabhip
