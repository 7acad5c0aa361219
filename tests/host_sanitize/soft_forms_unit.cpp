// soft_forms_unit.cpp -- the decoder-form rule (dabtools_amd/csrc/decoder_form.hpp) with the soft multi-lane switch: a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_soft_forms_unit.py).  With FormKnobs::soft_lanes off the rule for soft input is the table that
// host_units.cpp pins; with it on, forced forms, the 0 / 1 / N reading of the two soft knobs, and hard input untouched by all three.
#include <cstdio>
#include <cstdlib>

#include "../../dabtools_amd/csrc/decoder_form.hpp"

using namespace dabhip;

static int g_failures = 0;
#define CHECK(x)                                                                  \
  do {                                                                            \
    if (!(x)) {                                                                   \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x);  \
      ++g_failures;                                                               \
    }                                                                             \
  } while (0)

static const int AUTO = DABHIP_FORM_AUTO, WAVE = DABHIP_FORM_WAVE, LANE = DABHIP_FORM_LANE, TWO = DABHIP_FORM_TWO, PLAIN = DABHIP_FORM_TWO_PLAIN,
                 FOUR = DABHIP_FORM_FOUR;

// the rule as it stood before the switch existed
static int old_msc_form(const FormKnobs& k, int forced, bool soft, bool wave_batch, int ngroups)
{
  if (wave_batch) return WAVE;
  if (soft) return LANE;
  if (forced != AUTO) return forced == TWO || forced == PLAIN || forced == FOUR ? forced : LANE;
  if (knob_admits(k.four_lanes_max_groups, ngroups)) return FOUR;
  if (knob_admits(k.two_lanes_max_groups, ngroups)) return k.two_lanes_plain ? PLAIN : TWO;
  return LANE;
}
static int old_fic_form(const FormKnobs& k, int forced, bool soft, int nblocks, int ntiles)
{
  const bool is_forced = forced != AUTO;
  if (is_forced ? forced == WAVE : nblocks <= k.wave_max_fic_blocks) return WAVE;
  if (!soft && (is_forced ? forced == FOUR : knob_admits(k.fic_four_lanes_max_tiles, ntiles))) return FOUR;
  return LANE;
}

static const int kSizes[] = {1, 5, 48, 49, 128, 129, 800, 801, 1536, 1537, 100000};

static void test_switch_off()
{
  const FormKnobs def;
  CHECK(!def.soft_lanes);
  // off: the soft knobs are dead, whatever they hold
  for (int soft_four : {0, 1, 500}) {
    FormKnobs k;
    k.soft_four_lanes_max_groups = soft_four;
    k.soft_fic_four_lanes_max_tiles = soft_four;
    for (int forced = AUTO; forced <= FOUR; ++forced)
      for (int n : kSizes)
        for (int wave = 0; wave < 2; ++wave) {
          CHECK(msc_form(k, forced, true, wave != 0, n) == old_msc_form(k, forced, true, wave != 0, n));
          CHECK(msc_form(k, forced, true, wave != 0, n) == (wave ? WAVE : LANE));
          if (fic_form_valid(forced)) CHECK(fic_form(k, forced, true, 64 * n, n) == old_fic_form(k, forced, true, 64 * n, n));
        }
  }
  // today's table for soft input, spelled out
  CHECK(msc_form(def, FOUR, true, false, 5) == LANE && msc_form(def, PLAIN, true, false, 5) == LANE && msc_form(def, TWO, true, false, 5) == LANE);
  CHECK(fic_form(def, FOUR, true, 4, 1) == LANE && fic_form(def, AUTO, true, 3076, 49) == LANE && fic_form(def, AUTO, true, 3072, 48) == WAVE);
}

static void test_switch_on()
{
  FormKnobs on;
  on.soft_lanes = true;
  // forced forms, soft input: FOUR and TWO_PLAIN honoured, TWO (tables of hard metrics) and the rest the lane form; a wave batch stays a wave batch
  for (int n : kSizes) {
    CHECK(msc_form(on, FOUR, true, false, n) == FOUR);
    CHECK(msc_form(on, PLAIN, true, false, n) == PLAIN);
    CHECK(msc_form(on, TWO, true, false, n) == LANE);
    CHECK(msc_form(on, LANE, true, false, n) == LANE);
    CHECK(msc_form(on, WAVE, true, false, n) == LANE);
    CHECK(msc_form(on, FOUR, true, true, n) == WAVE);
    CHECK(fic_form(on, FOUR, true, 64 * n, n) == FOUR);
    CHECK(fic_form(on, LANE, true, 64 * n, n) == LANE);
    CHECK(fic_form(on, WAVE, true, 64 * n, n) == WAVE);
  }
  // AUTO: the soft knobs decide between FOUR and LANE, read 0 / 1 / N; two lanes are never asked for, and the hard knobs do not count
  struct { int knob, n, want; } msc[] = {{0, 1, LANE}, {0, 100000, LANE}, {1, 1, FOUR}, {1, 100000, FOUR}, {40, 40, FOUR}, {40, 41, LANE}, {800, 800, FOUR}, {800, 801, LANE}};
  for (const auto& t : msc)
    for (int two : {0, 1, 1536})
      for (int plain = 0; plain < 2; ++plain) {
        FormKnobs k = on;
        k.soft_four_lanes_max_groups = t.knob;
        k.two_lanes_max_groups = two;
        k.two_lanes_plain = plain != 0;
        k.four_lanes_max_groups = 1;
        CHECK(msc_form(k, AUTO, true, false, t.n) == t.want);
        CHECK(msc_form(k, AUTO, true, true, t.n) == WAVE);
      }
  struct { int wave, knob, nblocks, ntiles, want; } fic[] = {{3072, 0, 3076, 49, LANE}, {3072, 1, 400000, 6250, FOUR}, {3072, 128, 8192, 128, FOUR}, {3072, 128, 8196, 129, LANE},
                                                              {0, 10, 640, 10, FOUR},   {0, 10, 644, 11, LANE},        {3072, 128, 3072, 48, WAVE},  {3, 128, 4, 1, FOUR}};
  for (const auto& t : fic) {
    FormKnobs k = on;
    k.wave_max_fic_blocks = t.wave;
    k.soft_fic_four_lanes_max_tiles = t.knob;
    k.fic_four_lanes_max_tiles = 1;             // the hard knob does not count for soft input ...
    CHECK(fic_form(k, AUTO, true, t.nblocks, t.ntiles) == t.want);
    k.fic_four_lanes_max_tiles = 0;
    CHECK(fic_form(k, AUTO, true, t.nblocks, t.ntiles) == t.want);
  }
}

// hard input: none of the three new knobs moves anything
static void test_hard_unaffected()
{
  for (int lanes = 0; lanes < 2; ++lanes)
    for (int soft_four : {0, 1, 40})
      for (int soft_fic : {0, 1, 40}) {
        FormKnobs k;
        const FormKnobs def;
        k.soft_lanes = lanes != 0;
        k.soft_four_lanes_max_groups = soft_four;
        k.soft_fic_four_lanes_max_tiles = soft_fic;
        for (int forced = AUTO; forced <= FOUR; ++forced)
          for (int n : kSizes)
            for (int wave = 0; wave < 2; ++wave) {
              CHECK(msc_form(k, forced, false, wave != 0, n) == old_msc_form(def, forced, false, wave != 0, n));
              if (fic_form_valid(forced)) CHECK(fic_form(k, forced, false, 64 * n, n) == old_fic_form(def, forced, false, 64 * n, n));
            }
        CHECK(msc_wave_max(k, AUTO) == msc_wave_max(def, AUTO));
      }
  // the form ids did not grow: 5 is still no form
  CHECK(!msc_form_valid(5) && !fic_form_valid(5) && msc_form_valid(FOUR) && fic_form_valid(FOUR));
}

// the environment: DABHIP_SOFT_LANES and the two soft knobs, read like their hard kin
static void test_env()
{
  setenv("DABHIP_SOFT_LANES", "1", 1);
  setenv("DABHIP_VIT_SOFT_FOUR_LANES", "77", 1);
  setenv("DABHIP_FIC_SOFT_FOUR_LANES", "1", 1);
  FormKnobs k;
  k.from_env();
  CHECK(k.soft_lanes && k.soft_four_lanes_max_groups == 77 && k.soft_fic_four_lanes_max_tiles == 1);
  CHECK(msc_form(k, AUTO, true, false, 77) == FOUR && msc_form(k, AUTO, true, false, 78) == LANE);
  CHECK(fic_form(k, AUTO, true, 400000, 6250) == FOUR);
  setenv("DABHIP_SOFT_LANES", "0", 1);
  FormKnobs off;
  off.from_env();
  CHECK(!off.soft_lanes && msc_form(off, AUTO, true, false, 77) == LANE);
  unsetenv("DABHIP_SOFT_LANES");
  unsetenv("DABHIP_VIT_SOFT_FOUR_LANES");
  unsetenv("DABHIP_FIC_SOFT_FOUR_LANES");
}

int main()
{
  test_switch_off();
  test_switch_on();
  test_hard_unaffected();
  test_env();
  if (g_failures) return 1;
  std::printf("ok soft-forms\n");
  return 0;
}
