// scan_plan.hpp — the schedule of one K1 scan (engine_scan.cpp runs it): how many calls per stream, whether the split scan (chain + verification)
// and the chain's look-ahead pass run, and with which table and passes.  Host-only, no GPU call (tests/host_sanitize pins the rule at every crossover).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "device_types.hpp"

namespace dabhip {

// measurement knobs (tools/gpu/k1_ahead_sweep.sh): the window of start positions the pass covers (DABHIP_K1_HYP: odd, 3 .. 63; default 33 = +-16 samples) and
// the largest batch that takes the pass by default (DABHIP_K1_SPEC_MAX_STREAMS, default 4)
struct ScanKnobs {
  int hypotheses = 33, spec_max_streams = 4;
  static int odd_window(int v) { return std::max(3, std::min(63, v | 1)); }
  static ScanKnobs from_env()
  {
    ScanKnobs k;
    if (const char* e = std::getenv("DABHIP_K1_HYP")) k.hypotheses = std::atoi(e);
    if (const char* e = std::getenv("DABHIP_K1_SPEC_MAX_STREAMS")) k.spec_max_streams = std::atoi(e);
    return k;
  }
};

struct ScanPlan {
  int max_calls = 1;       // calls of the stream that has most left; the stride of the scan's descriptors
  size_t ndesc = 0;        // nstreams x max_calls
  bool split = false;      // chain + parallel verification (false: the reference's order, call after call)
  bool ahead = false;      // the chain runs with the look-ahead pass
  int nspec = 0;           // calls of a stream per pass
  int nhyp = 0, passes = 0;
  int first_limit = 0;     // calls of the chain launch in front of the first pass
  size_t result_words = 0; // what the host fetches behind the scan, in 32-bit words (small: one kernel writes them; large: copy-engine commands)
  int pass_limit(int r) const { return r + 1 < passes ? nspec : -1; }      // calls of the chain launch behind pass r (-1: to the end)
};

// The look-ahead schedule of the chain (k_sync.hip: sync_ahead_kernel) where the chain would leave most of the device idle: few streams, many calls.
// spec_mode 0 / 1: never / always (tests run both); -1: up to spec_max_streams streams of at least kAheadMinCalls calls.
// (forced on, the pass is still bounded: beyond kAheadForcedMaxStreams streams -- where it cannot help and its table, nstreams x nspec x 33 x 8 bytes
// with nspec >= 64, would run to tens of megabytes and 33 x nspec x nstreams workgroups -- the plain chain runs whatever the mode says)
// ncalls[b]: complete calls stream b holds; calls_done[b]: those an earlier segment scanned.  cont: a session's further segment.
inline ScanPlan plan_scan(int nstreams, const int* ncalls, const int* calls_done, bool afc, bool full_scan, bool cont, int spec_mode, const ScanKnobs& knobs)
{
  constexpr int kAheadMinCalls = 16, kAheadForcedMaxStreams = 512;
  ScanPlan p;
  for (int b = 0; b < nstreams; ++b) p.max_calls = std::max(p.max_calls, ncalls[b] - calls_done[b]);
  p.ndesc = static_cast<size_t>(nstreams) * p.max_calls;
  p.split = !(afc || full_scan);
  p.ahead = p.split && spec_mode != 0 &&
            (spec_mode > 0 ? nstreams <= kAheadForcedMaxStreams : (nstreams <= std::max(0, std::min(512, knobs.spec_max_streams)) && p.max_calls >= kAheadMinCalls));
  // calls of a stream per pass: all it has, within a bound on the table (8 bytes per call, start position and stream)
  p.nspec = std::min(p.max_calls, std::min(4096, std::max(64, (1 << 20) / nstreams)));
  p.nhyp = ScanKnobs::odd_window(knobs.hypotheses);
  p.passes = std::min(16, (p.max_calls + p.nspec - 1) / p.nspec);
  // a short chain to lock on (a fresh capture: the first frame is dropped, the second finds the null symbol, the third the fine shift -- seven calls;
  // a session's further segment stands where it stands)
  p.first_limit = cont ? 0 : 7;
  p.result_words = (p.split ? nstreams + 1 : 0) + (p.ahead ? 1 : 0) + p.ndesc * 2 + static_cast<size_t>(nstreams) * (sizeof(StreamState) / 4);
  return p;
}

}  // namespace dabhip
