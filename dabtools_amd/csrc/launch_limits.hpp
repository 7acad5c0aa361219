// launch_limits.hpp — the sizes past which a decode is split into several launches (or takes another path), in one place.  Host only.
//
// Every loop below runs once at any test-sized input with the default limits; an engine whose limits are lowered (dabhip_engine_set_launch_limits: test
// knob, per engine) runs the same loops in many pieces over a small input, and LaunchReport says how many there were (DESIGN.md has the table).
#pragma once

#include <cstdint>

namespace dabhip {

constexpr int64_t kMaxDecisionRows = int64_t(48) << 20;   // x 512 B = 24 GiB of survivor decisions per decoder launch
constexpr int kMaxRegroupTiles = 32768;                   // tiles of 64 records per regroup launch
constexpr int kMaxFicGroupTiles = 32768;                  // tiles of 64 FIC blocks per FIC-group launch
constexpr int kMaxGridY = 65535;                          // what a launch's grid.y holds: the bound of the FIC-group and device-gather limits
constexpr int kMaxGatherDescs = kMaxGridY;                    // descriptors per device-gather launch: grid.y holds 65,535
constexpr int64_t kMaxFetchWords = int64_t(1) << 18;      // scan results fetched by one kernel that writes the host arrays; more: copy-engine commands
constexpr int kFftChunkTfs = 4096;                        // spectra buffer: 4096 TF x 1.19 MiB = 4.75 GiB (measured: 1024 -> 4096 shortens K2 by 5 %, launch tails)

struct LaunchLimits {
  int64_t decision_rows = kMaxDecisionRows;   // survivor-record rows per decoder launch (worklist.hpp: plan_decode_batch)
  int regroup_tiles = kMaxRegroupTiles;       // a multiple of 8: the kernel deals tiles to the XCDs in eights
  int fic_group_tiles = kMaxFicGroupTiles;
  int gather_descs = kMaxGatherDescs;         // at most 65535
  int64_t fetch_words = kMaxFetchWords;
  int fft_chunk_tfs = kFftChunkTfs;           // TFs per chunk of the two-kernel OFDM stage (its FIC pre-pass: 19 x as many)
};
constexpr int kLaunchLimitCount = 6;

// v[0 .. 6): the fields in the order above, 0 = the default.  Null when every value is legal (then *out holds them), else what is wrong with the first that is not.
inline const char* launch_limits_from(const int64_t* v, LaunchLimits* out)
{
  LaunchLimits l;
  for (int i = 0; i < kLaunchLimitCount; ++i)
    if (v[i] < 0) return "a launch limit is negative";
  if (v[1] % 8 != 0) return "the regroup limit must be a multiple of 8 tiles (the kernel deals tiles in eights)";
  if (v[1] > kMaxRegroupTiles) return "the regroup limit is above 32768 tiles";
  if (v[2] > kMaxGridY) return "the FIC-group limit is above 65535 tiles (grid.y)";
  if (v[3] > kMaxGatherDescs) return "the device-gather limit is above 65535 descriptors (grid.y)";
  if (v[5] > (int64_t(1) << 20)) return "the OFDM chunk is above 2^20 transmission frames";
  if (v[0]) l.decision_rows = v[0];
  if (v[1]) l.regroup_tiles = static_cast<int>(v[1]);
  if (v[2]) l.fic_group_tiles = static_cast<int>(v[2]);
  if (v[3]) l.gather_descs = static_cast<int>(v[3]);
  if (v[4]) l.fetch_words = v[4];
  if (v[5]) l.fft_chunk_tfs = static_cast<int>(v[5]);
  *out = l;
  return nullptr;
}

// [0, n) cut into pieces of at most `limit` (limit >= 1): piece i is [first(i), first(i) + size(i)), all but the last are full.  The launch loops share it.
struct Pieces {
  int64_t n, limit;
  int64_t count() const { return n <= 0 ? 0 : (n + limit - 1) / limit; }
  int64_t first(int64_t i) const { return i * limit; }
  int64_t size(int64_t i) const { return n - i * limit < limit ? n - i * limit : limit; }
};

// What the last decode (segment, stage entry) really did: launches made by each of the loops above, and how the scan's results came back.
enum { kFetchNone = 0, kFetchKernel = 1, kFetchCopyEngine = 2 };
struct LaunchReport {
  int64_t decoder = 0;        // MSC Viterbi launches = slices of the batch
  int64_t regroup = 0;
  int64_t fic_group = 0;
  int64_t gather = 0;         // device-gather launches (streaming sessions)
  int64_t ofdm_chunks = 0;    // launches of the OFDM stage over the MSC symbols (either stage; read_demapped_tf's completion adds its own), chunks of the two-kernel audit
  int64_t fic_prepass = 0;    // the two-kernel stage's pre-pass over the FIC symbols (launches made: a rescan lays the frames out and runs it again)
  int64_t fetch_form = 0;     // kFetch*: of the last scan fetch
  int64_t fetches = 0;        // scan fetches (2: a stream was scanned again)
  int64_t gather_calls = 0;   // device gathers those launches belong to
  int64_t decoder_planned = 0;   // slices the host plan of the MSC batch holds (slice_start.size() - 1): decoder must equal it
};
constexpr int kLaunchReportCount = 10;

}  // namespace dabhip
