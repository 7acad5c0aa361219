// ingest_plan.hpp — the host rule of the ingest stage (ingest.cpp runs it, k_ingest.hip is its kernel): which sample rates are taken and with which
// ratio, the tap table and the conditions it is held to, the automatic gain, and the bookkeeping of one push.  Host-only, no GPU call
// (tests/host_sanitize/ingest_units.cpp runs it on byte arrays of exactly the planned sizes).  The arithmetic is stated in include/dabhip.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

namespace dabhip {

constexpr int kIngestFormats = 4;                  // DABHIP_INGEST_CU8 / CS8 / CS16 / CF32
constexpr int64_t kIngestOutRate = 2048000;
constexpr int64_t kIngestMinRate = 2048000, kIngestMaxRate = 10240000;
constexpr int kIngestMaxL = 1024;
constexpr int64_t kIngestGainWindow = 65536;       // W: input samples of a stream the automatic gain is measured over
constexpr uint32_t kIngestUnitGain = 256, kIngestMaxGain = (1u << 24) - 1;
constexpr int kIngestTile = 1024;                  // outputs of one workgroup of the kernel
constexpr size_t kIngestMaxTableBytes = 65536;     // the table as the kernel holds it in LDS (rows padded by one word), beside the input tile

inline int ingest_sample_bytes(int format) { return format == 0 || format == 1 ? 2 : format == 2 ? 4 : format == 3 ? 8 : 0; }

struct IngestRatio {
  int L = 1, M = 1, T = 0;                         // out/in = L/M reduced; T taps per phase (even; 0: L/M = 1/1, no filter)
  bool bypass() const { return T == 0; }
  size_t lds_row_words() const { return static_cast<size_t>(T / 2 + 1); }      // a phase in LDS: T/2 tap pairs and one word of padding (odd stride)
  size_t lds_table_bytes() const { return bypass() ? 0 : static_cast<size_t>(L) * lds_row_words() * 4; }
  // input samples one workgroup's tile of outputs can reach (rounded up to whole pairs on both sides)
  int tile_span() const { return static_cast<int>((static_cast<int64_t>(kIngestTile - 1) * M) / L) + 1 + T + 2; }
};

// the ratio of a rate, or the reason it is refused ("" = taken)
inline std::string ingest_ratio(int64_t rate_hz, IngestRatio* r)
{
  if (rate_hz < kIngestMinRate || rate_hz > kIngestMaxRate)
    return "sample rate " + std::to_string(rate_hz) + " Hz is outside 2048000 .. 10240000";
  int64_t a = kIngestOutRate, b = rate_hz;
  while (b) { const int64_t t = a % b; a = b; b = t; }
  const int64_t L = kIngestOutRate / a, M = rate_hz / a;
  if (L > kIngestMaxL) return "sample rate " + std::to_string(rate_hz) + " Hz reduces to " + std::to_string(L) + "/" + std::to_string(M) + ": more than 1024 filter phases";
  r->L = static_cast<int>(L);
  r->M = static_cast<int>(M);
  r->T = (L == 1 && M == 1) ? 0 : static_cast<int>(4 * ((8 * M + L - 1) / L));
  if (r->lds_table_bytes() > kIngestMaxTableBytes)
    return "sample rate " + std::to_string(rate_hz) + " Hz needs a tap table of " + std::to_string(r->lds_table_bytes()) + " bytes: the kernel holds 65536";
  return "";
}

// ---- the tap table: taps[p][k], int16 in Q14 ------------------------------------------------------------------
// Prototype at rate L Fin: a Kaiser (beta = 7) windowed sinc with its -6 dB point at 1.024 MHz, centred on zero delay: taps[p][k] is the prototype
// at (k - T/2) L + p.  Each phase is scaled to sum 16384 and the rounding remainder goes on its largest tap.
inline double ingest_bessel_i0(double x)
{
  double sum = 1.0, term = 1.0;
  for (int k = 1; k < 64; ++k) {
    term *= (x / (2.0 * k)) * (x / (2.0 * k));
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}
// (The tuned mode's table, further down, is the same construction with its own T, cut-off and beta.)
inline std::vector<int16_t> ingest_design_taps(const IngestRatio& r, int64_t rate_hz, double cutoff_hz = 1024000.0, double beta = 7.0)
{
  const int L = r.L, T = r.T;
  std::vector<int16_t> taps(static_cast<size_t>(L) * T);
  const double pi = 3.14159265358979323846, half = 0.5 * T * L;
  const double fc = 2.0 * cutoff_hz / (static_cast<double>(L) * static_cast<double>(rate_hz));      // cycles per prototype sample, doubled: sinc(fc i)
  const double i0b = ingest_bessel_i0(beta);
  std::vector<double> h(static_cast<size_t>(T));
  for (int p = 0; p < L; ++p) {
    double sum = 0;
    for (int k = 0; k < T; ++k) {
      const double i = static_cast<double>(k - T / 2) * L + p, u = i / half, a = pi * fc * i;
      const double w = ingest_bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
      h[static_cast<size_t>(k)] = (i == 0 ? 1.0 : std::sin(a) / a) * w;
      sum += h[static_cast<size_t>(k)];
    }
    int total = 0, big = 0;
    for (int k = 0; k < T; ++k) {
      const int q = static_cast<int>(std::lrint(h[static_cast<size_t>(k)] * 16384.0 / sum));
      taps[static_cast<size_t>(p) * T + k] = static_cast<int16_t>(q);
      total += q;
      if (std::abs(q) > std::abs(taps[static_cast<size_t>(p) * T + big])) big = k;
    }
    taps[static_cast<size_t>(p) * T + big] = static_cast<int16_t>(taps[static_cast<size_t>(p) * T + big] + (16384 - total));
  }
  return taps;
}
// what the kernel's int32 accumulators rest on: every phase sums to 16384 and its absolute sum is at most 65535 ("" = holds)
inline std::string ingest_check_taps(const IngestRatio& r, const int16_t* taps)
{
  for (int p = 0; p < r.L; ++p) {
    int64_t sum = 0, mag = 0;
    for (int k = 0; k < r.T; ++k) { sum += taps[static_cast<size_t>(p) * r.T + k]; mag += std::abs(static_cast<int>(taps[static_cast<size_t>(p) * r.T + k])); }
    if (sum != 16384) return "tap table: phase " + std::to_string(p) + " sums to " + std::to_string(sum) + ", not 16384";
    if (mag > 65535) return "tap table: phase " + std::to_string(p) + " has an absolute sum of " + std::to_string(mag) + " > 65535 (int32 accumulators could overflow)";
  }
  return "";
}

// ---- automatic gain: from E = sum(I^2 + Q^2) over the first W samples in the 16-bit domain to 32 LSB rms per rail -----------------------------
inline uint32_t ingest_auto_gain(uint64_t energy)
{
  if (energy == 0) return kIngestUnitGain;
  const double rms = std::sqrt(static_cast<double>(energy) / (2.0 * static_cast<double>(kIngestGainWindow)));
  const double g = std::floor(32.0 * 65536.0 / rms + 0.5);
  return g < 1.0 ? 1u : g > static_cast<double>(kIngestMaxGain) ? kIngestMaxGain : static_cast<uint32_t>(g);
}

// ---- bookkeeping of one stream -------------------------------------------------------------------------------
// Positions are absolute and 64-bit: `pushed` input samples so far, `produced` outputs so far, input samples [kept_from, pushed) carried.
struct IngestStreamState {
  int64_t pushed = 0, produced = 0, kept_from = 0;
  bool window_open = false;                        // automatic gain, fewer than W samples seen: everything is held back
};
struct IngestPush {
  int64_t first_out = 0, nout = 0;                 // outputs [first_out, first_out + nout) are completed by this push
  int64_t carry_from = 0, carry = 0;               // before the push: input samples [carry_from, carry_from + carry) are what was kept
  int64_t new_from = 0;                            // position of the push's first sample
  int64_t end = 0;                                 // samples there are afterwards
  int64_t keep_from = 0, keep = 0;                 // to carry afterwards: T - 1 samples, or all of them while the gain window is open
  bool closes = false;                             // the gain window closes in this push: the energy of samples [0, W) is wanted first
};
// outputs that exist once `pushed` samples are there: output m needs input sample floor(m M / L) + T/2
inline int64_t ingest_outputs_complete(const IngestRatio& r, int64_t pushed)
{
  const int64_t k = pushed - 1 - r.T / 2;          // the newest n0 that is served
  if (k < 0) return 0;
  return static_cast<int64_t>((static_cast<unsigned __int128>(k + 1) * static_cast<unsigned>(r.L) + static_cast<unsigned>(r.M) - 1) / static_cast<unsigned>(r.M));
}
inline IngestPush ingest_plan_push(const IngestRatio& r, IngestStreamState& s, int64_t nsamples)
{
  IngestPush p;
  p.carry_from = s.kept_from;
  p.carry = s.pushed - s.kept_from;
  p.new_from = s.pushed;
  s.pushed += nsamples;
  p.end = s.pushed;
  p.first_out = s.produced;
  if (s.window_open && s.pushed < kIngestGainWindow) {
    p.keep_from = 0;
  } else {
    p.closes = s.window_open;
    s.window_open = false;
    const int64_t total = ingest_outputs_complete(r, s.pushed);
    p.nout = total - s.produced;
    s.produced = total;
    p.keep_from = std::max<int64_t>(0, s.pushed - std::max(0, r.T - 1));
  }
  p.keep = s.pushed - p.keep_from;
  s.kept_from = p.keep_from;
  return p;
}
// dabhip_ingest_skip: n zero samples whose outputs nobody wants.  Once T of them have gone through the filter the carry is all zeros and stays so:
// `through` of them are pushed for real (at most T), the rest only moves the positions.  Explicit gain only (no window to hold).
inline int64_t ingest_skip_through(const IngestRatio& r, int64_t n) { return std::min<int64_t>(n, r.T); }
inline void ingest_skip_rest(const IngestRatio& r, IngestStreamState& s, int64_t rest)
{
  s.pushed += rest;
  s.produced = ingest_outputs_complete(r, s.pushed);
  s.kept_from = std::max<int64_t>(0, s.pushed - std::max(0, r.T - 1));
}

// ---- the tuned mode (dabhip_ingest_create_tuned): K channels out of one wideband stream ------------------------------------------------------
// A mixer in front of the resampler (include/dabhip.h, "tuned mode").  The table is steeper, because the neighbouring block begins 944 kHz from the
// wanted one's centre: twice the taps, cut-off 856 kHz.  The kernel holds that table, the input tile and the NCO table in one workgroup's LDS.
constexpr int kTuneMaxChannels = 16;
constexpr int64_t kTuneHalfBand = 768000;          // a DAB block's occupied half width: |f| + this must lie within Fin / 2
constexpr double kTuneCutoffHz = 856000.0, kTuneBeta = 7.0;
constexpr int kTuneNcoSize = 4096;                 // entries of (cos, sin) in Q14
constexpr size_t kTuneMaxLdsBytes = 160 * 1024;    // gfx950: LDS of one CU, all of which one workgroup may have

// what the tuned kernel asks of LDS: the table (rounded up to a double word), the tile's pairs of both rails, the NCO table
inline size_t ingest_tune_lds_bytes(const IngestRatio& r)
{
  if (r.bypass()) return 0;
  return ((r.lds_table_bytes() / 4 + 1) & ~size_t(1)) * 4 + static_cast<size_t>(r.tile_span() / 2 + 2) * 8 + static_cast<size_t>(kTuneNcoSize) * 4;
}
inline std::string ingest_tune_fits(const IngestRatio& r, int64_t rate_hz)
{
  if (ingest_tune_lds_bytes(r) > kTuneMaxLdsBytes)
    return "sample rate " + std::to_string(rate_hz) + " Hz needs " + std::to_string(ingest_tune_lds_bytes(r)) + " bytes of LDS for the tuned table, the input tile and the NCO table: a workgroup has 163840";
  return "";
}
// the tuned ratio of a rate: ingest_ratio's with twice the taps, or the reason it is refused
inline std::string ingest_tune_ratio(int64_t rate_hz, IngestRatio* r)
{
  const std::string why = ingest_ratio(rate_hz, r);
  if (!why.empty()) return why;
  r->T *= 2;
  return ingest_tune_fits(*r, rate_hz);
}
inline std::vector<int16_t> ingest_tune_design_taps(const IngestRatio& r, int64_t rate_hz) { return ingest_design_taps(r, rate_hz, kTuneCutoffHz, kTuneBeta); }

// the NCO table: cs[2 i] = rint(16384 cos(2 pi i / 4096)), cs[2 i + 1] = the same of sin.  One quarter wave is computed and the rest mirrored, so that
// the quarter points and the symmetries are exact.
inline std::vector<int16_t> ingest_tune_nco()
{
  const int N = kTuneNcoSize, Q = N / 4;
  std::vector<int> s(static_cast<size_t>(N));
  for (int i = 0; i <= Q; ++i) s[static_cast<size_t>(i)] = i == Q ? 16384 : static_cast<int>(std::lrint(16384.0 * std::sin(2.0 * 3.14159265358979323846 * i / N)));
  for (int i = Q + 1; i <= 2 * Q; ++i) s[static_cast<size_t>(i)] = s[static_cast<size_t>(2 * Q - i)];
  for (int i = 2 * Q + 1; i < N; ++i) s[static_cast<size_t>(i)] = -s[static_cast<size_t>(i - 2 * Q)];
  std::vector<int16_t> cs(static_cast<size_t>(2 * N));
  for (int i = 0; i < N; ++i) {
    cs[static_cast<size_t>(2 * i)] = static_cast<int16_t>(s[static_cast<size_t>((i + Q) % N)]);
    cs[static_cast<size_t>(2 * i + 1)] = static_cast<int16_t>(s[static_cast<size_t>(i)]);
  }
  return cs;
}
// the table as the kernels hold it (k_ingest.hip, k_scan.hip, k_tii.hip): one word per entry, cos in the low half and sin in the high half
inline std::vector<uint32_t> ingest_tune_nco_words()
{
  const std::vector<int16_t> cs = ingest_tune_nco();
  std::vector<uint32_t> words(static_cast<size_t>(kTuneNcoSize));
  for (size_t i = 0; i < words.size(); ++i) words[i] = static_cast<uint16_t>(cs[2 * i]) | static_cast<uint32_t>(static_cast<uint16_t>(cs[2 * i + 1])) << 16;
  return words;
}
// may a block centred f Hz from the capture's centre be tuned to?  ("" = yes)
inline std::string ingest_tune_offset(int64_t rate_hz, int64_t f)
{
  const int64_t mag = f < -kIngestMaxRate || f > kIngestMaxRate ? kIngestMaxRate : f < 0 ? -f : f;      // beyond every rate's reach anyway
  if (2 * (mag + kTuneHalfBand) > rate_hz)
    return "offset " + std::to_string(f) + " Hz: the block's +-768000 Hz do not lie within the capture's +-" + std::to_string(rate_hz / 2) + " Hz";
  return "";
}
// step = floor((2 f 2^32 + Fin) / (2 Fin)) mod 2^32: f / Fin of a turn in 2^-32 turns, rounded to nearest
inline uint32_t ingest_tune_step(int64_t rate_hz, int64_t f)
{
  const __int128 num = static_cast<__int128>(2 * f) * (static_cast<__int128>(1) << 32) + rate_hz, den = 2 * static_cast<__int128>(rate_hz);
  __int128 q = num / den;
  if (num % den < 0) --q;                          // floor towards minus infinity
  return static_cast<uint32_t>(static_cast<unsigned __int128>(q) & 0xffffffffu);
}
// everything dabhip_ingest_create_tuned refuses before it looks for a device ("" = taken)
inline std::string ingest_tune_check(int nstreams, int64_t rate_hz, const int64_t* offsets_hz, int nchannels, IngestRatio* r)
{
  if (nchannels < 1 || nchannels > kTuneMaxChannels) return "nchannels must be 1 .. 16";
  if (!offsets_hz) return "null offsets";
  if (nstreams <= 0 || static_cast<int64_t>(nstreams) * nchannels > 65535) return "nstreams times nchannels must be 1 .. 65535";
  const std::string why = ingest_tune_ratio(rate_hz, r);
  if (!why.empty()) return why;
  for (int c = 0; c < nchannels; ++c) {
    const std::string bad = ingest_tune_offset(rate_hz, offsets_hz[c]);
    if (!bad.empty()) return bad;
  }
  return "";
}
// input samples of a stream that complete its first k outputs (k >= 1)
inline int64_t ingest_samples_for_outputs(const IngestRatio& r, int64_t k) { return (k - 1) * r.M / r.L + r.T / 2 + 1; }
// The bookkeeping of one push in the tuned mode: ingest_plan_push's, except that the automatic gain is measured on OUTPUTS -- the window stays open,
// and everything is carried, until the pushed input completes output W - 1.
inline IngestPush ingest_tune_plan_push(const IngestRatio& r, IngestStreamState& s, int64_t nsamples)
{
  if (!s.window_open || ingest_outputs_complete(r, s.pushed + nsamples) >= kIngestGainWindow) return ingest_plan_push(r, s, nsamples);
  IngestPush p;
  p.carry_from = s.kept_from;
  p.carry = s.pushed - s.kept_from;
  p.new_from = s.pushed;
  s.pushed += nsamples;
  p.end = s.pushed;
  p.first_out = s.produced;
  p.keep = s.pushed;                               // keep_from = 0
  s.kept_from = 0;
  return p;
}

}  // namespace dabhip
