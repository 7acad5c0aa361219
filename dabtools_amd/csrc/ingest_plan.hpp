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
inline std::vector<int16_t> ingest_design_taps(const IngestRatio& r, int64_t rate_hz)
{
  const int L = r.L, T = r.T;
  std::vector<int16_t> taps(static_cast<size_t>(L) * T);
  const double pi = 3.14159265358979323846, beta = 7.0, half = 0.5 * T * L;
  const double fc = 2.0 * 1024000.0 / (static_cast<double>(L) * static_cast<double>(rate_hz));      // cycles per prototype sample, doubled: sinc(fc i)
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

}  // namespace dabhip
