// tune_units.cpp — the tuned mode's host rule (csrc/ingest_plan.hpp) as a stand-alone program under -fsanitize=address,undefined
// (tests/test_tune_model.py builds and runs it).  The refusals, the step rule against its defining inequality, and random pushes per rate: the carry,
// the push's samples and the outputs of two channels live in arrays of EXACTLY the planned sizes, and a straightforward host rendering of the
// arithmetic (mixer, tuned table, energy over outputs) reads and writes them the way the kernel's descriptors say: an index outside what the plan
// promised is an overrun the sanitizer reports.  The bytes and gains are compared with a one-shot run of the same rendering.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../dabtools_amd/csrc/ingest_plan.hpp"

using namespace dabhip;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace {
constexpr int kChannels = 2;
struct Stream {
  IngestRatio r;
  std::vector<int16_t> taps, nco;
  IngestStreamState st;
  std::vector<int16_t> carry;      // exactly plan.keep samples (I, Q), cs16: shared by the channels
  uint32_t step[kChannels] = {0, 0};
  uint32_t gain[kChannels] = {0, 0};
};

// y of sample n out of (carry, src) as the descriptors place them
inline void fetch_mixed(const Stream& s, const IngestPush& p, const std::vector<int16_t>& src, int c, int64_t n, int64_t* yi, int64_t* yq)
{
  if (n < p.carry_from || n >= p.end) { *yi = *yq = 0; return; }
  const std::vector<int16_t>& from = n < p.new_from ? s.carry : src;
  const size_t at = static_cast<size_t>(2 * (n - (n < p.new_from ? p.carry_from : p.new_from)));
  const int64_t xi = from.at(at), xq = from.at(at + 1);
  const uint32_t theta = static_cast<uint32_t>(static_cast<uint64_t>(n)) * s.step[c];
  const size_t i = static_cast<uint32_t>(theta + (1u << 19)) >> 20;
  const int64_t co = s.nco.at(2 * i), si = s.nco.at(2 * i + 1);
  const int64_t a = (xi * co + xq * si + 8192) >> 14, b = (xq * co - xi * si + 8192) >> 14;
  *yi = a < -32768 ? -32768 : a > 32767 ? 32767 : a;
  *yq = b < -32768 ? -32768 : b > 32767 ? 32767 : b;
}
inline uint8_t requant(int64_t v, uint32_t g)
{
  const int64_t o = 127 + ((v * static_cast<int64_t>(g) + 32768) >> 16);
  return static_cast<uint8_t>(o < 0 ? 0 : o > 255 ? 255 : o);
}
// v of output m of channel c
void output(const Stream& s, const IngestPush& p, const std::vector<int16_t>& src, int c, int64_t m, int64_t* vi, int64_t* vq)
{
  const int T = s.r.T, L = s.r.L, M = s.r.M;
  const int64_t n0 = m * M / L, ph = m * M % L;
  if (T == 0) {
    CHECK(m >= p.carry_from && m < p.end);
    fetch_mixed(s, p, src, c, m, vi, vq);
    return;
  }
  CHECK(n0 + T / 2 < p.end);                                      // complete
  int64_t ai = 0, aq = 0;
  for (int k = 0; k < T; ++k) {
    const int64_t n = n0 + T / 2 - k;
    CHECK(n < 0 || n >= p.carry_from);                            // within what was carried
    int64_t i, q;
    fetch_mixed(s, p, src, c, n, &i, &q);
    ai += s.taps[static_cast<size_t>(ph) * T + k] * i;
    aq += s.taps[static_cast<size_t>(ph) * T + k] * q;
  }
  CHECK(ai < (int64_t(1) << 31) && ai >= -(int64_t(1) << 31) && aq < (int64_t(1) << 31) && aq >= -(int64_t(1) << 31));
  *vi = (ai + 8192) >> 14;
  *vq = (aq + 8192) >> 14;
}

// one push of cs16 samples: the outputs it completes, per channel
std::vector<std::vector<uint8_t>> push(Stream& s, const std::vector<int16_t>& src)
{
  const bool was_open = s.st.window_open;
  const IngestPush p = ingest_tune_plan_push(s.r, s.st, static_cast<int64_t>(src.size() / 2));
  CHECK(p.carry == static_cast<int64_t>(s.carry.size() / 2) && p.new_from == p.carry_from + p.carry && p.end == p.new_from + static_cast<int64_t>(src.size() / 2));
  CHECK(p.keep_from >= p.carry_from && p.keep_from + p.keep == p.end);
  CHECK(p.closes == (was_open && ingest_outputs_complete(s.r, p.end) >= kIngestGainWindow));
  CHECK(!(was_open && !p.closes) || (p.nout == 0 && p.keep == p.end && p.end < ingest_samples_for_outputs(s.r, kIngestGainWindow)));
  if (p.closes) {
    CHECK(p.first_out == 0 && p.nout >= kIngestGainWindow && p.carry_from == 0);
    for (int c = 0; c < kChannels; ++c) {
      uint64_t e = 0;
      for (int64_t m = 0; m < kIngestGainWindow; ++m) {
        int64_t vi, vq;
        output(s, p, src, c, m, &vi, &vq);
        e += static_cast<uint64_t>(vi * vi + vq * vq);
      }
      s.gain[c] = ingest_auto_gain(e);
      CHECK(s.gain[c] >= 1 && s.gain[c] <= kIngestMaxGain);
    }
  }
  std::vector<std::vector<uint8_t>> out(kChannels, std::vector<uint8_t>(static_cast<size_t>(2 * p.nout)));
  for (int c = 0; c < kChannels; ++c) {
    CHECK(p.nout == 0 || s.gain[c] != 0);
    for (int64_t o = 0; o < p.nout; ++o) {
      int64_t vi, vq;
      output(s, p, src, c, p.first_out + o, &vi, &vq);
      out[static_cast<size_t>(c)].at(static_cast<size_t>(2 * o)) = requant(vi, s.gain[c]);
      out[static_cast<size_t>(c)].at(static_cast<size_t>(2 * o + 1)) = requant(vq, s.gain[c]);
    }
  }
  std::vector<int16_t> keep(static_cast<size_t>(2 * p.keep));       // exactly what the plan says is carried: the samples as they came, not y
  for (int64_t j = 0; j < p.keep; ++j) {
    const int64_t n = p.keep_from + j;
    const std::vector<int16_t>& from = n < p.new_from ? s.carry : src;
    const size_t at = static_cast<size_t>(2 * (n - (n < p.new_from ? p.carry_from : p.new_from)));
    keep.at(static_cast<size_t>(2 * j)) = from.at(at);
    keep.at(static_cast<size_t>(2 * j + 1)) = from.at(at + 1);
  }
  s.carry.swap(keep);
  return out;
}

Stream make(int64_t rate, uint32_t gain, const int64_t* offsets)
{
  Stream s;
  CHECK(ingest_tune_check(1, rate, offsets, kChannels, &s.r).empty());
  if (!s.r.bypass()) {
    s.taps = ingest_tune_design_taps(s.r, rate);
    CHECK(ingest_check_taps(s.r, s.taps.data()).empty());
    CHECK(ingest_tune_lds_bytes(s.r) <= kTuneMaxLdsBytes && s.r.tile_span() > s.r.T);
  }
  s.nco = ingest_tune_nco();
  CHECK(s.nco.size() == 2 * static_cast<size_t>(kTuneNcoSize));
  for (int c = 0; c < kChannels; ++c) { s.step[c] = ingest_tune_step(rate, offsets[c]); s.gain[c] = gain; }
  s.st.window_open = gain == 0;
  return s;
}

void refusals()
{
  IngestRatio r;
  const int64_t zero[17] = {0};
  CHECK(!ingest_tune_check(1, 10000000, zero, 0, &r).empty() && !ingest_tune_check(1, 10000000, zero, 17, &r).empty());
  CHECK(ingest_tune_check(1, 10000000, zero, 1, &r).empty() && ingest_tune_check(4095, 10000000, zero, 16, &r).empty() && r.T == 320);
  CHECK(!ingest_tune_check(4096, 10000000, zero, 16, &r).empty() && !ingest_tune_check(0, 10000000, zero, 1, &r).empty() && !ingest_tune_check(1, 10000000, nullptr, 1, &r).empty());
  for (int64_t rate : {2047999, 10240001, 2400001, 10229760}) CHECK(!ingest_tune_check(1, rate, zero, 1, &r).empty());
  CHECK(ingest_ratio(10229760, &r).empty());                          // the plain path takes it: it is the tuned table that does not fit
  const int64_t edge[2] = {4232000, -4232000}, past[2] = {0, 4232001}, wild[1] = {INT64_MIN};
  CHECK(ingest_tune_check(1, 10000000, edge, 2, &r).empty() && !ingest_tune_check(1, 10000000, past, 2, &r).empty() && !ingest_tune_check(1, 10000000, wild, 1, &r).empty());
  CHECK(ingest_tune_ratio(10000000, &r).empty() && r.lds_table_bytes() == 82432 && ingest_tune_lds_bytes(r) == 82432 + 21288 + 16384);
  r.L = 1024; r.M = 5119; r.T = 320;                                   // no rate gives this one: the rule on its own
  CHECK(!ingest_tune_fits(r, 0).empty());
}

void step_rule(std::mt19937_64& rng)
{
  for (int64_t rate : {2048000, 2400000, 4096000, 8192000, 10000000, 10240000}) {
    const int64_t reach = rate / 2 - kTuneHalfBand;
    for (int k = 0; k < 2000; ++k) {
      const int64_t f = k == 0 ? reach : k == 1 ? -reach : k == 2 ? 0 : static_cast<int64_t>(rng() % static_cast<uint64_t>(2 * reach + 1)) - reach;
      CHECK(ingest_tune_offset(rate, f).empty());
      // the floor: q 2 Fin <= 2 f 2^32 + Fin < (q + 1) 2 Fin, and |f| < Fin / 2 puts q within int32
      const __int128 q = static_cast<int32_t>(ingest_tune_step(rate, f)), num = static_cast<__int128>(2 * f) * (static_cast<__int128>(1) << 32) + rate;
      CHECK(q * 2 * rate <= num && num < (q + 1) * 2 * rate);
    }
  }
}
}  // namespace

int main()
{
  std::mt19937_64 rng(13);
  refusals();
  step_rule(rng);
  for (int64_t rate : {2048000, 2400000, 2500000, 4096000, 8192000, 10000000}) {
    const int64_t reach = rate / 2 - kTuneHalfBand;
    const int64_t offsets[kChannels] = {-reach, static_cast<int64_t>(rng() % static_cast<uint64_t>(reach + 1))};
    for (uint32_t gain : {256u, 0u}) {
      IngestRatio r;
      CHECK(ingest_tune_ratio(rate, &r).empty());
      const size_t closes_at = static_cast<size_t>(ingest_samples_for_outputs(r, kIngestGainWindow));
      CHECK(ingest_outputs_complete(r, static_cast<int64_t>(closes_at)) >= kIngestGainWindow && ingest_outputs_complete(r, static_cast<int64_t>(closes_at) - 1) < kIngestGainWindow);
      const size_t n = gain ? 5000 : closes_at + 3000;
      std::vector<int16_t> all(2 * n);
      for (auto& v : all) v = static_cast<int16_t>(rng() % 3 == 0 ? (rng() & 1 ? 32767 : -32768) : static_cast<int>(rng() % 65536) - 32768);
      for (size_t i = 0; i < n && gain == 0; ++i) all[2 * i] = static_cast<int16_t>(all[2 * i] / 7);      // not symmetric: the channels' energies differ
      Stream one = make(rate, gain, offsets), cut = make(rate, gain, offsets);
      const std::vector<std::vector<uint8_t>> want = push(one, all);
      CHECK(static_cast<int64_t>(want[0].size() / 2) == ingest_outputs_complete(one.r, static_cast<int64_t>(n)) && want[1].size() == want[0].size());
      std::vector<std::vector<uint8_t>> got(kChannels);
      const bool at_end = rate % 3 != 0;                              // the window closes exactly at a push's end, or inside one
      for (size_t at = 0; at < n;) {
        const size_t kind = rng() % 8;
        size_t len = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? static_cast<size_t>(one.r.T / 2) : rng() % (gain ? 1500 : 60000);
        if (gain == 0 && at_end && at < closes_at && at + len >= closes_at) len = closes_at - at;
        if (gain == 0 && !at_end && at < closes_at && at + len == closes_at) ++len;
        len = std::min(len, n - at);
        const std::vector<int16_t> src(all.begin() + static_cast<long>(2 * at), all.begin() + static_cast<long>(2 * (at + len)));
        const std::vector<std::vector<uint8_t>> o = push(cut, src);
        for (int c = 0; c < kChannels; ++c) got[static_cast<size_t>(c)].insert(got[static_cast<size_t>(c)].end(), o[static_cast<size_t>(c)].begin(), o[static_cast<size_t>(c)].end());
        at += len;
      }
      for (int c = 0; c < kChannels; ++c) CHECK(got[static_cast<size_t>(c)] == want[static_cast<size_t>(c)] && cut.gain[c] == one.gain[c]);
      // skip: the positions behind it are those of as many pushed samples, and the phase goes on from there
      if (gain) {
        Stream a = make(rate, gain, offsets);
        const int64_t far = (int64_t(1) << 32) - 1000, through = ingest_skip_through(a.r, far);
        push(a, std::vector<int16_t>(static_cast<size_t>(2 * through), 0));
        ingest_skip_rest(a.r, a.st, far - through);
        a.carry.assign(static_cast<size_t>(2 * (a.st.pushed - a.st.kept_from)), 0);      // zeros all of them
        CHECK(a.st.pushed == far && a.st.produced == ingest_outputs_complete(a.r, far));
        const std::vector<int16_t> src(all.begin(), all.begin() + 6000);                   // 3000 samples across 2^32
        const std::vector<std::vector<uint8_t>> o = push(a, src);
        CHECK(static_cast<int64_t>(o[0].size() / 2) == ingest_outputs_complete(a.r, far + 3000) - ingest_outputs_complete(a.r, far));
      }
    }
  }
  std::puts("ok tune-units");
  return 0;
}
