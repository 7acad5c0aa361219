// ingest_units.cpp — the ingest stage's host rule (csrc/ingest_plan.hpp) as a stand-alone program under -fsanitize=address,undefined
// (tests/test_ingest_model.py builds and runs it).  Random pushes per rate; the carry, the push's samples and the outputs live in byte arrays of
// EXACTLY the planned sizes, and a straightforward host rendering of the arithmetic reads and writes them the way the kernel's descriptors say:
// an index outside what the plan promised is an overrun the sanitizer reports.  The bytes are compared with a one-shot run of the same rendering.
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
struct Stream {
  IngestRatio r;
  std::vector<int16_t> taps;
  IngestStreamState st;
  std::vector<int16_t> carry;      // exactly plan.keep samples (I, Q), cs16
  uint32_t gain = 0;
};

// sample n out of (carry, src) as the descriptors place them
inline void fetch(const IngestPush& p, const std::vector<int16_t>& carry, const std::vector<int16_t>& src, int64_t n, int64_t* i, int64_t* q)
{
  if (n < p.carry_from || n >= p.end) { *i = *q = 0; return; }
  const std::vector<int16_t>& from = n < p.new_from ? carry : src;
  const size_t at = static_cast<size_t>(2 * (n - (n < p.new_from ? p.carry_from : p.new_from)));
  *i = from.at(at);
  *q = from.at(at + 1);
}
inline uint8_t requant(int64_t v, uint32_t g)
{
  const int64_t o = 127 + ((v * static_cast<int64_t>(g) + 32768) >> 16);
  return static_cast<uint8_t>(o < 0 ? 0 : o > 255 ? 255 : o);
}

// one push of cs16 samples: returns the outputs it completes
std::vector<uint8_t> push(Stream& s, const std::vector<int16_t>& src)
{
  const IngestPush p = ingest_plan_push(s.r, s.st, static_cast<int64_t>(src.size() / 2));
  CHECK(p.carry == static_cast<int64_t>(s.carry.size() / 2) && p.new_from == p.carry_from + p.carry && p.end == p.new_from + static_cast<int64_t>(src.size() / 2));
  CHECK(p.keep_from >= p.carry_from && p.keep_from + p.keep == p.end);
  if (p.closes) {
    uint64_t e = 0;
    for (int64_t n = 0; n < kIngestGainWindow; ++n) {
      int64_t i, q;
      CHECK(n >= p.carry_from && n < p.end);
      fetch(p, s.carry, src, n, &i, &q);
      e += static_cast<uint64_t>(i * i + q * q);
    }
    s.gain = ingest_auto_gain(e);
    CHECK(s.gain >= 1 && s.gain <= kIngestMaxGain);
  }
  std::vector<uint8_t> out(static_cast<size_t>(2 * p.nout));
  const int T = s.r.T, L = s.r.L, M = s.r.M;
  for (int64_t o = 0; o < p.nout; ++o) {
    const int64_t m = p.first_out + o, n0 = m * M / L, ph = m * M % L;
    int64_t ai = 0, aq = 0, vi, vq;
    if (T == 0) {
      CHECK(m >= p.carry_from && m < p.end);
      fetch(p, s.carry, src, m, &vi, &vq);
    } else {
      CHECK(n0 + T / 2 < p.end);                                    // complete
      for (int k = 0; k < T; ++k) {
        const int64_t n = n0 + T / 2 - k;
        CHECK(n < 0 || n >= p.carry_from);                          // within what was carried
        int64_t i, q;
        fetch(p, s.carry, src, n, &i, &q);
        ai += s.taps[static_cast<size_t>(ph) * T + k] * i;
        aq += s.taps[static_cast<size_t>(ph) * T + k] * q;
      }
      CHECK(ai < (int64_t(1) << 31) && ai >= -(int64_t(1) << 31) && aq < (int64_t(1) << 31) && aq >= -(int64_t(1) << 31));
      vi = (ai + 8192) >> 14;
      vq = (aq + 8192) >> 14;
    }
    out.at(static_cast<size_t>(2 * o)) = requant(vi, s.gain);
    out.at(static_cast<size_t>(2 * o + 1)) = requant(vq, s.gain);
  }
  CHECK(p.nout == 0 || s.gain != 0);
  std::vector<int16_t> keep(static_cast<size_t>(2 * p.keep));       // exactly what the plan says is carried
  for (int64_t j = 0; j < p.keep; ++j) {
    int64_t i, q;
    fetch(p, s.carry, src, p.keep_from + j, &i, &q);
    keep.at(static_cast<size_t>(2 * j)) = static_cast<int16_t>(i);
    keep.at(static_cast<size_t>(2 * j + 1)) = static_cast<int16_t>(q);
  }
  s.carry.swap(keep);
  return out;
}

Stream make(int64_t rate, uint32_t gain)
{
  Stream s;
  CHECK(ingest_ratio(rate, &s.r).empty());
  if (!s.r.bypass()) {
    s.taps = ingest_design_taps(s.r, rate);
    CHECK(ingest_check_taps(s.r, s.taps.data()).empty());
    CHECK(s.r.lds_table_bytes() <= kIngestMaxTableBytes && s.r.tile_span() > s.r.T);
  }
  s.gain = gain;
  s.st.window_open = gain == 0;
  return s;
}
}  // namespace

int main()
{
  std::mt19937_64 rng(12);
  IngestRatio r;
  CHECK(!ingest_ratio(2047999, &r).empty() && !ingest_ratio(10240001, &r).empty() && !ingest_ratio(2400001, &r).empty());
  for (int64_t rate : {2048000, 2400000, 2500000, 2560000, 2880000, 3000000, 3200000, 4096000, 6000000, 8000000, 8192000, 10000000, 10240000}) {
    for (uint32_t gain : {256u, 0u}) {
      const size_t n = gain ? 6000 : static_cast<size_t>(kIngestGainWindow) + 5000;
      std::vector<int16_t> all(2 * n);
      for (auto& v : all) v = static_cast<int16_t>(rng() % 3 == 0 ? (rng() & 1 ? 32767 : -32768) : static_cast<int>(rng() % 65536) - 32768);
      Stream one = make(rate, gain), cut = make(rate, gain);
      const std::vector<uint8_t> want = push(one, all);
      CHECK(static_cast<int64_t>(want.size() / 2) == ingest_outputs_complete(one.r, static_cast<int64_t>(n)));
      std::vector<uint8_t> got;
      for (size_t at = 0; at < n;) {
        const size_t kind = rng() % 8;
        size_t len = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? static_cast<size_t>(one.r.T / 2) : rng() % 3000;
        if (gain == 0 && at < static_cast<size_t>(kIngestGainWindow) && rng() % 4 == 0) len = static_cast<size_t>(kIngestGainWindow) - at;      // close exactly at a push's end
        len = std::min(len, n - at);
        const std::vector<int16_t> src(all.begin() + static_cast<long>(2 * at), all.begin() + static_cast<long>(2 * (at + len)));
        const std::vector<uint8_t> o = push(cut, src);
        got.insert(got.end(), o.begin(), o.end());
        at += len;
      }
      CHECK(got == want && cut.gain == one.gain);
      // skip: the positions behind it are those of as many pushed samples
      if (gain) {
        Stream a = make(rate, gain), b = make(rate, gain);
        const int64_t far = (int64_t(1) << 32) + 12345, through = ingest_skip_through(a.r, far);
        push(a, std::vector<int16_t>(static_cast<size_t>(2 * through), 0));
        ingest_skip_rest(a.r, a.st, far - through);
        CHECK(a.st.pushed == far && a.st.produced == ingest_outputs_complete(a.r, far) && a.st.pushed - a.st.kept_from == static_cast<int64_t>(a.carry.size() / 2));
        const std::vector<int16_t> src(all.begin(), all.begin() + 4000);
        const std::vector<uint8_t> o = push(a, src);
        // the same through a stream that really saw T zeros in front (its first outputs differ only in their phase, so compare the counts and the carry)
        CHECK(static_cast<int64_t>(o.size() / 2) == ingest_outputs_complete(a.r, far + 2000) - ingest_outputs_complete(a.r, far));
        (void)b;
      }
    }
  }
  std::puts("ok ingest-units");
  return 0;
}
