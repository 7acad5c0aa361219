// rs_units.cpp — the Reed-Solomon text of the DAB+, packet-mode and MPEG-2 TS stages (csrc/rs_code.hpp) under ASan + UBSan, as a stand-alone
// program: the tables of rs_tables_fill, the syndromes by rs_horner, their way through rs_pack and the decoder rs_solve, at both sizes the kernels
// use, (120,10,5) and (204,16,8).
//   rs_units words   one received word per line of stdin, "<code length> <hex bytes>" -> "<symbols corrected, or -1> <hex bytes after decoding>"
//   rs_units         words made here: encoded by shift-and-reduce arithmetic that shares nothing with the tables, 0 .. t + 3 errors put on them,
//                    and what the decoder may answer checked by that arithmetic.  Prints "ok rs-units" and what it saw.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../dabtools_amd/csrc/rs_code.hpp"

using namespace dabhip;

namespace {
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// One word the way a stage's two kernels take it: syndromes byte by byte, status, the 16 bytes of scratch, the solver, the corrections (here of
// every byte, the parity's too).  Returns 0 for a clean word, the symbols corrected, or -1 with the word untouched.
template <int kN, int kRoots, int kT>
int decode(const GfRs<kRoots>& g, uint8_t* word)
{
  uint32_t S[kRoots] = {0};
  for (int k = 0; k < kN; ++k) rs_horner(&g.mul[0][0], S, word[k]);
  uint32_t any = 0;
  for (int i = 0; i < kRoots; ++i) any |= S[i];
  if (!any) return 0;
  uint32_t syn[4] = {0, 0, 0, 0};
  rs_pack(S, syn);
  uint8_t S8[kRoots];
  for (int i = 0; i < kRoots; ++i) S8[i] = static_cast<uint8_t>(syn[i >> 2] >> (8 * (i & 3)));
  int pos[kT] = {0};
  uint8_t val[kT] = {0};
  const int n = rs_solve<kN, kRoots, kT>(g, S8, pos, val);
  if (n < 0) return -1;
  CHECK(n >= 1 && n <= kT);
  for (int r = 0; r < n; ++r) {
    CHECK(pos[r] >= 0 && pos[r] < kN && val[r] != 0);
    word[pos[r]] ^= val[r];
  }
  return n;
}

// ---- GF(256) by 0x11D without tables ------------------------------------------------------------------------------------------------------------
uint8_t mul_plain(uint8_t a, uint8_t b)
{
  unsigned p = 0;
  for (int i = 0; i < 8; ++i)
    if (b >> i & 1) p ^= static_cast<unsigned>(a) << i;
  for (int i = 14; i >= 8; --i)
    if (p >> i & 1) p ^= 0x11du << (i - 8);
  return static_cast<uint8_t>(p);
}

uint8_t alpha_power(int n)
{
  uint8_t x = 1;
  for (int i = 0; i < n; ++i) x = mul_plain(x, 2);
  return x;
}

// prod (x + alpha^i), i < nroots, highest degree first
std::vector<uint8_t> generator_plain(int nroots)
{
  std::vector<uint8_t> g(static_cast<size_t>(nroots) + 1, 0);
  g[0] = 1;
  for (int i = 0; i < nroots; ++i)
    for (int k = i + 1; k >= 1; --k) g[k] ^= mul_plain(g[k - 1], alpha_power(i));
  return g;
}

// the word's data bytes (all but the last nroots) -> its parity: the remainder of data(x) x^nroots by the generator, by long division
void encode_plain(std::vector<uint8_t>& word, const std::vector<uint8_t>& gen)
{
  const size_t nroots = gen.size() - 1, k = word.size() - nroots;
  std::vector<uint8_t> work(word.begin(), word.begin() + k);
  work.resize(word.size(), 0);
  for (size_t i = 0; i < k; ++i) {
    const uint8_t f = work[i];
    if (!f) continue;
    for (size_t q = 0; q <= nroots; ++q) work[i + q] ^= mul_plain(f, gen[q]);
  }
  std::copy(work.begin() + k, work.end(), word.begin() + k);
}

// word(alpha^i) = 0 for i < nroots, the first byte the highest coefficient
bool is_code_word(const std::vector<uint8_t>& word, int nroots)
{
  for (int i = 0; i < nroots; ++i) {
    const uint8_t a = alpha_power(i);
    uint8_t v = 0;
    for (uint8_t b : word) v = mul_plain(v, a) ^ b;
    if (v) return false;
  }
  return true;
}

template <int kRoots>
void check_tables(const GfRs<kRoots>& g)
{
  for (int i = 0; i < kRoots; ++i)
    for (int x = 0; x < 256; ++x) CHECK(g.mul[i][x] == mul_plain(static_cast<uint8_t>(x), alpha_power(i)));
  uint8_t a = 1;
  for (int i = 0; i < 512; ++i) {
    CHECK(g.exp[i] == a);
    if (i < 255) CHECK(g.log[a] == i);
    a = mul_plain(a, 2);
  }
  CHECK(g.log[0] == -1);
  for (int x = 1; x < 256; ++x) {
    CHECK(mul_plain(static_cast<uint8_t>(x), ginv(g, static_cast<uint8_t>(x))) == 1);
    for (int y = 0; y < 256; y += 7) CHECK(gmul(g, static_cast<uint8_t>(x), static_cast<uint8_t>(y)) == mul_plain(static_cast<uint8_t>(x), static_cast<uint8_t>(y)));
  }
}

// ---- words by construction ----------------------------------------------------------------------------------------------------------------------
struct Seen {
  long words = 0, corrected = 0, failed = 0, miscorrected = 0;
};

template <int kN, int kRoots, int kT>
Seen constructed(std::mt19937_64& rng, int nwords)
{
  GfRs<kRoots> g;
  rs_tables_fill(g);
  check_tables(g);
  const std::vector<uint8_t> gen = generator_plain(kRoots);
  constexpr int kK = kN - kRoots;
  // places every count of errors is tried on first: the word's two ends and the two sides of the data / parity border
  const int edges[4] = {0, kN - 1, kK - 1, kK};
  Seen seen;
  for (int w = 0; w < nwords; ++w) {
    std::vector<uint8_t> sent(kN);
    for (int k = 0; k < kK; ++k) sent[k] = static_cast<uint8_t>(rng());
    encode_plain(sent, gen);
    CHECK(is_code_word(sent, kRoots));
    const int ne = w % (kT + 4);                                   // 0 .. t + 3
    std::vector<int> at;
    if (w < 4 * (kT + 4))                                          // the first rounds: as many of the edges as the count allows, then random places
      for (int e = 0; e < 4 && static_cast<int>(at.size()) < ne; ++e) at.push_back(edges[(e + w / (kT + 4)) % 4]);
    while (static_cast<int>(at.size()) < ne) {
      const int k = static_cast<int>(rng() % kN);
      if (std::find(at.begin(), at.end(), k) == at.end()) at.push_back(k);
    }
    std::vector<uint8_t> rx = sent;
    for (int k : at) rx[k] ^= static_cast<uint8_t>(1 + rng() % 255);
    std::vector<uint8_t> got = rx;
    const int n = decode<kN, kRoots, kT>(g, got.data());
    ++seen.words;
    if (ne <= kT) {
      CHECK(n == ne && got == sent);
      seen.corrected += n;
      continue;
    }
    if (n < 0) {
      CHECK(got == rx);
      ++seen.failed;
      continue;
    }
    // beyond the bound the decoder may land on another code word: then on one within t of what it received, and it says how far
    CHECK(n >= 1 && n <= kT && is_code_word(got, kRoots));
    int differ = 0;
    for (int k = 0; k < kN; ++k) differ += got[k] != rx[k];
    CHECK(differ == n);
    ++seen.miscorrected;
  }
  return seen;
}

// ---- words from stdin ---------------------------------------------------------------------------------------------------------------------------
int from_stdin()
{
  GfRs<10> g120;
  GfRs<16> g204;
  rs_tables_fill(g120);
  rs_tables_fill(g204);
  char line[1024];
  while (std::fgets(line, sizeof line, stdin)) {
    int len = 0, used = 0;
    if (std::sscanf(line, "%d %n", &len, &used) != 1 || (len != 120 && len != 204)) { std::printf("FAILED bad line\n"); return 1; }
    std::vector<uint8_t> word(static_cast<size_t>(len));
    for (int k = 0; k < len; ++k) {
      unsigned v = 0;
      if (std::sscanf(line + used + 2 * k, "%2x", &v) != 1) { std::printf("FAILED short word\n"); return 1; }
      word[static_cast<size_t>(k)] = static_cast<uint8_t>(v);
    }
    const int n = len == 120 ? decode<120, 10, 5>(g120, word.data()) : decode<204, 16, 8>(g204, word.data());
    std::printf("%d ", n);
    for (uint8_t b : word) std::printf("%02x", b);
    std::printf("\n");
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc > 1 && !std::strcmp(argv[1], "words")) return from_stdin();
  std::mt19937_64 rng(120204);
  const Seen a = constructed<120, 10, 5>(rng, 4000), b = constructed<204, 16, 8>(rng, 4000);
  std::printf("ok rs-units\n");
  std::printf("rs120: %ld words, %ld symbols corrected, %ld failed, %ld miscorrected; rs204: %ld words, %ld symbols corrected, %ld failed, %ld miscorrected\n",
              a.words, a.corrected, a.failed, a.miscorrected, b.words, b.corrected, b.failed, b.miscorrected);
  return 0;
}
