// rs_code.hpp — the Reed-Solomon codes over GF(256) by 0x11D whose errors the GPU corrects: RS(120,110) of the DAB+ superframes (k_dabplus.hip)
// and RS(204,188) of the packet mode's FEC frames (k_packet.hip) and of the MPEG-2 TS sub-channels (k_ts.hip); both shortened from RS(255, .) with
// the generator prod (x + alpha^i), i = 0 .. kRoots - 1 (first consecutive root 0).  The field, the tables the kernels keep in LDS, the
// bounded-distance decoder of one word, and of the syndrome kernels the Horner step and the packing of their result.  Each stage keeps its sizes
// (dabplus.hpp, packet_sync.hpp), its addressing and its kernels; what else those kernels have in common (the table loads, the decode kernels'
// "does any lane need the tables" and their unpacking) stays in them, because as functions here each changed the code of a kernel it went
// into (one Reed-Solomon text).  Free of the HIP runtime: the kernels, the synthetic modulator (synth.cpp, through gf_build) and
// tests/host_sanitize/rs_units.cpp, a plain g++ program, run this text.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define DABHIP_RS_HD __host__ __device__
#else
#define DABHIP_RS_HD
#endif

namespace dabhip {

// GF(256) with x^8+x^4+x^3+x^2+1 (0x11D), alpha = 0x02
struct GfTables {
  uint8_t exp[512];                         // doubled: exp[a + b] for log sums up to 508 needs no modulo
  int16_t log[256];                         // log[0] = -1
};
inline void gf_build(GfTables& t)
{
  int x = 1;
  for (int i = 0; i < 255; ++i) {
    t.exp[i] = t.exp[i + 255] = static_cast<uint8_t>(x);
    t.log[x] = static_cast<int16_t>(i);
    x <<= 1;
    if (x & 0x100) x ^= 0x11d;
  }
  t.exp[510] = t.exp[0];
  t.exp[511] = t.exp[1];
  t.log[0] = -1;
}

// The tables of a code with kRoots generator roots, as the kernels hold them in LDS: mul[i][x] = x alpha^i (the syndromes' Horner steps and the
// Chien search's term updates), exp (doubled) and log.  Filled on the host and uploaded as they are.
template <int kRoots>
struct GfRs {
  uint8_t mul[kRoots][256];
  uint8_t exp[512];
  int16_t log[256];
};

template <int kRoots>
inline void rs_tables_fill(GfRs<kRoots>& g)
{
  GfTables t;
  gf_build(t);
  for (int i = 0; i < kRoots; ++i)
    for (int x = 0; x < 256; ++x) g.mul[i][x] = x ? t.exp[t.log[x] + i] : 0;
  for (int i = 0; i < 512; ++i) g.exp[i] = t.exp[i];
  for (int i = 0; i < 256; ++i) g.log[i] = t.log[i];
}

template <int kRoots>
DABHIP_RS_HD inline uint8_t gmul(const GfRs<kRoots>& g, uint8_t a, uint8_t b)
{
  return (a && b) ? g.exp[g.log[a] + g.log[b]] : 0;
}
template <int kRoots>
DABHIP_RS_HD inline uint8_t ginv(const GfRs<kRoots>& g, uint8_t a) { return g.exp[255 - g.log[a]]; }

// One Horner step of the syndromes S_i = r(alpha^i), the word's bytes taken first to last: S_i <- S_i alpha^i + b.  mul is GfRs::mul.
template <int kRoots>
DABHIP_RS_HD inline void rs_horner(const uint8_t* mul, uint32_t (&S)[kRoots], uint32_t b)
{
  S[0] ^= b;
#pragma unroll
  for (int i = 1; i < kRoots; ++i) S[i] = mul[i * 256 + S[i]] ^ b;
}

// The syndromes as a syndrome kernel leaves them for its decode kernel: four to a word, S_0 lowest, in the 16 bytes of scratch a code word has.
// (The decode kernels take them apart again as S8[i] = byte i & 3 of word i >> 2.)
template <int kRoots>
DABHIP_RS_HD inline void rs_pack(const uint32_t (&S)[kRoots], uint32_t* o)
{
  static_assert(kRoots <= 16 && kRoots % 2 == 0, "a code word has 16 bytes of scratch; the last word is full or half full");
#pragma unroll
  for (int w = 0; w < kRoots / 4; ++w) o[w] = S[4 * w] | (S[4 * w + 1] << 8) | (S[4 * w + 2] << 16) | (S[4 * w + 3] << 24);
  if constexpr (kRoots % 4 == 2) o[kRoots / 4] = S[kRoots - 2] | (S[kRoots - 1] << 8);
}

// Error path of one code word of kN bytes with syndromes S (not all zero): the unique code word within distance kT, if there is one.  Returns the
// symbols corrected (1..kT) with their positions and error values, or -1.  static, not inline: with internal linkage and no inline hint each
// decode kernel compiles to what it did while it had this text to itself.
template <int kN, int kRoots, int kT>
static DABHIP_RS_HD int rs_solve(const GfRs<kRoots>& g, const uint8_t (&S)[kRoots], int (&pos)[kT], uint8_t (&val)[kT])
{
  // Berlekamp-Massey (Massey's form: B kept as b^-1 x^m B), every index a constant once unrolled
  uint8_t lam[kRoots + 1] = {1}, B[kRoots + 1] = {1};
  int L = 0;
#pragma unroll
  for (int n = 0; n < kRoots; ++n) {
    uint8_t d = 0;
#pragma unroll
    for (int i = 0; i <= n; ++i) d ^= gmul(g, lam[i], S[n - i]);
#pragma unroll
    for (int i = kRoots; i >= 1; --i) B[i] = B[i - 1];
    B[0] = 0;
    if (d) {
      uint8_t Tn[kRoots + 1];
#pragma unroll
      for (int i = 0; i <= kRoots; ++i) Tn[i] = lam[i] ^ gmul(g, d, B[i]);
      if (2 * L <= n) {
        const uint8_t di = ginv(g, d);
#pragma unroll
        for (int i = 0; i <= kRoots; ++i) B[i] = gmul(g, di, lam[i]);
        L = n + 1 - L;
      }
#pragma unroll
      for (int i = 0; i <= kRoots; ++i) lam[i] = Tn[i];
    }
  }
  int deg = 0;
#pragma unroll
  for (int i = 1; i <= kRoots; ++i)
    if (lam[i]) deg = i;
  if (deg > kT || deg != L) return -1;
  // Chien search over the kN live positions: byte k is the coefficient of x^(kN - 1 - k); it is in error iff lambda(alpha^-(kN-1-k)) = 0.
  // term[i] = lam[i] alpha^(-(kN-1-k) i), stepped by alpha^i per position.  A root among the 255 - kN shortened positions leaves the count short.
  uint8_t term[kT + 1];
#pragma unroll
  for (int i = 0; i <= kT; ++i) term[i] = lam[i] ? g.exp[(g.log[lam[i]] + (255 - ((kN - 1) * i) % 255)) % 255] : 0;
  int nroots = 0;
  for (int k = 0; k < kN; ++k) {
    uint8_t v = 0;
#pragma unroll
    for (int i = 0; i <= kT; ++i) v ^= term[i];
    if (v == 0) {
      if (nroots < kT) {
#pragma unroll
        for (int r = 0; r < kT; ++r)
          if (r == nroots) pos[r] = k;
      }
      ++nroots;
    }
#pragma unroll
    for (int i = 1; i <= kT; ++i) term[i] = g.mul[i][term[i]];
  }
  if (nroots != deg) return -1;
  // Forney, first consecutive root 0: e = X omega(X^-1) / lambda'(X^-1), omega = S lambda mod x^kRoots
  uint8_t om[kRoots];
#pragma unroll
  for (int i = 0; i < kRoots; ++i) {
    uint8_t o = 0;
#pragma unroll
    for (int j = 0; j <= i && j <= kT; ++j) o ^= gmul(g, S[i - j], lam[j]);
    om[i] = o;
  }
  uint8_t chk[kRoots];
#pragma unroll
  for (int i = 0; i < kRoots; ++i) chk[i] = S[i];
#pragma unroll
  for (int r = 0; r < kT; ++r) {
    if (r >= deg) break;
    const int p = kN - 1 - pos[r];
    const uint8_t X = g.exp[p], Xi = g.exp[255 - p];
    uint8_t num = 0, den = 0, xp = 1;
#pragma unroll
    for (int i = 0; i < kRoots; ++i) {               // xp = Xi^i
      num ^= gmul(g, om[i], xp);
      if ((i & 1) && i <= kT) den ^= gmul(g, lam[i], g.exp[(g.log[Xi] * (i - 1)) % 255]);
      xp = gmul(g, xp, Xi);
    }
    if (!den) return -1;
    const uint8_t e = gmul(g, X, gmul(g, num, ginv(g, den)));
    // An early exit only, it cannot change a result: were some e zero and the check below still passed, fewer than deg errors would explain the
    // syndromes, Berlekamp-Massey would have returned L < deg, and deg != L has ruled that out above.
    if (!e) return -1;
    val[r] = e;
    uint8_t xq = e;                                  // the corrected word's syndromes: S_i + sum e X^i
#pragma unroll
    for (int i = 0; i < kRoots; ++i) {
      chk[i] ^= xq;
      xq = gmul(g, xq, X);
    }
  }
  uint8_t any = 0;
#pragma unroll
  for (int i = 0; i < kRoots; ++i) any |= chk[i];
  return any ? -1 : deg;
}

}  // namespace dabhip
