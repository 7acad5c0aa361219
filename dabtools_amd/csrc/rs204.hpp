// rs204.hpp — the bounded-distance decoder of RS(204,188) over GF(256) by 0x11D, shared by the stages whose outer code it is: the enhanced
// packet mode's FEC frames (k_packet.hip) and the MPEG-2 TS sub-channels (k_ts.hip).  Device code only; the sizes are packet_sync.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "packet_sync.hpp"

namespace dabhip {

// GF(256) tables in LDS: mul[i][x] = x alpha^i (i = 0..15: the syndromes' Horner steps and the Chien search's term updates), exp (doubled) and log
struct Gf204 {
  uint8_t mul[kPkRoots][256];
  uint8_t exp[512];
  int16_t log[256];
};

__device__ inline uint8_t gmul(const Gf204& g, uint8_t a, uint8_t b)
{
  return (a && b) ? g.exp[g.log[a] + g.log[b]] : 0;
}
__device__ inline uint8_t ginv(const Gf204& g, uint8_t a) { return g.exp[255 - g.log[a]]; }

// Error path of one code word with syndromes S (not all zero): the unique code word within distance 8, if there is one.  Returns the symbols
// corrected (1..8) with their positions and error values, or -1.  (k_dabplus.hip's rs_solve at this code's sizes.)  static, not inline: with
// internal linkage and no inline hint each decode kernel compiles to what the packet stage's did while this text lay in k_packet.hip.
static __device__ int rs204_solve(const Gf204& g, const uint8_t (&S)[kPkRoots], int (&pos)[kPkT], uint8_t (&val)[kPkT])
{
  // Berlekamp-Massey (Massey's form: B kept as b^-1 x^m B), every index a constant once unrolled
  uint8_t lam[kPkRoots + 1] = {1}, B[kPkRoots + 1] = {1};
  int L = 0;
#pragma unroll
  for (int n = 0; n < kPkRoots; ++n) {
    uint8_t d = 0;
#pragma unroll
    for (int i = 0; i <= n; ++i) d ^= gmul(g, lam[i], S[n - i]);
#pragma unroll
    for (int i = kPkRoots; i >= 1; --i) B[i] = B[i - 1];
    B[0] = 0;
    if (d) {
      uint8_t Tn[kPkRoots + 1];
#pragma unroll
      for (int i = 0; i <= kPkRoots; ++i) Tn[i] = lam[i] ^ gmul(g, d, B[i]);
      if (2 * L <= n) {
        const uint8_t di = ginv(g, d);
#pragma unroll
        for (int i = 0; i <= kPkRoots; ++i) B[i] = gmul(g, di, lam[i]);
        L = n + 1 - L;
      }
#pragma unroll
      for (int i = 0; i <= kPkRoots; ++i) lam[i] = Tn[i];
    }
  }
  int deg = 0;
#pragma unroll
  for (int i = 1; i <= kPkRoots; ++i)
    if (lam[i]) deg = i;
  if (deg > kPkT || deg != L) return -1;
  // Chien search over the 204 live positions: byte k is the coefficient of x^(203 - k); it is in error iff lambda(alpha^-(203-k)) = 0.
  // term[i] = lam[i] alpha^(-(203-k) i), stepped by alpha^i per position.  A root among the 51 shortened positions leaves the count short.
  uint8_t term[kPkT + 1];
#pragma unroll
  for (int i = 0; i <= kPkT; ++i) term[i] = lam[i] ? g.exp[(g.log[lam[i]] + (255 - ((kPkN - 1) * i) % 255)) % 255] : 0;
  int nroots = 0;
  for (int k = 0; k < kPkN; ++k) {
    uint8_t v = 0;
#pragma unroll
    for (int i = 0; i <= kPkT; ++i) v ^= term[i];
    if (v == 0) {
      if (nroots < kPkT) {
#pragma unroll
        for (int r = 0; r < kPkT; ++r)
          if (r == nroots) pos[r] = k;
      }
      ++nroots;
    }
#pragma unroll
    for (int i = 1; i <= kPkT; ++i) term[i] = g.mul[i][term[i]];
  }
  if (nroots != deg) return -1;
  // Forney, first consecutive root 0: e = X omega(X^-1) / lambda'(X^-1), omega = S lambda mod x^16
  uint8_t om[kPkRoots];
#pragma unroll
  for (int i = 0; i < kPkRoots; ++i) {
    uint8_t o = 0;
#pragma unroll
    for (int j = 0; j <= i && j <= kPkT; ++j) o ^= gmul(g, S[i - j], lam[j]);
    om[i] = o;
  }
  uint8_t chk[kPkRoots];
#pragma unroll
  for (int i = 0; i < kPkRoots; ++i) chk[i] = S[i];
#pragma unroll
  for (int r = 0; r < kPkT; ++r) {
    if (r >= deg) break;
    const int p = kPkN - 1 - pos[r];
    const uint8_t X = g.exp[p], Xi = g.exp[255 - p];
    uint8_t num = 0, den = 0, xp = 1;
#pragma unroll
    for (int i = 0; i < kPkRoots; ++i) {             // xp = Xi^i
      num ^= gmul(g, om[i], xp);
      if ((i & 1) && i <= kPkT) den ^= gmul(g, lam[i], g.exp[(g.log[Xi] * (i - 1)) % 255]);
      xp = gmul(g, xp, Xi);
    }
    if (!den) return -1;
    const uint8_t e = gmul(g, X, gmul(g, num, ginv(g, den)));
    if (!e) return -1;
    val[r] = e;
    uint8_t xq = e;                                  // the corrected word's syndromes: S_i + sum e X^i
#pragma unroll
    for (int i = 0; i < kPkRoots; ++i) {
      chk[i] ^= xq;
      xq = gmul(g, xq, X);
    }
  }
  uint8_t any = 0;
#pragma unroll
  for (int i = 0; i < kPkRoots; ++i) any |= chk[i];
  return any ? -1 : deg;
}

}  // namespace dabhip
