// edi_plan.hpp — the rules of the EDI stage (ETSI TS 102 693 over TS 102 821, as dabhip.h states them in words) as pure functions, free of HIP:
// what an ETI frame gives (edi_parse), the sizes of PFT (edi_plan), the packing of the AF, TAG and PF headers, the CRC-16 with its combine rule
// and the RS(255,207) generator.  The kernels (k_edi.hip, through edi.hpp), the host object (edi.cpp: dabhip_edi_plan) and
// tests/host_sanitize/edi_units.cpp run this text; tests/edi_model.py restates it in numpy.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define DABHIP_EDI_HD __host__ __device__
#else
#define DABHIP_EDI_HD
#endif

namespace dabhip {

constexpr int kEdiEti = 6144;
constexpr int kEdiMstEnd = 6140;                       // the main stream ends at or before this byte (EOF and TIST follow it)
constexpr int kEdiMaxNst = 64;
constexpr int kEdiFic = 96;
constexpr int kEdiAfHead = 10, kEdiAfOver = 12;        // "AF" LEN SEQ 0x90 "T" in front, the CRC behind
constexpr int kEdiPtrItem = 16, kEdiDetiHead = 14, kEdiEstHead = 11;
constexpr int kEdiRsN = 255, kEdiRsK = 207, kEdiRsP = 48;
constexpr int kEdiFcthMod = 20;
constexpr int kEdiMinL = 13, kEdiPlanMaxL = 1 << 20;   // what edi_plan takes
// What a frame can give: the TAG packet is 30 + 96 FICF + 11 NST + 8 sum(STL) bytes and the main stream ends at 12 + 4 NST + 96 FICF + 8 sum(STL)
// <= 6140, so the TAG packet has at most 6158 + 7 NST <= 6606 bytes, 6608 padded; l <= 6620 and c <= 32.
constexpr int kEdiMaxL = 6620;
constexpr int kEdiMaxChunks = 32;
constexpr int kEdiWorkStride = 6656;                   // a frame's AF packet in the work buffer: l bytes, then zeros up to this
// Fragments of one frame.  Mode 1: ceil(6620 / 64) = 104.  Mode 2: s_max >= min(8 c, 64) and B <= 255 c, so f <= 32 + 1 (c <= 8) or
// f <= 255 * 32 / 64 + 1 = 129.
constexpr int kEdiMaxFrags = 132;
constexpr int kEdiMinFrag = 64, kEdiMaxFrag = 1472, kEdiMaxRecover = 5;

// ---- CRC-16: x^16 + x^12 + x^5 + 1, MSB first; the packets carry the complement of the register started at 0xFFFF --------------------------
// One byte into the register: reg' = (reg x^8 + byte x^16) mod P.
DABHIP_EDI_HD inline uint16_t edi_crc_byte(uint16_t reg, uint8_t b)
{
  uint32_t r = reg ^ (static_cast<uint32_t>(b) << 8);
  for (int i = 0; i < 8; ++i) r = (r & 0x8000) ? ((r << 1) ^ 0x1021) & 0xFFFF : (r << 1) & 0xFFFF;
  return static_cast<uint16_t>(r);
}
// the register after n bytes, from `reg`
DABHIP_EDI_HD inline uint16_t edi_crc_run(uint16_t reg, const uint8_t* p, int64_t n)
{
  for (int64_t i = 0; i < n; ++i) reg = edi_crc_byte(reg, p[i]);
  return reg;
}
DABHIP_EDI_HD inline uint16_t edi_crc16(const uint8_t* p, int64_t n) { return static_cast<uint16_t>(~edi_crc_run(0xFFFF, p, n)); }
// a b mod P over GF(2)
DABHIP_EDI_HD inline uint16_t edi_crc_mulmod(uint16_t a, uint16_t b)
{
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r <<= 1;
    if (r & 0x10000) r ^= 0x11021;
    if ((b >> i) & 1) r ^= a;
  }
  return static_cast<uint16_t>(r);
}
// reg x^(8 n) mod P: the register `reg` after n zero bytes
DABHIP_EDI_HD inline uint16_t edi_crc_shift(uint16_t reg, int64_t n)
{
  uint16_t base = 0x0100, acc = 1;                     // x^8, 1
  for (; n > 0; n >>= 1) {
    if (n & 1) acc = edi_crc_mulmod(acc, base);
    base = edi_crc_mulmod(base, base);
  }
  return edi_crc_mulmod(reg, acc);
}
// The register is linear in (start value, message): run(s, A | B) = shift(run(s, A), |B|) ^ run(0, B), and run(s, A) = shift(s, |A|) ^ run(0, A).
// So the pieces of a message are run from 0 side by side and combined: XOR of shift(run(0, piece), bytes behind it), and shift(s, all bytes).
// The split the assemble kernel makes of n bytes: 64 pieces of edi_crc_piece(n) bytes, piece i ending at n - (63 - i) pieces (the first ones
// short or empty), so that every piece is shifted by a whole number of pieces.  The start value 0xFFFF is the complement of the first two bytes.
DABHIP_EDI_HD inline int edi_crc_piece(int n) { return (n + 63) / 64; }
DABHIP_EDI_HD inline uint16_t edi_crc_combine(uint16_t reg_a, uint16_t raw_b, int64_t len_b) { return static_cast<uint16_t>(edi_crc_shift(reg_a, len_b) ^ raw_b); }

// ---- GF(256) by 0x11D, alpha = 2; g(x) = prod (x + alpha^i), i = 0..47 --------------------------------------------------------------------------
DABHIP_EDI_HD inline uint8_t edi_gmul(uint8_t a, uint8_t b)
{
  uint32_t r = 0, x = a;
  for (int i = 0; i < 8; ++i) {
    if ((b >> i) & 1) r ^= x;
    x <<= 1;
    if (x & 0x100) x ^= 0x11D;
  }
  return static_cast<uint8_t>(r);
}
// g[i] = coefficient of x^i, i = 0..48 (g[48] = 1)
inline void edi_rs_generator(uint8_t g[kEdiRsP + 1])
{
  for (int i = 0; i <= kEdiRsP; ++i) g[i] = 0;
  g[0] = 1;
  uint8_t root = 1;
  for (int d = 0; d < kEdiRsP; ++d) {                  // times (x + alpha^d)
    for (int i = d + 1; i > 0; --i) g[i] = static_cast<uint8_t>(g[i - 1] ^ edi_gmul(g[i], root));
    g[0] = edi_gmul(g[0], root);
    root = edi_gmul(root, 2);
  }
}
// The feedback table of the encoder: row v is v g(x) without its leading term, highest power first: t[48 v + j] = v g[47 - j].  With the
// remainder r[0..47] (r[0] the coefficient of x^47), a message byte d gives v = d ^ r[0], r = (r << one byte) ^ row v.
inline void edi_rs_table_fill(uint8_t* t)
{
  uint8_t g[kEdiRsP + 1];
  edi_rs_generator(g);
  for (int v = 0; v < 256; ++v)
    for (int j = 0; j < kEdiRsP; ++j) t[kEdiRsP * v + j] = edi_gmul(static_cast<uint8_t>(v), g[kEdiRsP - 1 - j]);
}
// parity of a chunk of k bytes (207 - k zero bytes behind it) through the table
inline void edi_rs_parity(const uint8_t* table, const uint8_t* chunk, int k, uint8_t par[kEdiRsP])
{
  for (int j = 0; j < kEdiRsP; ++j) par[j] = 0;
  for (int i = 0; i < kEdiRsK; ++i) {
    const uint8_t v = static_cast<uint8_t>((i < k ? chunk[i] : 0) ^ par[0]);
    const uint8_t* row = table + kEdiRsP * v;
    for (int j = 0; j + 1 < kEdiRsP; ++j) par[j] = static_cast<uint8_t>(par[j + 1] ^ row[j]);
    par[kEdiRsP - 1] = row[kEdiRsP - 1];
  }
}

// ---- what a frame gives ----------------------------------------------------------------------------------------------------------------------
struct EdiHead {
  int32_t valid;                                       // 0: skipped
  int32_t err, fct, ficf, nst, fp, mid, mnsc;
  int32_t tag_bytes;                                   // the TAG packet, padding included (LEN)
  int32_t tag_pad;
  int32_t l;                                           // the AF packet
};

DABHIP_EDI_HD inline int edi_stc_stl(const uint8_t* f, int i) { return ((f[8 + 4 * i + 2] & 3) << 8) | f[8 + 4 * i + 3]; }

// the fixed fields alone (valid, tag_bytes, tag_pad and l stay 0): nothing past byte 8 + 4 * 127 + 1 is read
DABHIP_EDI_HD inline EdiHead edi_head(const uint8_t* f)
{
  EdiHead h = {};
  h.err = f[0];
  h.fct = f[4];
  h.ficf = f[5] >> 7;
  h.nst = f[5] & 0x7F;
  h.fp = f[6] >> 5;
  h.mid = (f[6] >> 3) & 3;
  h.mnsc = (f[8 + 4 * h.nst] << 8) | f[8 + 4 * h.nst + 1];
  return h;
}

DABHIP_EDI_HD inline EdiHead edi_parse(const uint8_t* f)
{
  EdiHead h = edi_head(f);
  if (h.nst > kEdiMaxNst || (h.ficf && h.mid != 1)) return h;
  int stl_sum = 0;
  for (int i = 0; i < h.nst; ++i) stl_sum += edi_stc_stl(f, i);
  if (12 + 4 * h.nst + kEdiFic * h.ficf + 8 * stl_sum > kEdiMstEnd) return h;
  const int raw = kEdiPtrItem + kEdiDetiHead + kEdiFic * h.ficf + kEdiEstHead * h.nst + 8 * stl_sum;
  h.tag_pad = (8 - raw % 8) % 8;
  h.tag_bytes = raw + h.tag_pad;
  h.l = h.tag_bytes + kEdiAfOver;
  h.valid = 1;
  return h;
}

// ---- headers, byte by byte (big-endian fields) -------------------------------------------------------------------------------------------------
DABHIP_EDI_HD inline void edi_put16(uint8_t* p, uint32_t v) { p[0] = static_cast<uint8_t>(v >> 8); p[1] = static_cast<uint8_t>(v); }
DABHIP_EDI_HD inline void edi_put24(uint8_t* p, uint32_t v) { p[0] = static_cast<uint8_t>(v >> 16); edi_put16(p + 1, v); }
DABHIP_EDI_HD inline void edi_put32(uint8_t* p, uint32_t v) { edi_put16(p, v >> 16); edi_put16(p + 2, v); }
DABHIP_EDI_HD inline void edi_put_name(uint8_t* p, char a, char b, char c, uint8_t d, uint32_t bits)
{
  p[0] = static_cast<uint8_t>(a); p[1] = static_cast<uint8_t>(b); p[2] = static_cast<uint8_t>(c); p[3] = d;
  edi_put32(p + 4, bits);
}
// 10 bytes: "AF", LEN, SEQ, 0x90 (CRC present, major 1, minor 0), 'T'
DABHIP_EDI_HD inline void edi_put_af_head(uint8_t* p, uint32_t len, uint32_t seq)
{
  p[0] = 'A'; p[1] = 'F';
  edi_put32(p + 2, len);
  edi_put16(p + 6, seq);
  p[8] = 0x90;
  p[9] = 'T';
}
// 16 bytes: *ptr, 64 bits: "DETI", major 0, minor 0
DABHIP_EDI_HD inline void edi_put_ptr(uint8_t* p)
{
  edi_put_name(p, '*', 'p', 't', 'r', 64);
  p[8] = 'D'; p[9] = 'E'; p[10] = 'T'; p[11] = 'I';
  p[12] = p[13] = p[14] = p[15] = 0;
}
// 14 bytes: the deti item's name, length and its two fixed fields; the FIC follows when FICF
DABHIP_EDI_HD inline void edi_put_deti(uint8_t* p, const EdiHead& h, int fcth)
{
  edi_put_name(p, 'd', 'e', 't', 'i', 48 + 8 * kEdiFic * h.ficf);
  edi_put16(p + 8, (static_cast<uint32_t>(h.ficf) << 14) | (static_cast<uint32_t>(fcth) << 8) | static_cast<uint32_t>(h.fct));
  edi_put32(p + 10, (static_cast<uint32_t>(h.err) << 24) | (static_cast<uint32_t>(h.mid) << 22) | (static_cast<uint32_t>(h.fp) << 19) | static_cast<uint32_t>(h.mnsc));
}
// 11 bytes: item "est" n (1-based), its length and SCID << 18 | SAD << 8 | TPL << 2 from the 4 bytes of the STC entry; 8 STL bytes follow
DABHIP_EDI_HD inline void edi_put_est(uint8_t* p, int n, const uint8_t* stc)
{
  const uint32_t scid = stc[0] >> 2, sad = ((stc[0] & 3u) << 8) | stc[1], tpl = stc[2] >> 2, stl = ((stc[2] & 3u) << 8) | stc[3];
  edi_put_name(p, 'e', 's', 't', static_cast<uint8_t>(n), 24 + 64 * stl);
  edi_put24(p + 8, (scid << 18) | (sad << 8) | (tpl << 2));
}
// PF header with its HCRC: 12 bytes, 14 with FEC; returns the size
DABHIP_EDI_HD inline int edi_put_pf(uint8_t* p, uint32_t pseq, uint32_t findex, uint32_t fcount, int fec, uint32_t plen, uint32_t rsk, uint32_t rsz)
{
  p[0] = 'P'; p[1] = 'F';
  edi_put16(p + 2, pseq);
  edi_put24(p + 4, findex);
  edi_put24(p + 7, fcount);
  edi_put16(p + 10, (fec ? 0x8000u : 0u) | (plen & 0x3FFF));
  int n = 12;
  if (fec) {
    p[12] = static_cast<uint8_t>(rsk);
    p[13] = static_cast<uint8_t>(rsz);
    n = 14;
  }
  edi_put16(p + n, edi_crc16(p, n));
  return n + 2;
}

// ---- sizes -------------------------------------------------------------------------------------------------------------------------------------
struct EdiPlan {
  int32_t c, k, z;                                     // mode 2: chunks, bytes per chunk, zero bytes behind the packet; else 0
  int32_t B;                                           // bytes that are cut into fragments: the RS block (mode 2) or the packet
  int32_t f, s;                                        // fragments, and the PLEN of every one but (mode 1) the last
};

// What is refused: 0 fine, else which argument (1 l, 2 mode, 3 recover, 4 max_frag).  recover counts in mode 2 only, max_frag in modes 1 and 2.
DABHIP_EDI_HD inline int edi_plan_check(int64_t l, int mode, int recover, int max_frag)
{
  if (l < kEdiMinL || l > kEdiPlanMaxL) return 1;
  if (mode < 0 || mode > 2) return 2;
  if (mode == 2 && (recover < 0 || recover > kEdiMaxRecover)) return 3;
  if (mode >= 1 && (max_frag < kEdiMinFrag || max_frag > kEdiMaxFrag)) return 4;
  return 0;
}

// arguments that passed edi_plan_check
DABHIP_EDI_HD inline EdiPlan edi_plan(int32_t l, int mode, int recover, int max_frag)
{
  EdiPlan p = {0, 0, 0, l, 1, l};
  if (mode == 1) {
    p.f = (l + max_frag - 1) / max_frag;
    p.s = l < max_frag ? l : max_frag;
  } else if (mode == 2) {
    p.c = (l + kEdiRsK - 1) / kEdiRsK;
    p.k = (l + p.c - 1) / p.c;
    p.z = p.c * p.k - l;
    p.B = p.c * (p.k + kEdiRsP);
    int s_max = kEdiRsP * p.c / (recover + 1);
    if (s_max > max_frag) s_max = max_frag;
    p.f = (p.B + s_max - 1) / s_max;
    p.s = (p.B + p.f - 1) / p.f;
  }
  return p;
}

// the size of PF header i's packet and where it starts among the frame's output bytes
DABHIP_EDI_HD inline int edi_pf_head_bytes(int mode) { return mode == 0 ? 0 : mode == 1 ? 14 : 16; }
DABHIP_EDI_HD inline int32_t edi_packet_bytes(const EdiPlan& p, int mode, int32_t l, int i)
{
  if (mode == 0) return l;
  if (mode == 1) return 14 + (i + 1 < p.f ? p.s : l - p.s * (p.f - 1));
  return 16 + p.s;
}
DABHIP_EDI_HD inline int32_t edi_packet_offset(const EdiPlan& p, int mode, int i) { return i * (edi_pf_head_bytes(mode) + p.s); }
DABHIP_EDI_HD inline int32_t edi_out_bytes(const EdiPlan& p, int mode, int32_t l) { return mode == 0 ? l : mode == 1 ? 14 * p.f + l : p.f * (16 + p.s); }

// byte j of fragment i in mode 2 is byte j f + i of the RS block (0 past its end): chunk b / (k + 48), and in it data below k, parity above
DABHIP_EDI_HD inline int32_t edi_block_index(const EdiPlan& p, int i, int j) { return j * p.f + i; }

}  // namespace dabhip
