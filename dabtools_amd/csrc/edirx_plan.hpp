// edirx_plan.hpp — the rules of the EDI receiving stage (dabhip.h: dabhip_edirx, in words) as pure functions, free of HIP: what makes a packet
// (edirx_check_packet), the window over sequence numbers fed one packet at a time (edirx_window_step, edirx_flush), m_max, the erasure positions
// of a code word, the TAG walk (edirx_walk) and the rebuild of the ETI(NI) frame (edirx_rebuild).  The kernels (k_edirx.hip, through edirx.hpp),
// the host object (edirx.cpp) and tests/host_sanitize/edirx_units.cpp compile this text; tests/edirx_model.py restates it in numpy.
#pragma once

#include <cstdint>

#include "edi_plan.hpp"

namespace dabhip {

constexpr int kEdirxMaxDepth = 16;
constexpr int kEdirxMaxFcount = 256, kEdirxMaxPlen = 1472, kEdirxMaxWords = 32;
constexpr int kEdirxMaxPayload = 8160 + 256;           // of one group: 32 code words of 255 bytes and the padding behind them
// A group's bytes in the work buffer and in the carry: the payload at its final place (AF: the packet; PFT: fragment i at i PLEN; FEC: the RS
// block, byte j of fragment i at j f + i), and from kEdirxTail on the last fragment of a PFT group without FEC, whose place is known only once
// another fragment has told the common PLEN.
constexpr int kEdirxTail = 8448;
constexpr int kEdirxStride = kEdirxTail + kEdirxMaxPlen;   // 9920
constexpr int kEdirxMaxPushPackets = 1 << 21;

enum EdirxKind : int { kEdirxBad = 0, kEdirxAf = 1, kEdirxPf = 2, kEdirxPfFec = 3 };
enum EdirxCounter : int {
  kEdirxCntPackets, kEdirxCntBadPackets, kEdirxCntLate, kEdirxCntDuplicates, kEdirxCntMismatched, kEdirxCntMissing,
  kEdirxCntIncomplete, kEdirxCntRsFailed, kEdirxCntCrcFailed, kEdirxCntRefused,
  kEdirxCntWordsFilled, kEdirxCntErasuresFilled, kEdirxCntItemsIgnored, kEdirxCntWithAtst, kEdirxCntFrames, kEdirxCntN = 15
};

DABHIP_EDI_HD inline uint32_t edirx_get16(const uint8_t* p) { return (static_cast<uint32_t>(p[0]) << 8) | p[1]; }
DABHIP_EDI_HD inline uint32_t edirx_get24(const uint8_t* p) { return (static_cast<uint32_t>(p[0]) << 16) | edirx_get16(p + 1); }
DABHIP_EDI_HD inline uint32_t edirx_get32(const uint8_t* p) { return (edirx_get16(p) << 16) | edirx_get16(p + 2); }

// ---- a packet ---------------------------------------------------------------------------------------------------------------------------------
struct EdirxHdr {
  int32_t kind;                                        // EdirxKind; kEdirxBad: dropped, the other fields 0
  int32_t q;                                           // SEQ / PSEQ
  int32_t findex, fcount;                              // AF: 0, 1
  int32_t plen;                                        // payload bytes; AF: the whole packet
  int32_t rsk, rsz;
  int32_t head;                                        // bytes in front of the payload: 0 (AF), 14, 16
};
static_assert(sizeof(EdirxHdr) == 32, "EdirxHdr layout");

// the n bytes of a datagram; never reads past n
DABHIP_EDI_HD inline EdirxHdr edirx_check_packet(const uint8_t* p, int64_t n)
{
  EdirxHdr h = {};
  if (n < 12) return h;
  if (p[0] == 'A' && p[1] == 'F') {
    if (static_cast<int64_t>(edirx_get32(p + 2)) + kEdiAfOver != n || (p[8] & 0xF0) != 0x90 || p[9] != 'T') return h;
    h.q = static_cast<int32_t>(edirx_get16(p + 6));
    h.fcount = 1;
    h.plen = static_cast<int32_t>(n);
    h.kind = kEdirxAf;
    return h;
  }
  if (p[0] != 'P' || p[1] != 'F' || n < 14) return h;
  const uint32_t word = edirx_get16(p + 10);
  const int fec = word >> 15, plen = word & 0x3FFF, head = fec ? 16 : 14;
  if (n != head + plen || (word & 0x4000) || plen < 1 || plen > kEdirxMaxPlen) return h;
  const uint32_t findex = edirx_get24(p + 4), fcount = edirx_get24(p + 7);
  if (fcount < 1 || fcount > kEdirxMaxFcount || findex >= fcount) return h;
  if (edi_crc16(p, head - 2) != edirx_get16(p + head - 2)) return h;
  int rsk = 0, rsz = 0;
  if (fec) {
    rsk = p[12];
    rsz = p[13];
    if (rsk < 1 || rsk > kEdiRsK) return h;
    const int c = static_cast<int>(fcount) * plen / (rsk + kEdiRsP);
    if (c < 1 || c > kEdirxMaxWords || rsz >= c) return h;
  }
  h.q = static_cast<int32_t>(edirx_get16(p + 2));
  h.findex = static_cast<int32_t>(findex);
  h.fcount = static_cast<int32_t>(fcount);
  h.plen = plen;
  h.rsk = rsk;
  h.rsz = rsz;
  h.head = head;
  h.kind = fec ? kEdirxPfFec : kEdirxPf;
  return h;
}

// ---- the window ---------------------------------------------------------------------------------------------------------------------------------
struct EdirxGroup {
  int32_t used, seq, kind, fcount;
  int32_t plen;                                        // FEC: of every fragment.  PFT: of the fragments but the last, 0 while none is held
  int32_t rsk, rsz;
  int32_t nrecv;
  int32_t last_plen;                                   // PFT: of fragment fcount - 1 when fcount > 1, -1 while it is not held
  int32_t bad;                                         // PFT: two fragments but the last disagree on PLEN
  int32_t local;                                       // the kernels': its index among the groups its stream touches in this push, -1: none yet
  int32_t carried;                                     // the kernels': it was open when this push began (its bytes lie in the carry)
  uint64_t mask[4];                                    // the FINDEX held
};
static_assert(sizeof(EdirxGroup) == 80, "EdirxGroup layout");

struct EdirxStream {
  int32_t started, next;
  EdirxGroup open[kEdirxMaxDepth];                     // the first `depth` are used; a group's place here is its place in the carry
};
static_assert(sizeof(EdirxStream) == 8 + 80 * kEdirxMaxDepth, "EdirxStream layout");

DABHIP_EDI_HD inline bool edirx_held(const uint64_t mask[4], int i) { return (mask[i >> 6] >> (i & 63)) & 1; }
DABHIP_EDI_HD inline int edirx_m_max(int rsk, int fcount) { return kEdiRsP / ((rsk + kEdiRsP + fcount - 1) / fcount); }
DABHIP_EDI_HD inline bool edirx_ready(const EdirxGroup& g)
{
  if (g.kind == kEdirxPfFec) return g.nrecv >= g.fcount - edirx_m_max(g.rsk, g.fcount);
  return g.nrecv == g.fcount;
}
// A complete PFT group without FEC that cannot be an AF packet: fragments but the last of unequal PLEN, a last one longer than they, or more
// bytes than a group may have
DABHIP_EDI_HD inline bool edirx_pft_refused(const EdirxGroup& g)
{
  if (g.kind != kEdirxPf || g.fcount == 1) return false;
  return g.bad || g.last_plen > g.plen || (g.fcount - 1) * g.plen + g.last_plen > kEdirxMaxPayload;
}
// the bytes of the AF packet a ready group gives (PFT: not refused)
DABHIP_EDI_HD inline int edirx_af_bytes(const EdirxGroup& g)
{
  if (g.kind == kEdirxPfFec) return g.fcount * g.plen / (g.rsk + kEdiRsP) * g.rsk - g.rsz;
  if (g.kind == kEdirxPf && g.fcount > 1) return (g.fcount - 1) * g.plen + g.last_plen;
  return g.plen;
}
// where the payload of a packet that joined its group goes among the group's kEdirxStride bytes: byte j at at + j step
DABHIP_EDI_HD inline void edirx_place(const EdirxHdr& h, int* at, int* step)
{
  *step = 1;
  *at = 0;
  if (h.kind == kEdirxPfFec) {
    *at = h.findex;
    *step = h.fcount;
  } else if (h.kind == kEdirxPf && h.fcount > 1) {
    *at = h.findex + 1 == h.fcount ? kEdirxTail : h.findex * h.plen;
  }
}

// Sink: void finalise(EdirxStream&, int entry, bool ready) is told of every group that leaves, in order, before its entry is freed.
template <class Sink>
DABHIP_EDI_HD inline void edirx_finalise(EdirxStream& st, int e, int64_t* cnt, Sink& sink)
{
  EdirxGroup& g = st.open[e];
  const bool ready = edirx_ready(g);
  if (!ready) ++cnt[kEdirxCntIncomplete];
  else if (edirx_pft_refused(g)) ++cnt[kEdirxCntRefused];
  sink.finalise(st, e, ready && !edirx_pft_refused(g));
  g.used = 0;
}

DABHIP_EDI_HD inline int edirx_find(const EdirxStream& st, int depth, int seq)
{
  for (int e = 0; e < depth; ++e)
    if (st.open[e].used && st.open[e].seq == seq) return e;
  return -1;
}

// the n sequence numbers from `next` on leave the window, in order: work bounded by the open groups
template <class Sink>
DABHIP_EDI_HD inline void edirx_leave(EdirxStream& st, int depth, int n, int64_t* cnt, Sink& sink)
{
  int gone = 0;
  for (;;) {
    int best = -1, best_d = n;
    for (int e = 0; e < depth; ++e) {
      const int d = (st.open[e].seq - st.next) & 0xFFFF;
      if (st.open[e].used && d < best_d) { best = e; best_d = d; }
    }
    if (best < 0) break;
    edirx_finalise(st, best, cnt, sink);
    ++gone;
  }
  cnt[kEdirxCntMissing] += n - gone;
  st.next = (st.next + n) & 0xFFFF;
}

// One packet, in arrival order.  Returns the entry of the group it joined (the entry may have been finalised and freed by the time this
// returns; sink.joined(st, entry) was called while it was open), or -1 when it was dropped.
template <class Sink>
DABHIP_EDI_HD inline int edirx_window_step(EdirxStream& st, int depth, const EdirxHdr& h, int64_t* cnt, Sink& sink)
{
  ++cnt[kEdirxCntPackets];
  if (h.kind == kEdirxBad) { ++cnt[kEdirxCntBadPackets]; return -1; }
  if (!st.started) { st.started = 1; st.next = h.q; }
  const int d = (h.q - st.next) & 0xFFFF;
  if (d >= 32768) { ++cnt[kEdirxCntLate]; return -1; }
  if (d >= depth) edirx_leave(st, depth, d - depth + 1, cnt, sink);
  int e = edirx_find(st, depth, h.q);
  const bool last = h.kind == kEdirxPf && h.fcount > 1 && h.findex + 1 == h.fcount;
  // the bytes the group needs once this packet lies at its place
  const int reach = h.kind == kEdirxPfFec ? h.fcount * h.plen : last ? 0 : (h.findex + 1) * h.plen;
  bool drop = false;
  if (e >= 0) {
    EdirxGroup& g = st.open[e];
    if (g.kind != h.kind || g.fcount != h.fcount || g.rsk != h.rsk || g.rsz != h.rsz || (h.kind == kEdirxPfFec && g.plen != h.plen)) { ++cnt[kEdirxCntMismatched]; drop = true; }
    else if (edirx_held(g.mask, h.findex)) { ++cnt[kEdirxCntDuplicates]; drop = true; }
  }
  if (!drop && reach > kEdirxMaxPayload) { ++cnt[kEdirxCntMismatched]; drop = true; }
  if (!drop && e < 0) {
    for (e = 0; e < depth && st.open[e].used; ++e) {}  // one is free: the open groups' numbers are distinct and lie in the window with q
    if (e == depth) { ++cnt[kEdirxCntMismatched]; drop = true; }             // (never: a guard against a state that breaks that)
  }
  if (!drop) {
    if (!st.open[e].used) {
      EdirxGroup g = {};
      g.used = 1;
      g.seq = h.q;
      g.kind = h.kind;
      g.fcount = h.fcount;
      g.rsk = h.rsk;
      g.rsz = h.rsz;
      g.plen = h.kind == kEdirxPf && h.fcount > 1 ? 0 : h.plen;
      g.last_plen = -1;
      g.local = -1;
      st.open[e] = g;
    }
    EdirxGroup& g = st.open[e];
    if (last) g.last_plen = h.plen;
    else if (h.kind == kEdirxPf && h.fcount > 1) {
      if (g.plen == 0) g.plen = h.plen;
      else if (g.plen != h.plen) g.bad = 1;
    }
    g.mask[h.findex >> 6] |= 1ull << (h.findex & 63);
    ++g.nrecv;
    sink.joined(st, e);
  } else {
    e = -1;
  }
  for (;;) {
    const int at = edirx_find(st, depth, st.next);
    if (at < 0 || st.open[at].nrecv != st.open[at].fcount) break;
    edirx_finalise(st, at, cnt, sink);
    st.next = (st.next + 1) & 0xFFFF;
  }
  return e;
}

// the open groups leave in order; next moves past the last of them
template <class Sink>
DABHIP_EDI_HD inline void edirx_flush(EdirxStream& st, int depth, int64_t* cnt, Sink& sink)
{
  int last = -1;
  for (;;) {
    int best = -1, best_d = 1 << 16;
    for (int e = 0; e < depth; ++e) {
      const int d = (st.open[e].seq - st.next) & 0xFFFF;
      if (st.open[e].used && d < best_d) { best = e; best_d = d; }
    }
    if (best < 0) break;
    last = best_d;
    edirx_finalise(st, best, cnt, sink);
  }
  if (last >= 0) st.next = (st.next + last + 1) & 0xFFFF;
}

// ---- code words -----------------------------------------------------------------------------------------------------------------------------------
// byte t (0 .. RSk + 47) of a code word among its 255: the RSk data bytes lead, the parity bytes are the last 48
DABHIP_EDI_HD inline int edirx_cw_index(int rsk, int t) { return t < rsk ? t : kEdiRsK + t - rsk; }
// The erasures of code word w of a group: the places (0 .. 254, byte j the coefficient of x^(254 - j)) of its bytes that lie in fragments not
// held, in rising order; at most 48 in a ready group.  pos may be null.  Returns their number.
DABHIP_EDI_HD inline int edirx_word_erasures(const uint64_t mask[4], int fcount, int rsk, int w, uint8_t* pos)
{
  const int cw = rsk + kEdiRsP;
  int n = 0, frag = w * cw % fcount;                    // the fragment of byte t: (w cw + t) mod fcount, counted along
  for (int t = 0; t < cw; ++t) {
    if (!edirx_held(mask, frag)) {
      if (pos) pos[n] = static_cast<uint8_t>(edirx_cw_index(rsk, t));
      ++n;
    }
    if (++frag == fcount) frag = 0;
  }
  return n;
}

// ---- the TAG walk and the ETI frame -------------------------------------------------------------------------------------------------------------
struct EdirxLayout {
  int32_t stat, fct, fcth, ficf, nst, fp, mid, mnsc, atstf, rfudf;
  int32_t fic_at;                                      // the FIC among the AF packet's bytes
  int32_t stl_sum, items_ignored, have_deti;
  int16_t est_at[kEdiMaxNst];                          // the 3 bytes SCID / SAD / TPL of entry i; its 8 STL bytes follow them
  int16_t est_stl[kEdiMaxNst];
};

// An AF packet of len bytes (12 .. kEdirxMaxPayload) whose "AF", LEN and CRC were found right.  0: fine, else refused.
DABHIP_EDI_HD inline int edirx_walk(const uint8_t* af, int len, EdirxLayout& o)
{
  o.have_deti = o.nst = o.stl_sum = o.items_ignored = 0;
  int at = kEdiAfHead;
  const int end = len - 2;
  while (end - at >= 8) {
    const uint8_t* name = af + at;
    const uint32_t bits = edirx_get32(af + at + 4);
    if ((bits & 7) || (bits >> 3) > static_cast<uint32_t>(end - at - 8)) return 1;
    const int n = static_cast<int>(bits >> 3);
    const uint8_t* v = af + at + 8;
    at += 8 + n;
    if (name[0] == '*' && name[1] == 'p' && name[2] == 't' && name[3] == 'r') {
      if (n != 8 || v[0] != 'D' || v[1] != 'E' || v[2] != 'T' || v[3] != 'I') return 2;
    } else if (name[0] == 'd' && name[1] == 'e' && name[2] == 't' && name[3] == 'i') {
      if (o.have_deti || n < 6) return 3;
      const uint32_t a = edirx_get16(v), b = edirx_get32(v + 2);
      o.atstf = a >> 15;
      o.ficf = (a >> 14) & 1;
      o.rfudf = (a >> 13) & 1;
      o.fcth = (a >> 8) & 31;
      o.fct = a & 255;
      o.stat = b >> 24;
      o.mid = (b >> 22) & 3;
      o.fp = (b >> 19) & 7;
      o.mnsc = b & 0xFFFF;
      if (n != 6 + 8 * o.atstf + kEdiFic * o.ficf + 3 * o.rfudf) return 3;
      o.fic_at = static_cast<int>(v - af) + 6 + 8 * o.atstf;
      o.have_deti = 1;
    } else if (name[0] == 'e' && name[1] == 's' && name[2] == 't') {
      if (name[3] != o.nst + 1 || o.nst >= kEdiMaxNst || n < 3 || (n - 3) % 8 || (n - 3) / 8 > 1023) return 4;
      o.est_at[o.nst] = static_cast<int16_t>(v - af);
      o.est_stl[o.nst] = static_cast<int16_t>((n - 3) / 8);
      o.stl_sum += (n - 3) / 8;
      ++o.nst;
    } else {
      ++o.items_ignored;
    }
  }
  for (; at < end; ++at)
    if (af[at]) return 5;
  if (!o.have_deti || (o.ficf && o.mid != 1)) return 6;
  if (12 + 4 * o.nst + kEdiFic * o.ficf + 8 * o.stl_sum > kEdiMstEnd) return 7;
  return 0;
}

// bytes 0 .. 11 + 4 NST of the frame: STAT, FSYNC, FCT, FICF | NST, FP | MID | FL, the STC entries, MNSC and the HCRC.  Returns 12 + 4 NST.
DABHIP_EDI_HD inline int edirx_eti_header(const uint8_t* af, const EdirxLayout& o, uint8_t* f)
{
  const bool odd = o.fct & 1;
  f[0] = static_cast<uint8_t>(o.stat);
  f[1] = odd ? 0xF8 : 0x07;
  f[2] = odd ? 0xC5 : 0x3A;
  f[3] = odd ? 0x49 : 0xB6;
  f[4] = static_cast<uint8_t>(o.fct);
  f[5] = static_cast<uint8_t>((o.ficf << 7) | o.nst);
  const int fl = o.nst + 1 + 24 * o.ficf + 2 * o.stl_sum;
  f[6] = static_cast<uint8_t>((o.fp << 5) | (o.mid << 3) | (fl >> 8));
  f[7] = static_cast<uint8_t>(fl);
  for (int i = 0; i < o.nst; ++i) {
    const uint32_t w = edirx_get24(af + o.est_at[i]);
    edi_put32(f + 8 + 4 * i, ((w >> 18) << 26) | (((w >> 8) & 0x3FF) << 16) | (((w >> 2) & 0x3F) << 10) | static_cast<uint32_t>(o.est_stl[i]));
  }
  edi_put16(f + 8 + 4 * o.nst, static_cast<uint32_t>(o.mnsc));
  edi_put16(f + 10 + 4 * o.nst, edi_crc16(f + 4, 6 + 4 * o.nst));
  return 12 + 4 * o.nst;
}

// the whole frame, byte by byte (the kernel builds the same in parallel)
DABHIP_EDI_HD inline void edirx_rebuild(const uint8_t* af, const EdirxLayout& o, uint8_t* f)
{
  const int mst0 = edirx_eti_header(af, o, f);
  int at = mst0;
  if (o.ficf)
    for (int i = 0; i < kEdiFic; ++i) f[at++] = af[o.fic_at + i];
  for (int e = 0; e < o.nst; ++e)
    for (int i = 0; i < 8 * o.est_stl[e]; ++i) f[at++] = af[o.est_at[e] + 3 + i];
  edi_put16(f + at, edi_crc16(f + mst0, at - mst0));
  for (int i = 2; i < 8 && at + i < kEdiEti; ++i) f[at + i] = 0xFF;      // a main stream that ends past byte 6136 leaves no room for all six
  for (at += 8; at < kEdiEti; ++at) f[at] = 0x55;
}

// log and antilog of GF(256) by 0x11D, alpha = 2: exp[0 .. 509] (doubled, so that a sum of two logs needs no reduction), log[1 .. 255]
inline void edirx_gf_fill(uint8_t* exp512, uint8_t* log256)
{
  uint8_t x = 1;
  log256[0] = 0;
  for (int i = 0; i < 255; ++i) {
    exp512[i] = exp512[i + 255] = x;
    log256[x] = static_cast<uint8_t>(i);
    x = edi_gmul(x, 2);
  }
  exp512[510] = exp512[0];
  exp512[511] = exp512[1];
}

}  // namespace dabhip
