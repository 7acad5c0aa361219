// dir_figs.hpp — the rules of the ensemble directory (dabhip.h: "ensemble directory"), free of HIP: the CRC of a FIB, the strict FIG walk of one
// FIB into facts, the public records out of the kept facts, complete and resolve.  The kernels (k_dir.hip, through dir.hpp), the host object
// (dir.cpp), eti2info and tests/host_sanitize/dir_units.cpp run this text; tests/dir_model.py restates it in plain Python.
#pragma once

#include <cstdint>

#include "../../include/dabhip.h"

#ifdef __HIPCC__
#define DABHIP_DIR_HD __host__ __device__
#else
#define DABHIP_DIR_HD
#endif

namespace dabhip {

constexpr int kDirFibBytes = 32, kDirFibData = 30, kDirFicBytes = 96;
constexpr int kDirFactSlots = 32;                        // a FIB gives at most 28 facts (28 bytes of FIG 0/14)
constexpr int kDirTable = 64;                            // sub-channels, services, packet components: one entry per lane of a wave
constexpr int kDirMaxComp = 15;
constexpr int kDirNstMax = 64;

// A fact: one entry of one FIG, its fields normalised into payload bytes (big-endian, what is not kept left out), so that "the fact altered a
// kept field" is a comparison of bytes.  Payloads, and their lengths in kDirFactLen:
//   kDirEns00   EId(2) change flag, Al, CIF high, CIF low
//   kDirSub01   form, UEP index, protlev, start(2), size(2), bit rate(2)                       key = SubChId
//   kDirSvc02   the 0/2 byte, then 2 bytes per component, zeros up to 31                        key = SId, pd
//   kDirPkt03   SCCA flag, DG flag, DSCTy, SubChId, address(2), SCCA(2)                         key = SCId
//   kDirEns09   LTO byte, ECC, international table id
//   kDirEns10   MJD(3), LSI, UTC flag, hours, minutes, seconds, milliseconds(2)
//   kDirFec14   scheme                                                                         key = SubChId
//   kDirLblEns  EId(2) charset, 16 characters, flag field(2)
//   kDirLblSvc  charset, 16 characters, flag field(2)                                          key = SId, pd
enum DirKind : int { kDirNone, kDirEns00, kDirSub01, kDirSvc02, kDirPkt03, kDirEns09, kDirEns10, kDirFec14, kDirLblEns, kDirLblSvc, kDirKinds };
constexpr int kDirPayload = 32;
DABHIP_DIR_HD inline int dir_fact_len(int kind)
{
  return kind == kDirEns00 ? 6 : kind == kDirSub01 ? 9 : kind == kDirSvc02 ? 31 : kind == kDirPkt03 ? 8 : kind == kDirEns09 ? 3 : kind == kDirEns10 ? 10 :
         kind == kDirFec14 ? 1 : kind == kDirLblEns ? 21 : kind == kDirLblSvc ? 19 : 0;
}
struct DirFact {
  uint8_t kind;                                          // DirKind
  uint8_t pd;
  uint8_t pad[2];
  uint32_t key;
  uint8_t payload[kDirPayload];
};
static_assert(sizeof(DirFact) == 40, "DirFact layout");

struct DirFibStat {
  int figs, truncated, ignored, nfacts;
};

// CRC-16-CCITT, initial value 0xFFFF, MSB first, of n bytes
DABHIP_DIR_HD inline uint16_t dir_crc16(const uint8_t* p, int n)
{
  unsigned crc = 0xffff;
  for (int i = 0; i < n; ++i) {
    crc ^= static_cast<unsigned>(p[i]) << 8;
    for (int b = 0; b < 8; ++b) crc = (crc & 0x8000) ? ((crc << 1) ^ 0x1021) & 0xffff : (crc << 1) & 0xffff;
  }
  return static_cast<uint16_t>(crc);
}
DABHIP_DIR_HD inline bool dir_fib_crc_ok(const uint8_t* fib /*32*/)
{
  const unsigned want = ~dir_crc16(fib, kDirFibData) & 0xffffu;
  return fib[30] == (want >> 8) && fib[31] == (want & 0xff);
}

// what a frame's header says: 0 = it has a Mode-I FIC at *fic_off, 1 = FICF 0, 2 = skipped (MID != 1 or NST > 64)
DABHIP_DIR_HD inline int dir_frame_class(const uint8_t* frame, int* fic_off)
{
  const int nst = frame[5] & 0x7f, ficf = frame[5] >> 7, mid = (frame[6] >> 3) & 3;
  *fic_off = 12 + 4 * nst;
  if (!ficf) return 1;
  if (mid != 1 || nst > kDirNstMax) return 2;
  return 0;
}

// ETSI table 7 as (bit rate, size in CU, protection level) per UEP index: the columns of uep_table() (dab_tables.hpp) that FIG 0/1 needs;
// dir_units.cpp holds the two together
DABHIP_DIR_HD inline void dir_uep_row(int index, int* bitrate, int* size_cu, int* protlev)
{
  static constexpr uint16_t rate[64] = {32,  32,  32,  32,  32,  48,  48,  48,  48,  48,  56,  56,  56,  56,  64,  64,  64,  64,  64,  80,  80,  80,
                                        80,  80,  96,  96,  96,  96,  96,  112, 112, 112, 112, 128, 128, 128, 128, 128, 160, 160, 160, 160, 160, 192,
                                        192, 192, 192, 192, 224, 224, 224, 224, 224, 256, 256, 256, 256, 256, 320, 320, 320, 384, 384, 384};
  static constexpr uint16_t size[64] = {16,  21,  24,  29,  35,  24,  29,  35,  42,  52,  29,  35,  42,  52,  32,  42,  48,  58,  70,  40,  52,  58,
                                        70,  84,  48,  58,  70,  84,  104, 58,  70,  84,  104, 64,  84,  96,  116, 140, 80,  104, 116, 140, 168, 96,
                                        116, 140, 168, 208, 116, 140, 168, 208, 232, 128, 168, 192, 232, 280, 160, 208, 280, 192, 280, 416};
  static constexpr uint8_t level[64] = {5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 3, 2, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 3,
                                        2, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1, 5, 4, 2, 5, 3, 1};
  *bitrate = rate[index & 63];
  *size_cu = size[index & 63];
  *protlev = level[index & 63];
}
DABHIP_DIR_HD inline int dir_eep_multiple(int protlev)
{
  static constexpr uint8_t m[8] = {12, 8, 6, 4, 27, 21, 18, 15};
  return m[protlev & 7];
}

// a fact begun: its head written, its payload zeroed
DABHIP_DIR_HD inline uint8_t* dir_fact_begin(DirFact* out, int n, int kind, int pd, uint32_t key)
{
  DirFact& f = out[n];
  f.kind = static_cast<uint8_t>(kind);
  f.pd = static_cast<uint8_t>(pd);
  f.pad[0] = f.pad[1] = 0;
  f.key = key;
  for (int k = 0; k < kDirPayload; ++k) f.payload[k] = 0;
  return f.payload;
}

// The FIG walk of one FIB whose CRC holds: reads fib[0..29] only, writes at most kDirFactSlots facts to out in byte order.
DABHIP_DIR_HD inline DirFibStat dir_walk_fib(const uint8_t* fib, DirFact* out)
{
  DirFibStat st = {0, 0, 0, 0};
  int i = 0;
  while (i < kDirFibData && fib[i] != 0xff) {
    const int type = fib[i] >> 5, len = fib[i] & 0x1f;
    ++st.figs;
    if (len == 0 || i + 1 + len > kDirFibData) { ++st.truncated; break; }
    const uint8_t* d = fib + i + 1;                      // the data field, len >= 1 bytes
    const uint8_t* b = d + 1;                            // the body
    const int bl = len - 1;
    i += 1 + len;
    if (type == 0) {
      const int cn = d[0] >> 7, oe = (d[0] >> 6) & 1, pd = (d[0] >> 5) & 1, ext = d[0] & 0x1f;
      const bool list = ext == 1 || ext == 2 || ext == 3 || ext == 14;
      if (oe || (cn && list) || !(list || ext == 0 || ext == 9 || ext == 10)) { ++st.ignored; continue; }
      if (ext == 0) {
        if (bl < 4) { ++st.truncated; continue; }
        uint8_t* p = dir_fact_begin(out, st.nfacts++, kDirEns00, 0, static_cast<uint32_t>(b[0] << 8 | b[1]));
        p[0] = b[0]; p[1] = b[1]; p[2] = b[2] >> 6; p[3] = (b[2] >> 5) & 1; p[4] = b[2] & 0x1f; p[5] = b[3];
      } else if (ext == 9) {
        if (bl < 3) { ++st.truncated; continue; }
        uint8_t* p = dir_fact_begin(out, st.nfacts++, kDirEns09, 0, 0);
        p[0] = b[0]; p[1] = b[1]; p[2] = b[2];
      } else if (ext == 10) {
        if (bl < 4 || (((b[2] >> 3) & 1) && bl < 6)) { ++st.truncated; continue; }
        const int utc = (b[2] >> 3) & 1;
        const uint32_t mjd = (static_cast<uint32_t>(b[0] & 0x7f) << 10) | (static_cast<uint32_t>(b[1]) << 2) | (b[2] >> 6);
        uint8_t* p = dir_fact_begin(out, st.nfacts++, kDirEns10, 0, 0);
        p[0] = static_cast<uint8_t>(mjd >> 16); p[1] = static_cast<uint8_t>(mjd >> 8); p[2] = static_cast<uint8_t>(mjd);
        p[3] = (b[2] >> 5) & 1;
        p[4] = static_cast<uint8_t>(utc);
        p[5] = static_cast<uint8_t>(((b[2] & 7) << 2) | (b[3] >> 6));
        p[6] = b[3] & 0x3f;
        if (utc) { p[7] = b[4] >> 2; p[8] = b[4] & 3; p[9] = b[5]; }
      } else {
        int j = 0;
        while (j < bl) {
          if (st.nfacts >= kDirFactSlots) { ++st.truncated; break; }      // (cannot happen: every fact takes a body byte of at most 28)
          if (ext == 14) {
            uint8_t* p = dir_fact_begin(out, st.nfacts++, kDirFec14, 0, static_cast<uint32_t>(b[j] >> 2));
            p[0] = b[j] & 3;
            j += 1;
          } else if (ext == 1) {
            if (j + 3 > bl) { ++st.truncated; break; }
            const int form = b[j + 2] >> 7, size = form ? 4 : 3;
            if (j + size > bl) { ++st.truncated; break; }
            const int start = ((b[j] & 3) << 8) | b[j + 1];
            int index = 0, protlev, size_cu, bitrate;
            if (!form) {
              index = b[j + 2] & 0x3f;
              dir_uep_row(index, &bitrate, &size_cu, &protlev);
            } else {
              protlev = ((b[j + 2] >> 2) & 3) | (((b[j + 2] >> 4) & 7) << 2);
              size_cu = ((b[j + 2] & 3) << 8) | b[j + 3];
              bitrate = (size_cu / dir_eep_multiple(protlev)) * ((protlev & 4) ? 32 : 8);
            }
            uint8_t* p = dir_fact_begin(out, st.nfacts++, kDirSub01, 0, static_cast<uint32_t>(b[j] >> 2));
            p[0] = static_cast<uint8_t>(form); p[1] = static_cast<uint8_t>(index); p[2] = static_cast<uint8_t>(protlev);
            p[3] = static_cast<uint8_t>(start >> 8); p[4] = static_cast<uint8_t>(start);
            p[5] = static_cast<uint8_t>(size_cu >> 8); p[6] = static_cast<uint8_t>(size_cu);
            p[7] = static_cast<uint8_t>(bitrate >> 8); p[8] = static_cast<uint8_t>(bitrate);
            j += size;
          } else if (ext == 2) {
            const int sl = pd ? 4 : 2;
            if (j + sl + 1 > bl) { ++st.truncated; break; }
            const int nc = b[j + sl] & 0x0f, size = sl + 1 + 2 * nc;
            if (j + size > bl) { ++st.truncated; break; }
            uint32_t sid = 0;
            for (int k = 0; k < sl; ++k) sid = (sid << 8) | b[j + k];
            uint8_t* p = dir_fact_begin(out, st.nfacts++, kDirSvc02, pd, sid);
            for (int k = 0; k < 1 + 2 * nc; ++k) p[k] = b[j + sl + k];
            j += size;
          } else {                                       // 0/3
            if (j + 2 > bl) { ++st.truncated; break; }
            const int flag = b[j + 1] & 1, size = flag ? 7 : 5;
            if (j + size > bl) { ++st.truncated; break; }
            uint8_t* p = dir_fact_begin(out, st.nfacts++, kDirPkt03, 0, static_cast<uint32_t>((b[j] << 4) | (b[j + 1] >> 4)));
            p[0] = static_cast<uint8_t>(flag); p[1] = b[j + 2] >> 7; p[2] = b[j + 2] & 0x3f; p[3] = b[j + 3] >> 2;
            p[4] = b[j + 3] & 3; p[5] = b[j + 4];
            if (flag) { p[6] = b[j + 5]; p[7] = b[j + 6]; }
            j += size;
          }
        }
      }
    } else if (type == 1) {
      const int charset = d[0] >> 4, oe = (d[0] >> 3) & 1, ext = d[0] & 7;
      if (oe || !(ext == 0 || ext == 1 || ext == 5)) { ++st.ignored; continue; }
      const int kl = ext == 5 ? 4 : 2;
      if (len != 1 + kl + 18) { ++st.truncated; continue; }
      uint32_t key = 0;
      for (int k = 0; k < kl; ++k) key = (key << 8) | b[k];
      uint8_t* p = dir_fact_begin(out, st.nfacts++, ext == 0 ? kDirLblEns : kDirLblSvc, ext == 5, key);
      if (ext == 0) { p[0] = b[0]; p[1] = b[1]; p += 2; }
      p[0] = static_cast<uint8_t>(charset);
      for (int k = 0; k < 18; ++k) p[1 + k] = b[kl + k];
    } else {
      ++st.ignored;
    }
  }
  return st;
}

// ---- the kept facts as the public records -------------------------------------------------------------------------------------------------
// An entry of a table keeps, per part, the payload of the latest fact of that kind (DirEntry, dir.hpp); these turn the parts into dabhip.h's
// records.  `have` bits are in part order.

DABHIP_DIR_HD inline void dir_subch_from(const uint8_t* p01, const uint8_t* p14, int have, int id, dabhip_dir_subch* o)
{
  o->have = static_cast<uint8_t>(have);
  o->id = static_cast<uint8_t>(id);
  o->form = p01[0]; o->uep_index = p01[1]; o->protlev = p01[2];
  o->start_cu = static_cast<uint16_t>(p01[3] << 8 | p01[4]);
  o->size_cu = static_cast<uint16_t>(p01[5] << 8 | p01[6]);
  o->bitrate = static_cast<uint16_t>(p01[7] << 8 | p01[8]);
  o->fec_scheme = p14[0];
}
DABHIP_DIR_HD inline void dir_service_from(const uint8_t* p02, const uint8_t* lbl, int have, int pd, uint32_t sid, dabhip_dir_service* o)
{
  o->sid = sid;
  o->pd = static_cast<uint8_t>(pd);
  o->have = static_cast<uint8_t>(have);
  o->info = p02[0];
  o->ncomp = p02[0] & 0x0f;
  for (int k = 0; k < 30; ++k) o->comp[k] = p02[1 + k];
  o->charset = lbl[0];
  for (int k = 0; k < 16; ++k) o->label[k] = lbl[1 + k];
  o->char_flags = static_cast<uint16_t>(lbl[17] << 8 | lbl[18]);
}
DABHIP_DIR_HD inline void dir_pktcomp_from(const uint8_t* p, uint32_t scid, dabhip_dir_pktcomp* o)
{
  o->scid = static_cast<uint16_t>(scid);
  o->scca_flag = p[0]; o->dg = p[1]; o->dscty = p[2]; o->subch = p[3];
  o->address = static_cast<uint16_t>(p[4] << 8 | p[5]);
  o->scca = static_cast<uint16_t>(p[6] << 8 | p[7]);
}
DABHIP_DIR_HD inline void dir_ensemble_from(const uint8_t* p00, const uint8_t* p09, const uint8_t* p10, const uint8_t* lbl, int have, dabhip_dir_ensemble_rec* o)
{
  o->have = static_cast<uint8_t>(have);
  o->eid = static_cast<uint16_t>(p00[0] << 8 | p00[1]);
  o->change_flag = p00[2]; o->al = p00[3]; o->cif_hi = p00[4]; o->cif_lo = p00[5];
  o->lto = p09[0]; o->ecc = p09[1]; o->inter_table = p09[2];
  o->mjd = static_cast<uint32_t>(p10[0]) << 16 | static_cast<uint32_t>(p10[1]) << 8 | p10[2];
  o->lsi = p10[3]; o->utc_flag = p10[4]; o->hours = p10[5]; o->minutes = p10[6]; o->seconds = p10[7];
  o->milliseconds = static_cast<uint16_t>(p10[8] << 8 | p10[9]);
  o->label_eid = static_cast<uint16_t>(lbl[0] << 8 | lbl[1]);
  o->charset = lbl[2];
  for (int k = 0; k < 16; ++k) o->label[k] = lbl[3 + k];
  o->char_flags = static_cast<uint16_t>(lbl[19] << 8 | lbl[20]);
}

// ---- complete and resolve over the public records -----------------------------------------------------------------------------------------
struct DirView {
  const dabhip_dir_ensemble_rec* ens;
  const dabhip_dir_subch* sub;                           // nsub entries in SubChId order
  int nsub;
  const dabhip_dir_service* svc;
  int nsvc;
  const dabhip_dir_pktcomp* pkt;
  int npkt;
};
inline bool dir_has_subch(const DirView& v, int id)
{
  for (int i = 0; i < v.nsub; ++i)
    if (v.sub[i].id == id) return (v.sub[i].have & DABHIP_DIR_SUB_HAVE_01) != 0;
  return false;
}
inline const dabhip_dir_pktcomp* dir_find_pkt(const DirView& v, int scid)
{
  for (int i = 0; i < v.npkt; ++i)
    if (v.pkt[i].scid == scid) return &v.pkt[i];
  return nullptr;
}
// 0 and *t, or DABHIP_DIR_NO_*
inline int dir_resolve_component(const DirView& v, const dabhip_dir_service& s, int component, dabhip_dir_target* t)
{
  if (!(s.have & DABHIP_DIR_SVC_HAVE_02) || component < 0 || component >= s.ncomp) return DABHIP_DIR_NO_COMPONENT;
  const int c0 = s.comp[2 * component], c1 = s.comp[2 * component + 1];
  const int tmid = c0 >> 6;
  *t = dabhip_dir_target{DABHIP_DIR_UNKNOWN, -1, 0, 0, 0, 0, -1, (c1 >> 1) & 1};
  if (tmid == 2) return 0;
  if (tmid == 3) {
    const int scid = ((c0 & 0x3f) << 6) | (c1 >> 2);
    const dabhip_dir_pktcomp* p = dir_find_pkt(v, scid);
    if (!p) return DABHIP_DIR_NO_PKTCOMP;
    if (!dir_has_subch(v, p->subch)) return DABHIP_DIR_NO_SUBCH;
    t->kind = DABHIP_DIR_PACKET;
    t->subch = p->subch;
    t->address = p->address;
    t->dg = p->dg;
    t->dscty = p->dscty;
    t->scid = scid;
    for (int i = 0; i < v.nsub; ++i)
      if (v.sub[i].id == p->subch) t->fec = (v.sub[i].have & DABHIP_DIR_SUB_HAVE_14) && v.sub[i].fec_scheme == 1;
    return 0;
  }
  const int ty = c0 & 0x3f, id = c1 >> 2;
  if (!dir_has_subch(v, id)) return DABHIP_DIR_NO_SUBCH;
  t->subch = id;
  if (tmid == 0) t->kind = ty == 0 ? DABHIP_DIR_MP2 : ty == 63 ? DABHIP_DIR_DABPLUS : DABHIP_DIR_UNKNOWN;
  else t->kind = ty == 24 ? DABHIP_DIR_TS : DABHIP_DIR_STREAM_DATA;
  return 0;
}
inline int dir_resolve(const DirView& v, int pd, uint32_t sid, int component, dabhip_dir_target* t)
{
  for (int i = 0; i < v.nsvc; ++i)
    if (v.svc[i].pd == pd && v.svc[i].sid == sid) return dir_resolve_component(v, v.svc[i], component, t);
  return DABHIP_DIR_NO_SERVICE;
}
inline bool dir_complete(const DirView& v)
{
  if ((v.ens->have & (DABHIP_DIR_HAVE_00 | DABHIP_DIR_HAVE_LABEL)) != (DABHIP_DIR_HAVE_00 | DABHIP_DIR_HAVE_LABEL) || v.nsvc < 1) return false;
  for (int i = 0; i < v.nsvc; ++i) {
    const dabhip_dir_service& s = v.svc[i];
    if (s.have != (DABHIP_DIR_SVC_HAVE_02 | DABHIP_DIR_SVC_HAVE_LABEL)) return false;
    for (int c = 0; c < s.ncomp; ++c) {
      dabhip_dir_target t;
      if (dir_resolve_component(v, s, c, &t) != 0) return false;
    }
  }
  return true;
}

}  // namespace dabhip
