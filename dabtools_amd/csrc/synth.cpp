// synth.cpp — synthetic DAB Mode-I modulator (host only): ensemble configuration ->
// 2.048 Msps cu8 IQ.  The reference contains no transmitter; this is the workload
// generator for tests and bench.py, built as the exact inverse of the receive chain the
// reference implements (fic.c:47-130 FIG parsing, depuncture.c, misc.c:29-58,
// input_sdr.c:132-162 demap, sdr_prstab.c PRS, dab_tables.c tables).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dabhip.h"
#include "dab_bits.hpp"
#include "dab_tables.hpp"
#include "dabplus.hpp"
#include "packet_sync.hpp"
#include "rs_code.hpp"
#include "ts_sync.hpp"
#include "synth.hpp"
#include "tii_detect.hpp"

namespace dabhip {
void set_error(const std::string& msg);

namespace {

// counter-based generator: value = f(seed, stream of keys); reproducible on any machine
inline uint64_t mix64(uint64_t z)
{
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
inline uint64_t key(uint64_t seed, uint64_t a, uint64_t b, uint64_t c) { return mix64(mix64(mix64(seed ^ mix64(a)) + b) + c); }

enum : uint64_t { kDomPayload = 1, kDomFiller = 2, kDomNoise = 3, kDomDabPlus = 4, kDomPacket = 5, kDomTs = 6 };

SubChannel to_subchannel(const dabhip_subch_cfg& c)
{
  SubChannel sc;
  sc.id = c.id;
  sc.start_cu = c.start_cu;
  sc.slform = c.slform;
  if (!c.slform) {
    const UepProfile& u = uep_table()[c.uep_index & 63];
    sc.uep_index = c.uep_index & 63;
    sc.size_cu = u.size_cu;
    sc.bitrate = u.bitrate;
    sc.protlev = u.protlevel;
  } else {
    sc.protlev = c.eep_protlev & 7;
    sc.size_cu = c.size_cu;
    sc.bitrate = (c.size_cu / eep_size_multiple(sc.protlev)) * ((sc.protlev & 4) ? 32 : 8);
  }
  return sc;
}

// the multiplex in force at logical CIF `cif`: in the MSC (lead = 0) or as announced by the FIC (lead = the entry's fic_lead)
struct Multiplex {
  int nsub;
  const dabhip_subch_cfg* sub;
};
Multiplex multiplex_at(const dabhip_synth_cfg& cfg, int cif, bool fic)
{
  Multiplex m{cfg.nsub, cfg.sub};
  for (const dabhip_reconf_cfg& r : cfg.reconf)
    if (r.at_cif > 0 && cif >= r.at_cif - (fic ? r.fic_lead : 0)) m = Multiplex{r.nsub, r.sub};
  return m;
}

bool validate_multiplex(int nsub, const dabhip_subch_cfg* sub)
{
  if (nsub < 0 || nsub > 64) { set_error("synth: nsub out of range"); return false; }
  std::vector<char> used(864, 0);
  for (int k = 0; k < nsub; ++k) {
    const SubChannel sc = to_subchannel(sub[k]);
    if (sc.id < 0 || sc.id > 63 || sc.bitrate <= 0 || sc.start_cu < 0 || sc.start_cu + sc.size_cu > 864) {
      set_error("synth: sub-channel " + std::to_string(k) + " does not fit the CIF");
      return false;
    }
    if (puncture_plan(sc).coded_bits() > sc.size_cu * 64) { set_error("synth: sub-channel over-long"); return false; }
    for (int cu = sc.start_cu; cu < sc.start_cu + sc.size_cu; ++cu) {
      if (used[cu]) { set_error("synth: overlapping sub-channels"); return false; }
      used[cu] = 1;
    }
  }
  return true;
}

bool channel_active(const dabhip_channel_cfg& c)
{
  return c.sro_ppm != 0.0 || c.echo_delay[0] || c.echo_delay[1] || c.fade_depth != 0.0 || c.iq_gain_db != 0.0 || c.iq_phase_deg != 0.0;
}

bool si_fits(const dabhip_synth_cfg& cfg);

bool validate(const dabhip_synth_cfg& cfg)
{
  if (!validate_multiplex(cfg.nsub, cfg.sub)) return false;
  if (cfg.dabplus_slots) {
    if (cfg.nsub < 64 && (cfg.dabplus_slots >> cfg.nsub)) { set_error("synth: dabplus_slots names a slot past nsub"); return false; }
    for (const dabhip_reconf_cfg& r : cfg.reconf)
      if (r.at_cif != 0) { set_error("synth: dabplus_slots cannot be combined with reconfigurations"); return false; }
    for (int k = 0; k < cfg.nsub; ++k)
      if ((cfg.dabplus_slots >> k & 1) && to_subchannel(cfg.sub[k]).bitrate % 8) { set_error("synth: a DAB+ slot needs a multiple of 8 kbit/s"); return false; }
  }
  if (cfg.packet_fec_slots & ~cfg.packet_slots) { set_error("synth: packet_fec_slots names a slot that packet_slots does not"); return false; }
  if (cfg.packet_slots) {
    if (cfg.nsub < 64 && (cfg.packet_slots >> cfg.nsub)) { set_error("synth: packet_slots names a slot past nsub"); return false; }
    if (cfg.packet_slots & cfg.dabplus_slots) { set_error("synth: a slot cannot be both a packet-mode and a DAB+ slot"); return false; }
    for (const dabhip_reconf_cfg& r : cfg.reconf)
      if (r.at_cif != 0) { set_error("synth: packet_slots cannot be combined with reconfigurations"); return false; }
    for (int k = 0; k < cfg.nsub; ++k)
      if ((cfg.packet_slots >> k & 1) && to_subchannel(cfg.sub[k]).bitrate % 8) { set_error("synth: a packet-mode slot needs a multiple of 8 kbit/s"); return false; }
  }
  if (cfg.ts_slots) {
    if (cfg.nsub < 64 && (cfg.ts_slots >> cfg.nsub)) { set_error("synth: ts_slots names a slot past nsub"); return false; }
    if (cfg.ts_slots & cfg.dabplus_slots) { set_error("synth: a slot cannot be both an MPEG-2 TS and a DAB+ slot"); return false; }
    if (cfg.ts_slots & cfg.packet_slots) { set_error("synth: a slot cannot be both an MPEG-2 TS and a packet-mode slot"); return false; }
    for (const dabhip_reconf_cfg& r : cfg.reconf)
      if (r.at_cif != 0) { set_error("synth: ts_slots cannot be combined with reconfigurations"); return false; }
  }
  if (cfg.si_mode) {
    if (cfg.si_mode != 1) { set_error("synth: si_mode must be 0 or 1"); return false; }
    for (const dabhip_reconf_cfg& r : cfg.reconf)
      if (r.at_cif != 0) { set_error("synth: si_mode cannot be combined with reconfigurations"); return false; }
    if (cfg.fib_patch_len > 0) { set_error("synth: si_mode cannot be combined with a FIB patch"); return false; }
    if (!si_fits(cfg)) { set_error("synth: si_mode: the FIBs have no room for a FIG of the service information"); return false; }
  }
  int prev = 0;
  for (const dabhip_reconf_cfg& r : cfg.reconf) {
    if (r.at_cif == 0) continue;
    if (r.at_cif <= prev || r.fic_lead < 0) { set_error("synth: reconfigurations must be at ascending CIFs > 0 with fic_lead >= 0"); return false; }
    prev = r.at_cif;
    if (!validate_multiplex(r.nsub, r.sub)) return false;
  }
  if (cfg.skip_samples < 0 || cfg.skip_samples >= kTfSamples) { set_error("synth: skip_samples out of range"); return false; }
  const dabhip_channel_cfg& c = cfg.channel;
  for (int e = 0; e < 2; ++e)
    if (c.echo_delay[e] < 0 || c.echo_delay[e] > 2047) { set_error("synth: echo delay out of range (0 .. 2047 samples)"); return false; }
  if (c.fade_depth < 0.0 || c.fade_depth >= 1.0 || std::fabs(c.sro_ppm) > 1000.0) { set_error("synth: channel parameters out of range"); return false; }
  for (const dabhip_tii_cfg& t : cfg.tii)
    if (t.enabled && (t.main_id < 0 || t.main_id >= kTiiPatterns || t.sub_id < 0 || t.sub_id >= kTiiSubs || !std::isfinite(t.level_db))) {
      set_error("synth: a TII comb needs main_id 0 .. 69, sub_id 0 .. 23 and a finite level");
      return false;
    }
  return true;
}

// ---- the outer codes' field and encoder (rs_code.hpp has the codes) -----------------------------------------------------------------------------
const GfTables& gf()
{
  struct Init {
    GfTables t;
    Init() { gf_build(t); }
  };
  static const Init g;
  return g.t;
}

inline uint8_t gf_mul(uint8_t a, uint8_t b)
{
  return (a && b) ? gf().exp[gf().log[a] + gf().log[b]] : 0;
}

// coefficients of prod_{i=0..kRoots-1} (x + alpha^i), highest degree first (gen[0] = 1)
template <int kRoots>
const uint8_t* rs_generator()
{
  struct Init {
    uint8_t g[kRoots + 1] = {1};
    Init()
    {
      for (int i = 0; i < kRoots; ++i) {
        const uint8_t r = gf().exp[i];
        for (int k = i + 1; k >= 1; --k) g[k] ^= gf_mul(g[k - 1], r);
      }
    }
  };
  static const Init g;
  return g.g;
}

// the kRoots parity bytes of the systematic code word whose ndata data bytes are data[0], data[dstride], ...: parity[0], parity[pstride], ...
template <int kRoots>
void rs_parity(int ndata, const uint8_t* data, size_t dstride, uint8_t* parity, size_t pstride)
{
  const uint8_t* g = rs_generator<kRoots>();
  uint8_t rem[kRoots] = {0};
  for (int k = 0; k < ndata; ++k) {
    const uint8_t fb = data[k * dstride] ^ rem[0];
    for (int q = 0; q < kRoots - 1; ++q) rem[q] = rem[q + 1] ^ gf_mul(fb, g[q + 1]);
    rem[kRoots - 1] = gf_mul(fb, g[kRoots]);
  }
  for (int q = 0; q < kRoots; ++q) parity[q * pstride] = rem[q];
}

// ---- DAB+ superframes (ETSI TS 102 563) --------------------------------------------------------------------------------------------------------
// the 110 s unprotected bytes of superframe n of a DAB+ slot of 8 s kbit/s
void dabplus_superframe(const dabhip_synth_cfg& cfg, int n, int slot, int s, uint8_t* out)
{
  const int total = kRsK * s;
  const uint64_t pk = key(cfg.seed, kDomDabPlus, static_cast<uint64_t>(slot), ~0ull);   // the slot's audio parameters
  static const int pairs[4][2] = {{0, 1}, {0, 0}, {1, 1}, {1, 0}};                      // (dac_rate, sbr_flag): 2, 4, 3, 6 AUs
  const uint64_t rot = key(cfg.seed, kDomDabPlus, 64, ~0ull) + static_cast<uint64_t>(slot);               // consecutive slots: all four pairs
  const int dac = pairs[rot & 3][0], sbr = pairs[rot & 3][1];
  const int ch = static_cast<int>(pk >> 8 & 1), ps = static_cast<int>(pk >> 9 & 1);
  int nau = 0, start0 = 0;
  au_layout(dac, sbr, &nau, &start0);
  const uint64_t sfk = (static_cast<uint64_t>(static_cast<uint32_t>(n)) << 8) | static_cast<uint64_t>(slot);
  // AU lengths (each >= 3: one byte and the CRC): weights from the key; au_start is 12 bits, so all AUs but the last start below 4096
  int64_t w[kMaxAus], wsum = 0, len[kMaxAus];
  for (int i = 0; i < nau; ++i) { w[i] = 1 + static_cast<int64_t>(key(cfg.seed, kDomDabPlus, sfk, 1000 + i) & 255); wsum += w[i]; }
  const int64_t extra = total - start0 - 3 * nau;
  int64_t used = 0;
  for (int i = 0; i < nau - 1; ++i) { len[i] = 3 + extra * w[i] / wsum; used += len[i]; }
  const int64_t room = 4095 - start0 - 3 * (nau - 1);          // the last AU's start, start0 + used, must stay <= 4095
  if (used - 3 * (nau - 1) > room) {
    const int64_t ex = used - 3 * (nau - 1);
    used = 0;
    for (int i = 0; i < nau - 1; ++i) { len[i] = 3 + (len[i] - 3) * room / ex; used += len[i]; }
  }
  len[nau - 1] = total - start0 - used;
  std::memset(out, 0, static_cast<size_t>(total));
  out[2] = static_cast<uint8_t>((dac << 6) | (sbr << 5) | (ch << 4) | (ps << 3));   // rfa 0, mpeg_surround_config 0
  int pos = start0;
  uint64_t bits = 0;
  for (int i = 0; i < nau; ++i) {
    if (i) bits = (bits << 12) | static_cast<uint64_t>(pos);
    const int body = static_cast<int>(len[i]) - 2;
    for (int b = 0; b < body; b += 8) {
      const uint64_t v = key(cfg.seed, kDomDabPlus, sfk, static_cast<uint64_t>(pos + b));
      for (int q = 0; q < 8 && b + q < body; ++q) out[pos + b + q] = static_cast<uint8_t>(v >> (8 * q));
    }
    const uint16_t crc = static_cast<uint16_t>(~crc16_ccitt(out + pos, static_cast<size_t>(body)));
    out[pos + body] = static_cast<uint8_t>(crc >> 8);
    out[pos + body + 1] = static_cast<uint8_t>(crc & 0xff);
    pos += static_cast<int>(len[i]);
  }
  const int nbits = 12 * (nau - 1), nbytes = (nbits + 7) / 8;
  bits <<= 8 * nbytes - nbits;
  for (int b = 0; b < nbytes; ++b) out[3 + b] = static_cast<uint8_t>(bits >> (8 * (nbytes - 1 - b)));
  const uint16_t fc = fire_code(out + 2);
  out[0] = static_cast<uint8_t>(fc >> 8);
  out[1] = static_cast<uint8_t>(fc & 0xff);
}

// bytes [24 s part, 24 s (part + 1)) of the protected superframe n: data, then the parity of the s interleaved codewords (codeword j = bytes j + k s)
void dabplus_protected_part(const dabhip_synth_cfg& cfg, int n, int part, int slot, int s, uint8_t* out)
{
  std::vector<uint8_t> sf(static_cast<size_t>(kRsN) * s);
  dabplus_superframe(cfg, n, slot, s, sf.data());
  uint8_t* parity = sf.data() + static_cast<size_t>(kRsK) * s;
  for (int j = 0; j < s; ++j) rs_parity<kRsRoots>(kRsK, sf.data() + j, s, parity + j, s);
  std::memcpy(out, sf.data() + static_cast<size_t>(24) * s * part, static_cast<size_t>(24) * s);
}

int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// ---- packet mode (ETSI EN 300 401 clauses 5.3.2, 5.3.3, 5.3.5; dabhip.h: dabhip_packet has the formats) ----------------------------------------
// the addresses a packet slot's groups go out on: two or three, from the slot's key
int packet_addresses(const dabhip_synth_cfg& cfg, int slot, int* out3)
{
  const uint64_t pk = key(cfg.seed, kDomPacket, static_cast<uint64_t>(slot), ~0ull);
  const int base = 1 + static_cast<int>((pk >> 8) % 300);
  for (int i = 0; i < 3; ++i) out3[i] = base + 301 * i;
  return 2 + static_cast<int>(pk & 1);
}

using PacketGroupList = std::vector<std::pair<int, std::vector<uint8_t>>>;

// Unit j of a packet slot -- the application table of FEC frame j, or without FEC the cells of logical CIF j: ncells cells filled exactly with the
// packets of data groups with random lengths and flags on the slot's addresses, which start and end inside the unit, with command and padding
// packets in between.  `groups`: every group in the order their last packets go out.
void packet_unit(const dabhip_synth_cfg& cfg, int slot, int j, int ncells, uint8_t* out, PacketGroupList* groups)
{
  uint64_t ctr = 0;
  const uint64_t uk = (static_cast<uint64_t>(static_cast<uint32_t>(j)) << 8) | static_cast<uint64_t>(slot);
  const auto below = [&](int m) { return static_cast<int>(key(cfg.seed, kDomPacket, uk, ctr++) % static_cast<uint64_t>(m)); };
  int addr[3];
  const int naddr = packet_addresses(cfg, slot, addr);
  std::vector<uint8_t> open[3];
  bool is_open[3] = {false, false, false}, crc_flag[3] = {false, false, false};
  int ci[3], nopen = 0, room = ncells;
  for (int a = 0; a < 3; ++a) ci[a] = below(4);
  uint8_t* p = out;
  // one packet of L cells; for a data packet of address index a, `useful` is what the group gets
  const auto packet = [&](int L, int cont, int fl, int address, int cmd, const uint8_t* useful, int ulen) {
    const int n = kPkCell * L;
    std::memset(p, 0, static_cast<size_t>(n));
    p[0] = static_cast<uint8_t>(((L - 1) << 6) | (cont << 4) | (fl << 2) | (address >> 8));
    p[1] = static_cast<uint8_t>(address & 0xff);
    p[2] = static_cast<uint8_t>((cmd << 7) | ulen);
    if (ulen) std::memcpy(p + 3, useful, static_cast<size_t>(ulen));
    const uint16_t crc = static_cast<uint16_t>(~crc16_ccitt(p, static_cast<size_t>(n - 2)));
    p[n - 2] = static_cast<uint8_t>(crc >> 8);
    p[n - 1] = static_cast<uint8_t>(crc & 0xff);
    p += n;
    room -= L;
  };
  // a data packet of address index a: opens a group (its header first), goes on with it or, with last, ends it (the group CRC last)
  const auto data_packet = [&](int a, int L, bool last) {
    const bool first = !is_open[a];
    std::vector<uint8_t>& g = open[a];
    const int cap = kPkCell * L - 5;
    uint8_t useful[kPkCell * 4];
    int n = 0;
    if (first) {
      g.clear();
      const int flags = below(16), ua = flags & 1;
      crc_flag[a] = flags >> 2 & 1;
      useful[n++] = static_cast<uint8_t>((flags << 4) | below(16));
      useful[n++] = static_cast<uint8_t>(below(256));
      for (int i = 0; i < ((flags >> 3 & 1) ? 2 : 0) + ((flags >> 1 & 1) ? 2 : 0); ++i) useful[n++] = static_cast<uint8_t>(below(256));
      if (ua) {
        const int tflag = below(2), li = 2 * tflag + below(4);
        useful[n++] = static_cast<uint8_t>((below(8) << 5) | (tflag << 4) | li);
        for (int i = 0; i < li; ++i) useful[n++] = static_cast<uint8_t>(below(256));
      }
    }
    const int tail = last && crc_flag[a] ? 2 : 0;
    const int least = std::max(n + tail, 1);
    const int ulen = below(4) ? cap : least + below(cap - least + 1);
    while (n < ulen - tail) useful[n++] = static_cast<uint8_t>(below(256));
    g.insert(g.end(), useful, useful + n);
    if (tail) {
      const uint16_t crc = static_cast<uint16_t>(~crc16_ccitt(g.data(), g.size()));
      useful[n++] = static_cast<uint8_t>(crc >> 8);
      useful[n++] = static_cast<uint8_t>(crc & 0xff);
      g.insert(g.end(), useful + n - 2, useful + n);
    }
    ci[a] = (ci[a] + 1) & 3;
    packet(L, ci[a], (first ? 2 : 0) | (last ? 1 : 0), addr[a], 0, useful, n);
    if (first && !last) ++nopen;
    if (!first && last) --nopen;
    is_open[a] = !last;
    if (last && groups) groups->emplace_back(addr[a], g);
  };
  while (room > 0) {
    const int slack = room - nopen;                   // the cells free beyond one closing cell for every open group
    if (slack == 0) {
      int a = 0;
      while (!is_open[a]) ++a;
      data_packet(a, 1, true);
      continue;
    }
    const int kind = below(10);
    if (kind <= 1) {
      const int L = 1 + below(std::min(4, slack));
      if (kind == 0) {
        packet(L, 0, 3, 0, 0, nullptr, 0);
      } else {
        uint8_t useful[kPkCell * 4];
        const int ulen = below(kPkCell * L - 4);
        for (int i = 0; i < ulen; ++i) useful[i] = static_cast<uint8_t>(below(256));
        packet(L, below(4), 3, addr[below(naddr)], 1, useful, ulen);
      }
      continue;
    }
    const int a = below(naddr);
    if (is_open[a]) {
      const bool last = below(3) == 0;
      data_packet(a, 1 + below(std::min(4, slack + (last ? 1 : 0))), last);
    } else {
      const bool only = slack < 2 || below(4) == 0;
      data_packet(a, 1 + below(std::min(4, only ? slack : slack - 1)), only);
    }
  }
}

// the cells of unit j of a packet slot as sent: without FEC the ncells cells; with it the 94 table cells and the 9 FEC cells
void packet_unit_cells(const dabhip_synth_cfg& cfg, int slot, int j, int ncells, bool fec, std::vector<uint8_t>& out)
{
  struct Cache {
    uint64_t seed = 0;
    int slot = -1, j = 0, ncells = 0;
    bool fec = false;
    std::vector<uint8_t> cells;
  };
  thread_local Cache cache;
  if (cache.slot == slot && cache.seed == cfg.seed && cache.j == j && cache.ncells == ncells && cache.fec == fec) {
    out = cache.cells;
    return;
  }
  out.assign(static_cast<size_t>(fec ? kPkFrameCells : ncells) * kPkCell, 0);
  packet_unit(cfg, slot, j, ncells, out.data(), nullptr);
  if (fec) {
    uint8_t parity[kPkRoots * kPkRows + 6] = {0};
    for (int r = 0; r < kPkRows; ++r) rs_parity<kPkRoots>(kPkK, out.data() + r, kPkRows, parity + r, kPkRows);
    for (int i = 0; i < kPkFecCells; ++i) {
      uint8_t* cell = out.data() + (kPkDataCells + i) * kPkCell;
      cell[0] = static_cast<uint8_t>((i << 2) | (kPkFecAddress >> 8));
      cell[1] = static_cast<uint8_t>(kPkFecAddress & 0xff);
      std::memcpy(cell + 2, parity + kPkFecPayload * i, kPkFecPayload);
    }
  }
  cache.seed = cfg.seed;
  cache.slot = slot;
  cache.j = j;
  cache.ncells = ncells;
  cache.fec = fec;
  cache.cells = out;
}

int64_t floor_div64(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// n cells of a packet slot of s cells per CIF from cell c on, cells counted from logical CIF 0's first
void packet_cells(const dabhip_synth_cfg& cfg, int slot, int s, int64_t c, int n, uint8_t* out)
{
  const bool fec = cfg.packet_fec_slots >> slot & 1;
  std::vector<uint8_t> unit;
  for (int i = 0; i < n; ++i, ++c) {
    const int64_t per = fec ? kPkFrameCells : s, rel = fec ? c - cfg.packet_phase : c;
    const int64_t j = floor_div64(rel, per);
    packet_unit_cells(cfg, slot, static_cast<int>(j), fec ? kPkDataCells : s, fec, unit);
    std::memcpy(out + static_cast<size_t>(i) * kPkCell, unit.data() + (rel - j * per) * kPkCell, kPkCell);
  }
}

// ---- MPEG-2 TS (ETSI TS 102 427; dabhip.h: dabhip_ts has the formats) --------------------------------------------------------------------------
// Code word n of a TS slot.  Words go in blocks of 8 with a fixed mix of the slot's two or three PIDs and null packets, shuffled by the block's
// key: so the continuity counter of a PID is a closed form of n (n may be negative) and needs no history.
void ts_word(const dabhip_synth_cfg& cfg, int slot, int64_t n, uint8_t* out)
{
  const uint64_t sk = key(cfg.seed, kDomTs, 64 + static_cast<uint64_t>(slot), 0);
  const bool three = sk & 1;
  const int base = 0x20 + static_cast<int>((sk >> 8) & 0xfff);
  static const int8_t mix2[8] = {0, 0, 0, 1, 1, 1, -1, -1}, mix3[8] = {0, 0, 0, 1, 1, 2, 2, -1};
  int8_t order[8];
  std::memcpy(order, three ? mix3 : mix2, 8);
  const int64_t blk = floor_div64(n, 8);
  const int idx = static_cast<int>(n - 8 * blk);
  for (int i = 7; i >= 1; --i) {
    const int j = static_cast<int>(key(cfg.seed, kDomTs, 128 + static_cast<uint64_t>(slot), static_cast<uint64_t>(blk) * 8 + static_cast<uint64_t>(i)) % static_cast<uint64_t>(i + 1));
    std::swap(order[i], order[j]);
  }
  const int who = order[idx];
  const uint64_t wk = key(cfg.seed, kDomTs, static_cast<uint64_t>(slot), static_cast<uint64_t>(n));
  int pid = kTsNullPid, cc = 0, pusi = 0;
  if (who >= 0) {
    int per = 0, before = 0;
    for (int i = 0; i < 8; ++i) {
      per += order[i] == who;
      before += i < idx && order[i] == who;
    }
    pid = base + 0x101 * who;
    cc = static_cast<int>((((blk % 16) * per + before) % 16 + 16) % 16);
    pusi = (wk & 7) == 0;
  }
  out[0] = kTsSyncByte;
  out[1] = static_cast<uint8_t>((pusi << 6) | (pid >> 8));
  out[2] = static_cast<uint8_t>(pid & 0xff);
  out[3] = static_cast<uint8_t>(0x10 | cc);                                // payload only
  for (int i = 4; i < kTsData; i += 8) {
    const uint64_t v = key(cfg.seed, kDomTs, wk, static_cast<uint64_t>(i));
    for (int b = 0; b < 8 && i + b < kTsData; ++b) out[i + b] = static_cast<uint8_t>(v >> (8 * b));
  }
  rs_parity<kPkRoots>(kTsData, out, 1, out + kTsData, 1);
}

// n bytes of a TS slot from stream position x on (bytes counted from logical CIF 0's first): the byte at x is byte k = (x - ts_phase) mod 204 of
// the word whose slot started 204 (k mod 12) bytes before x - k
void ts_bytes(const dabhip_synth_cfg& cfg, int slot, int64_t x, int n, uint8_t* out)
{
  struct Entry {
    uint64_t seed = 0;
    int slot = -1;
    int64_t n = 0;
    uint8_t word[kTsSlot];
  };
  thread_local Entry cache[64];
  for (int i = 0; i < n; ++i, ++x) {
    const int64_t rel = x - cfg.ts_phase;
    const int k = static_cast<int>(rel - kTsSlot * floor_div64(rel, kTsSlot));
    const int64_t w = (rel - k) / kTsSlot - k % kTsBranches;
    Entry& e = cache[static_cast<uint64_t>(w) & 63];
    if (e.slot != slot || e.seed != cfg.seed || e.n != w) {
      ts_word(cfg, slot, w, e.word);
      e.seed = cfg.seed;
      e.slot = slot;
      e.n = w;
    }
    out[i] = e.word[k];
  }
}

void payload_bytes(const dabhip_synth_cfg& cfg, int cif, int slot, uint8_t* out, int n)
{
  if (cfg.dabplus_slots >> slot & 1) {                     // n = 24 s
    const int rel = cif - cfg.dabplus_phase, sf = floor_div(rel, kSfFrames);
    dabplus_protected_part(cfg, sf, rel - kSfFrames * sf, slot, n / 24, out);
    return;
  }
  if (cfg.packet_slots >> slot & 1) {                      // n = 24 s
    packet_cells(cfg, slot, n / 24, static_cast<int64_t>(cif) * (n / 24), n / 24, out);
    return;
  }
  if (cfg.ts_slots >> slot & 1) {
    ts_bytes(cfg, slot, static_cast<int64_t>(cif) * n, n, out);
    return;
  }
  for (int i = 0; i < n; i += 8) {
    uint64_t v = key(cfg.seed, kDomPayload, (static_cast<uint64_t>(static_cast<uint32_t>(cif)) << 8) | static_cast<uint64_t>(slot), static_cast<uint64_t>(i));
    for (int b = 0; b < 8 && i + b < n; ++b) out[i + b] = static_cast<uint8_t>(v >> (8 * b));
  }
}

// ---- service information (dabhip_synth_cfg::si_mode; the directory's rules are in dabhip.h, "ensemble directory") -----------------------------
// The carousel: whole FIGs in a fixed order -- the ensemble label, FIG 0/9, FIG 0/10, then per slot its FIG 0/2, its label and, for a packet slot,
// its FIG 0/3 and (with FEC) its FIG 0/14.  Only FIG 0/10 depends on the CIF.
const char* si_kind_name(const dabhip_synth_cfg& cfg, int k)
{
  return (cfg.dabplus_slots >> k & 1) ? "DAB+" : (cfg.ts_slots >> k & 1) ? "TS" : (cfg.packet_slots >> k & 1) ? "PACKET" : "MP2";
}
std::vector<uint8_t> si_label_fig(int ext, uint32_t id, const char* text)
{
  std::vector<uint8_t> f;
  const int kl = ext == 5 ? 4 : 2;
  f.push_back(static_cast<uint8_t>(0x20 | (1 + kl + 18)));
  f.push_back(static_cast<uint8_t>(ext));                  // charset 0, OE 0
  for (int b = kl - 1; b >= 0; --b) f.push_back(static_cast<uint8_t>(id >> (8 * b)));
  const size_t n = std::strlen(text);
  for (size_t i = 0; i < 16; ++i) f.push_back(static_cast<uint8_t>(i < n ? text[i] : ' '));
  f.push_back(0xff);                                       // character flag field
  f.push_back(0x00);
  return f;
}
std::vector<std::vector<uint8_t>> si_carousel(const dabhip_synth_cfg& cfg, int cif)
{
  std::vector<std::vector<uint8_t>> figs;
  figs.push_back(si_label_fig(0, cfg.eid, "DABHIP SYNTH"));
  figs.push_back({0x04, 0x09, 0x00, 0xe1, 0x01});          // FIG 0/9: LTO 0, ECC 0xE1, international table 1
  {
    const int64_t t = std::max<int64_t>(0, static_cast<int64_t>(cfg.cif_count0) + cif) * 24;     // ms since MJD 60000, 00:00 UTC
    const uint32_t mjd = 60000 + static_cast<uint32_t>(t / 86400000), ms = static_cast<uint32_t>(t % 86400000);
    const uint32_t hours = ms / 3600000, minutes = ms / 60000 % 60, seconds = ms / 1000 % 60, milli = ms % 1000;
    const uint32_t w = mjd << 14 | 1u << 11 | hours << 6 | minutes;                              // rfu 0, LSI 0, rfa 0, UTC flag 1
    figs.push_back({0x07, 0x0a, static_cast<uint8_t>(w >> 24), static_cast<uint8_t>(w >> 16), static_cast<uint8_t>(w >> 8), static_cast<uint8_t>(w),
                    static_cast<uint8_t>(seconds << 2 | milli >> 8), static_cast<uint8_t>(milli)});
  }
  for (int k = 0; k < cfg.nsub && k < 64; ++k) {
    const int id = to_subchannel(cfg.sub[k]).id;
    const bool packet = cfg.packet_slots >> k & 1, ts = cfg.ts_slots >> k & 1, plus = cfg.dabplus_slots >> k & 1;
    const bool data = packet || ts;
    const uint32_t sid = data ? 0xE0001000u + static_cast<uint32_t>(k) : 0x1000u + static_cast<uint32_t>(k);
    std::vector<uint8_t> f = {static_cast<uint8_t>(data ? 8 : 6), static_cast<uint8_t>(data ? 0x22 : 0x02)};
    for (int b = (data ? 3 : 1); b >= 0; --b) f.push_back(static_cast<uint8_t>(sid >> (8 * b)));
    f.push_back(0x01);                                     // local 0, CAId 0, one component
    if (packet) { f.push_back(static_cast<uint8_t>(0xc0 | (k >> 6))); f.push_back(static_cast<uint8_t>((k & 63) << 2 | 2)); }       // TMId 3, SCId k, primary
    else { f.push_back(static_cast<uint8_t>(ts ? (0x40 | 24) : plus ? 63 : 0)); f.push_back(static_cast<uint8_t>(id << 2 | 2)); }
    figs.push_back(f);
    char text[24];
    std::snprintf(text, sizeof text, "SLOT %02d %s", k, si_kind_name(cfg, k));
    figs.push_back(si_label_fig(data ? 5 : 1, sid, text));
    if (packet) {
      int addr[3];
      packet_addresses(cfg, k, addr);
      figs.push_back({0x06, 0x03, static_cast<uint8_t>(k >> 4), static_cast<uint8_t>((k & 15) << 4), static_cast<uint8_t>(0x80 | 60),     // no SCCA; DG flag 1, DSCTy 60
                      static_cast<uint8_t>(id << 2 | addr[0] >> 8), static_cast<uint8_t>(addr[0])});
      if (cfg.packet_fec_slots >> k & 1) figs.push_back({0x02, 0x0e, static_cast<uint8_t>(id << 2 | 1)});
    }
  }
  return figs;
}
// Which FIGs of the carousel go where: the carousel is cut into loads, CIF c carries load c mod the number of loads.  A load takes FIGs in order,
// each into the first of the three FIBs with room left behind FIG 0/0 and FIG 0/1 (pos[f] bytes used); the first FIG that fits nowhere waits
// for the next load.  False: a FIG fits in no FIB at all.
bool si_loads(const std::vector<std::vector<uint8_t>>& figs, const int pos[3], std::vector<std::vector<std::pair<int, int>>>& loads)
{
  loads.clear();
  size_t next = 0;
  while (next < figs.size()) {
    int used[3] = {pos[0], pos[1], pos[2]};
    std::vector<std::pair<int, int>> load;
    for (; next < figs.size(); ++next) {
      int f = 0;
      while (f < 3 && used[f] + static_cast<int>(figs[next].size()) > 30) ++f;
      if (f == 3) break;
      used[f] += static_cast<int>(figs[next].size());
      load.emplace_back(f, static_cast<int>(next));
    }
    if (load.empty()) return false;
    loads.push_back(load);
  }
  return true;
}

// the three FIBs of one CIF: FIG 0/0 (ensemble, CIF counter) and FIG 0/1 (sub-channel
// organisation) entries packed greedily, then with si_mode the carousel's load, then end marker / padding and the FIB CRC.
// False: si_mode is set and a FIG of the carousel fits in no FIB.
bool build_fibs(const dabhip_synth_cfg& cfg, int cif, uint8_t* out96)
{
  const int count = ((cfg.cif_count0 + cif) % 5000 + 5000) % 5000;
  std::vector<std::vector<uint8_t>> entries;
  const Multiplex mux = multiplex_at(cfg, cif, true);
  for (int k = 0; k < mux.nsub; ++k) {
    const SubChannel sc = to_subchannel(mux.sub[k]);
    std::vector<uint8_t> e;
    e.push_back(static_cast<uint8_t>((sc.id << 2) | ((sc.start_cu >> 8) & 3)));
    e.push_back(static_cast<uint8_t>(sc.start_cu & 0xff));
    if (!sc.slform) {
      e.push_back(static_cast<uint8_t>(sc.uep_index & 0x3f));
    } else {
      e.push_back(static_cast<uint8_t>(0x80 | ((sc.protlev >> 2) << 4) | ((sc.protlev & 3) << 2) | ((sc.size_cu >> 8) & 3)));
      e.push_back(static_cast<uint8_t>(sc.size_cu & 0xff));
    }
    entries.push_back(e);
  }
  size_t next = 0;
  int used[3];
  for (int f = 0; f < 3; ++f) {
    uint8_t* fib = out96 + 32 * f;
    std::memset(fib, 0, 32);
    int pos = 0;
    if (f == 0) {
      const uint8_t fig00[6] = {0x05, 0x00, static_cast<uint8_t>(cfg.eid >> 8), static_cast<uint8_t>(cfg.eid & 0xff),
                                static_cast<uint8_t>(count / 250), static_cast<uint8_t>(count % 250)};
      std::memcpy(fib, fig00, 6);
      pos = 6;
    }
    if (next < entries.size() && pos + 2 + static_cast<int>(entries[next].size()) <= 30) {
      const int hdr = pos;
      pos += 2;
      int len = 1;
      while (next < entries.size() && pos + static_cast<int>(entries[next].size()) <= 30 && len + entries[next].size() <= 31) {
        std::memcpy(fib + pos, entries[next].data(), entries[next].size());
        pos += static_cast<int>(entries[next].size());
        len += static_cast<int>(entries[next].size());
        ++next;
      }
      fib[hdr] = static_cast<uint8_t>(len);   // FIG type 0, length
      fib[hdr + 1] = 0x01;                    // C/N=0 OE=0 P/D=0 extension 1
    }
    if (f == 2 && cfg.fib_patch_len > 0 && cif >= cfg.fib_patch_from_cif && pos == 0) {      // test vector: this FIB's content verbatim (dabhip.h)
      pos = std::min(cfg.fib_patch_len, 30);
      std::memcpy(fib, cfg.fib_patch, static_cast<size_t>(pos));
    }
    used[f] = pos;
  }
  if (cfg.si_mode) {
    const std::vector<std::vector<uint8_t>> figs = si_carousel(cfg, cif);
    std::vector<std::vector<std::pair<int, int>>> loads;
    if (!si_loads(figs, used, loads)) return false;
    const int nl = static_cast<int>(loads.size());
    for (const std::pair<int, int>& at : loads[static_cast<size_t>((cif % nl + nl) % nl)]) {
      const std::vector<uint8_t>& g = figs[static_cast<size_t>(at.second)];
      std::memcpy(out96 + 32 * at.first + used[at.first], g.data(), g.size());
      used[at.first] += static_cast<int>(g.size());
    }
  }
  for (int f = 0; f < 3; ++f) {
    uint8_t* fib = out96 + 32 * f;
    const int pos = used[f];
    if (pos < 30) fib[pos] = 0xff;            // end marker, rest zero padding
    const uint16_t crc = static_cast<uint16_t>(~crc16_ccitt(fib, 30));
    fib[30] = static_cast<uint8_t>(crc >> 8);
    fib[31] = static_cast<uint8_t>(crc & 0xff);
  }
  return true;
}

bool si_fits(const dabhip_synth_cfg& cfg)
{
  uint8_t fibs[96];
  return build_fibs(cfg, 0, fibs);
}

// keep the mother-code bits the puncturing plan transmits
void puncture(const std::vector<uint8_t>& mother, const PuncturePlan& plan, std::vector<uint8_t>& out)
{
  size_t x = 0;
  for (int s = 0; s < 4; ++s) {
    const uint32_t m = puncture_mask(plan.pi[s]);
    for (int i = 0; i < 128 * plan.blocks[s]; ++i, ++x)
      if ((m >> (i & 31)) & 1u) out.push_back(mother[x]);
  }
  const uint32_t mt = puncture_mask(8);
  for (int i = 0; i < 24; ++i, ++x)
    if ((mt >> i) & 1u) out.push_back(mother[x]);
}

// logical (pre time-interleaving) CIF r: 55296 bits
void logical_cif(const dabhip_synth_cfg& cfg, int r, uint8_t* bits)
{
  for (int i = 0; i < kCifBits; i += 64) {
    const uint64_t v = key(cfg.seed, kDomFiller, static_cast<uint64_t>(static_cast<uint32_t>(r)), static_cast<uint64_t>(i));
    for (int b = 0; b < 64; ++b) bits[i + b] = static_cast<uint8_t>((v >> b) & 1u);
  }
  if (r < 0) return;   // before the start of the transmission: filler only
  std::vector<uint8_t> data, coded;
  const Multiplex mux = multiplex_at(cfg, r, false);
  for (int k = 0; k < mux.nsub; ++k) {
    const SubChannel sc = to_subchannel(mux.sub[k]);
    const int nbytes = sc.bitrate * 3;
    data.resize(static_cast<size_t>(nbytes));
    payload_bytes(cfg, r, k, data.data(), nbytes);
    energy_dispersal(data.data(), data.size());
    const std::vector<uint8_t> mother = conv_encode(data.data(), nbytes * 8);
    coded.clear();
    puncture(mother, puncture_plan(sc), coded);
    std::memcpy(bits + sc.start_cu * 64, coded.data(), coded.size());
  }
}

void fic_bits_of_cif(const dabhip_synth_cfg& cfg, int cif, uint8_t* bits2304)
{
  uint8_t fibs[96];
  build_fibs(cfg, cif, fibs);
  energy_dispersal(fibs, 96);
  const std::vector<uint8_t> mother = conv_encode(fibs, 768);
  std::vector<uint8_t> coded;
  puncture(mother, fic_plan(), coded);
  std::memcpy(bits2304, coded.data(), 2304);
}

// in-place radix-2 complex DFT, sign = +1 for the synthesis direction
void fft2048(double* re, double* im, int sign)
{
  constexpr int n = 2048;
  struct Twiddles {
    std::vector<double> r, i;
    Twiddles() : r(n / 2), i(n / 2)
    {
      for (int k = 0; k < n / 2; ++k) { r[k] = std::cos(2 * M_PI * k / n); i[k] = std::sin(2 * M_PI * k / n); }
    }
  };
  static const Twiddles tw;   // thread-safe one-time initialisation
  const std::vector<double>&wr = tw.r, &wi = tw.i;
  for (int i = 1, j = 0; i < n; ++i) {
    int bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
  }
  for (int len = 2; len <= n; len <<= 1) {
    const int step = n / len;
    for (int i = 0; i < n; i += len)
      for (int k = 0; k < len / 2; ++k) {
        const double cr = wr[k * step], ci = sign * wi[k * step];
        const int a = i + k, b = a + len / 2;
        const double tr = re[b] * cr - im[b] * ci, ti = re[b] * ci + im[b] * cr;
        re[b] = re[a] - tr; im[b] = im[a] - ti;
        re[a] += tr; im[a] += ti;
      }
  }
}

struct Gauss {
  uint64_t seed, ctr = 0;
  bool have = false;
  double spare = 0;
  double next()
  {
    if (have) { have = false; return spare; }
    const uint64_t a = key(seed, kDomNoise, ctr, 0), b = key(seed, kDomNoise, ctr, 1);
    ++ctr;
    const double u1 = (static_cast<double>(a >> 11) + 1.0) / 9007199254740993.0;
    const double u2 = static_cast<double>(b >> 11) / 9007199254740992.0;
    const double r = std::sqrt(-2.0 * std::log(u1));
    spare = r * std::sin(2 * M_PI * u2);
    have = true;
    return r * std::cos(2 * M_PI * u2);
  }
};

// The channel between modulator and receiver (dabhip_channel_cfg): a chain of sample-by-sample stages, each of which is skipped when its parameters
// are zero, so that an ideal channel hands the modulator's samples through untouched (the captures of rounds 1-4, byte for byte).
// Not part of the receive path and of no parity claim: whatever IQ it makes, the reference, the oracle and the GPU get the same bytes.
class Channel {
 public:
  explicit Channel(const dabhip_synth_cfg& cfg)
      : c_(cfg.channel), cfo_turns_(cfg.cfo_hz / 2048000.0), echo_(c_.echo_delay[0] || c_.echo_delay[1]), hist_r_(kHist, 0.0), hist_i_(kHist, 0.0),
        ring_r_(kRing, 0.0), ring_i_(kRing, 0.0)
  {
    rate_ = 1.0 + c_.sro_ppm * 1e-6;
    iq_g_ = std::pow(10.0, c_.iq_gain_db / 20.0);
    iq_c_ = std::cos(c_.iq_phase_deg * M_PI / 180.0);
    iq_s_ = std::sin(c_.iq_phase_deg * M_PI / 180.0);
    iq_ = c_.iq_gain_db != 0.0 || c_.iq_phase_deg != 0.0;
    for (int k = 0; k < 2 * kHalf; ++k) {
      tab_c_[k] = std::cos(M_PI * (k - kHalf + 1) / kHalf);
      tab_s_[k] = std::sin(M_PI * (k - kHalf + 1) / kHalf);
    }
  }
  // modulator sample n (in order); out(re, im) receives the receiver-side samples, in order
  template <class Out>
  void push(double xr, double xi, Out&& out)
  {
    const long long n = n_++;
    if (echo_) {
      hist_r_[n & (kHist - 1)] = xr;
      hist_i_[n & (kHist - 1)] = xi;
      double yr = xr, yi = xi;
      for (int e = 0; e < 2; ++e) {
        const int d = c_.echo_delay[e];
        if (!d || n < d) continue;
        const double ph = 2 * M_PI * std::fmod(c_.echo_phase[e] + c_.echo_doppler_hz[e] / 2048000.0 * static_cast<double>(n), 1.0);
        const double gr = c_.echo_gain[e] * std::cos(ph), gi = c_.echo_gain[e] * std::sin(ph);
        const double pr = hist_r_[(n - d) & (kHist - 1)], pi = hist_i_[(n - d) & (kHist - 1)];
        yr += gr * pr - gi * pi;
        yi += gr * pi + gi * pr;
      }
      xr = yr;
      xi = yi;
    }
    if (c_.fade_depth != 0.0) {
      const double a = 1.0 - c_.fade_depth * 0.5 * (1.0 - std::cos(2 * M_PI * std::fmod(c_.fade_hz / 2048000.0 * static_cast<double>(n), 1.0)));
      xr *= a;
      xi *= a;
    }
    if (cfo_turns_ != 0.0) {
      const double ph = 2 * M_PI * std::fmod(cfo_turns_ * static_cast<double>(n), 1.0);
      const double c = std::cos(ph), s = std::sin(ph), r = xr * c - xi * s;
      xi = xr * s + xi * c;
      xr = r;
    }
    if (c_.sro_ppm == 0.0) { receiver(xr, xi, out); return; }
    ring_r_[n & (kRing - 1)] = xr;
    ring_i_[n & (kRing - 1)] = xi;
    // every output whose 2 kHalf taps end at or before sample n: output m sits at input position m * rate_
    for (;;) {
      const double pos = static_cast<double>(m_) * rate_;
      const long long i0 = static_cast<long long>(std::floor(pos));
      if (i0 + kHalf > n) break;
      const double f = pos - static_cast<double>(i0);
      double yr = 0, yi = 0;
      if (f == 0.0) {
        yr = ring_r_[i0 & (kRing - 1)];
        yi = ring_i_[i0 & (kRing - 1)];
      } else {
        // taps k = -kHalf+1 .. kHalf at distance t = k - f: sinc(t) = -(-1)^k sin(pi f) / (pi t), Hann window 0.5 (1 + cos(pi t / kHalf))
        const double sf = std::sin(M_PI * f), cw = std::cos(M_PI * f / kHalf), sw = std::sin(M_PI * f / kHalf);
        double sum = 0;
        for (int j = 0; j < 2 * kHalf; ++j) {
          const int k = j - kHalf + 1;
          const long long idx = i0 + k;
          const double t = static_cast<double>(k) - f;
          const double w = 0.5 * (1.0 + tab_c_[j] * cw + tab_s_[j] * sw);
          const double h = ((k & 1) ? sf : -sf) / (M_PI * t) * w;
          sum += h;
          if (idx < 0) continue;
          yr += h * ring_r_[idx & (kRing - 1)];
          yi += h * ring_i_[idx & (kRing - 1)];
        }
        yr /= sum;
        yi /= sum;
      }
      ++m_;
      receiver(yr, yi, out);
    }
  }

 private:
  template <class Out>
  void receiver(double xr, double xi, Out&& out)
  {
    if (iq_) xi = iq_g_ * (xi * iq_c_ + xr * iq_s_);
    out(xr, xi);
  }
  static constexpr int kHist = 2048, kRing = 64, kHalf = 8;
  dabhip_channel_cfg c_;
  double cfo_turns_, rate_ = 1.0, iq_g_ = 1.0, iq_c_ = 1.0, iq_s_ = 0.0;
  bool echo_, iq_ = false;
  long long n_ = 0, m_ = 0;
  std::vector<double> hist_r_, hist_i_, ring_r_, ring_i_;
  double tab_c_[2 * kHalf], tab_s_[2 * kHalf];
};

}  // namespace

bool synth_channel_active(const dabhip_synth_cfg& cfg) { return channel_active(cfg.channel); }

bool synth_tii_active(const dabhip_synth_cfg& cfg)
{
  for (const dabhip_tii_cfg& t : cfg.tii)
    if (t.enabled) return true;
  return false;
}

uint64_t synth_noise_key(uint64_t seed, uint64_t ctr, uint64_t which) { return key(seed, kDomNoise, ctr, which); }

bool synth_validate(const dabhip_synth_cfg& cfg) { return validate(cfg); }

double synth_noise_rms(const dabhip_synth_cfg& cfg)
{
  return cfg.snr_db >= 100.0 ? 0.0 : cfg.amplitude * std::sqrt(static_cast<double>(kCarriers)) / std::pow(10.0, cfg.snr_db / 20.0) / std::sqrt(2.0);
}

SymbolBits::SymbolBits(const dabhip_synth_cfg& cfg) : cfg_(cfg), window_(16, std::vector<uint8_t>(kCifBits))
{
  for (int r = -15; r < 0; ++r) logical_cif(cfg_, r, window_[(r + 16) & 15].data());
}

void SymbolBits::next_tf(uint8_t* symbits)
{
  static const int tmap[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};
  for (int q = 0; q < 4; ++q) {
    const int c = 4 * tf_ + q;
    fic_bits_of_cif(cfg_, c, symbits + 2304 * q);
    logical_cif(cfg_, c, window_[c & 15].data());
    // time interleaving: inverse of misc.c:29-39 (tx CIF c carries logical CIF c - map[i&15])
    uint8_t* txcif = symbits + 3 * kBitsPerSym + static_cast<size_t>(q) * kCifBits;
    for (int i = 0; i < kCifBits; ++i) txcif[i] = window_[(c - tmap[i & 15]) & 15][i];
  }
  ++tf_;
}

}  // namespace dabhip

using namespace dabhip;

extern "C" int dabhip_synth_preset(int preset, dabhip_synth_cfg* cfg)
{
  if (!cfg) return -1;
  std::memset(cfg, 0, sizeof *cfg);
  cfg->eid = 0xC181;
  cfg->seed = 1;
  cfg->amplitude = 1.0;
  cfg->snr_db = 1000.0;
  auto uep = [&](int id, int cu, int idx) { cfg->sub[cfg->nsub++] = dabhip_subch_cfg{id, cu, 0, idx, 0, 0}; };
  auto eep = [&](int id, int cu, int lev, int size) { cfg->sub[cfg->nsub++] = dabhip_subch_cfg{id, cu, 1, 0, lev, size}; };
  if (preset == 0) {          // 12 sub-channels, 1136 kbit/s, 862 of 864 CU
    uep(1, 0, 35); uep(2, 96, 35); uep(3, 192, 35); uep(4, 288, 35);   // 128 kbit/s PL3
    uep(5, 384, 45); uep(6, 524, 45);                                  // 192 kbit/s PL3
    eep(7, 664, 2, 48); eep(8, 712, 2, 48);                            // 64 kbit/s 3-A
    eep(9, 760, 0, 48);                                                // 32 kbit/s 1-A
    eep(10, 808, 5, 42);                                               // 64 kbit/s 2-B
    eep(11, 850, 1, 8);                                                // 8 kbit/s 2-A (special case)
    eep(12, 858, 3, 4);                                                // 8 kbit/s 4-A
  } else if (preset == 1) {   // 4 light sub-channels
    uep(1, 0, 35); eep(2, 100, 2, 48); eep(5, 200, 5, 21); eep(9, 300, 1, 8);
  } else {
    set_error("synth: unknown preset");
    return -1;
  }
  return 0;
}

extern "C" size_t dabhip_synth_bytes(const dabhip_synth_cfg* cfg, int ntf)
{
  if (!cfg || ntf <= 0) return 0;
  const size_t n = static_cast<size_t>(ntf) * kTfSamples;
  if (cfg->channel.sro_ppm == 0.0) return (n - static_cast<size_t>(cfg->skip_samples)) * 2;
  return (static_cast<size_t>(static_cast<double>(n) / (1.0 + cfg->channel.sro_ppm * 1e-6)) + 16 - static_cast<size_t>(cfg->skip_samples)) * 2;   // upper bound
}

extern "C" int dabhip_synth_payload(const dabhip_synth_cfg* cfg, int cif_index, int slot, uint8_t* out, int cap)
{
  if (!cfg) { set_error("synth_payload: bad slot"); return -1; }
  const Multiplex mux = multiplex_at(*cfg, cif_index, false);
  if (slot < 0 || slot >= mux.nsub) { set_error("synth_payload: bad slot"); return -1; }
  if ((cfg->dabplus_slots || cfg->packet_slots || cfg->packet_fec_slots || cfg->ts_slots) && !validate(*cfg)) return -1;
  const int n = to_subchannel(mux.sub[slot]).bitrate * 3;
  if (cap < n) { set_error("synth_payload: buffer too small"); return -1; }
  payload_bytes(*cfg, cif_index, slot, out, n);
  return n;
}

extern "C" int dabhip_synth_dabplus_superframe(const dabhip_synth_cfg* cfg, int sf_index, int slot, uint8_t* out, int cap)
{
  if (!cfg || !out || slot < 0 || slot >= cfg->nsub || slot >= 64 || !(cfg->dabplus_slots >> slot & 1)) {
    set_error("synth_dabplus_superframe: not a DAB+ slot");
    return -1;
  }
  if (!validate(*cfg)) return -1;
  const int s = to_subchannel(cfg->sub[slot]).bitrate / 8;
  if (cap < kRsK * s) { set_error("synth_dabplus_superframe: buffer too small"); return -1; }
  dabplus_superframe(*cfg, sf_index, slot, s, out);
  return kRsK * s;
}

namespace {
bool packet_slot_ok(const dabhip_synth_cfg* cfg, int slot, const char* who)
{
  if (!cfg || slot < 0 || slot >= cfg->nsub || slot >= 64 || !(cfg->packet_slots >> slot & 1)) {
    set_error(std::string(who) + ": not a packet-mode slot");
    return false;
  }
  return validate(*cfg);
}
}  // namespace

extern "C" int dabhip_synth_packet_addresses(const dabhip_synth_cfg* cfg, int slot, int32_t* out3)
{
  if (!out3 || !packet_slot_ok(cfg, slot, "synth_packet_addresses")) return -1;
  int a[3];
  const int n = packet_addresses(*cfg, slot, a);
  for (int i = 0; i < n; ++i) out3[i] = a[i];
  return n;
}

extern "C" int dabhip_synth_packet_cells(const dabhip_synth_cfg* cfg, int slot, int64_t cell_index, int ncells, uint8_t* out, int cap)
{
  if (!out || ncells < 0 || !packet_slot_ok(cfg, slot, "synth_packet_cells")) return -1;
  if (cap / kPkCell < ncells) { set_error("synth_packet_cells: buffer too small"); return -1; }
  packet_cells(*cfg, slot, to_subchannel(cfg->sub[slot]).bitrate / 8, cell_index, ncells, out);
  return ncells * kPkCell;
}

extern "C" int dabhip_synth_packet_group(const dabhip_synth_cfg* cfg, int slot, int address, int n, uint8_t* out, int cap)
{
  if (n < 0 || !packet_slot_ok(cfg, slot, "synth_packet_group")) return -1;
  const bool fec = cfg->packet_fec_slots >> slot & 1;
  const int ncells = fec ? kPkDataCells : to_subchannel(cfg->sub[slot]).bitrate / 8;
  std::vector<uint8_t> cells(static_cast<size_t>(ncells) * kPkCell);
  int seen = 0;
  for (int j = 0; j < (1 << 16); ++j) {
    PacketGroupList groups;
    packet_unit(*cfg, slot, j, ncells, cells.data(), &groups);
    for (const auto& g : groups) {
      if (g.first != address || seen++ != n) continue;
      const int len = static_cast<int>(g.second.size());
      if (out && cap > 0) std::memcpy(out, g.second.data(), static_cast<size_t>(std::min(len, cap)));
      return len;
    }
  }
  set_error("synth_packet_group: no such group");
  return -1;
}

extern "C" int dabhip_synth_ts_word(const dabhip_synth_cfg* cfg, int slot, int64_t n, uint8_t* out204)
{
  if (!cfg || !out204 || slot < 0 || slot >= cfg->nsub || slot >= 64 || !(cfg->ts_slots >> slot & 1)) {
    set_error("synth_ts_word: not an MPEG-2 TS slot");
    return -1;
  }
  if (!validate(*cfg)) return -1;
  ts_word(*cfg, slot, n, out204);
  return kTsSlot;
}

extern "C" int dabhip_synth_fibs(const dabhip_synth_cfg* cfg, int cif_index, uint8_t* out96)
{
  if (!cfg || !out96) return -1;
  if (cfg->si_mode && !validate(*cfg)) return -1;
  build_fibs(*cfg, cif_index, out96);
  return 96;
}

extern "C" int64_t dabhip_synth_generate(const dabhip_synth_cfg* cfg, int ntf, uint8_t* iq, size_t cap)
{
  if (!cfg || !iq || ntf <= 0) { set_error("synth_generate: bad arguments"); return -1; }
  if (!validate(*cfg)) return -1;
  const size_t total = dabhip_synth_bytes(cfg, ntf);
  if (cap < total) { set_error("synth_generate: buffer too small"); return -1; }

  const auto& qpsk_of_carrier = carrier_to_qpsk();
  const auto& prs = prs_quarter_turns();
  SymbolBits bits(*cfg);                                                  // logical CIFs in a sliding window of 16
  const double noise_rms_rail = synth_noise_rms(*cfg);
  Gauss gauss{cfg->seed};
  std::vector<uint8_t> symbits(static_cast<size_t>(kBitsPerSym) * 75);   // data symbols 1..75 of one TF
  std::vector<double> re(2048), im(2048);
  std::vector<uint8_t> phase(kCarriers);                                  // in eighth turns
  static const double c8[8] = {1, M_SQRT1_2, 0, -M_SQRT1_2, -1, -M_SQRT1_2, 0, M_SQRT1_2};
  static const double s8[8] = {0, M_SQRT1_2, 1, M_SQRT1_2, 0, -M_SQRT1_2, -1, -M_SQRT1_2};
  size_t outpos = 0;
  long long sample_index = 0;                             // receiver-side sample count
  Channel channel(*cfg);                                  // echoes, fading, carrier offset, sample-rate offset, I/Q imbalance
  auto quantise = [&](double xr, double xi) {
    if (sample_index++ < cfg->skip_samples) return;
    if (outpos + 2 > cap) return;
    if (noise_rms_rail > 0) { xr += noise_rms_rail * gauss.next(); xi += noise_rms_rail * gauss.next(); }
    double a = std::floor(127.0 + xr + 0.5), b = std::floor(127.0 + xi + 0.5);
    a = a < 1 ? 1 : (a > 254 ? 254 : a);
    b = b < 1 ? 1 : (b > 254 ? 254 : b);
    iq[outpos++] = static_cast<uint8_t>(a);
    iq[outpos++] = static_cast<uint8_t>(b);
  };
  auto emit = [&](double xr, double xi) { channel.push(xr, xi, quantise); };

  // one period of the TII symbol (include/dabhip.h, "TII"): the enabled combs' carriers, both of a pair with the phase reference of the lower one
  const bool tii = synth_tii_active(*cfg);
  std::vector<double> tii_re(2048, 0.0), tii_im(2048, 0.0);
  if (tii) {
    for (const dabhip_tii_cfg& t : cfg->tii) {
      if (!t.enabled) continue;
      int16_t k[kTiiCarriers];
      tii_carriers(t.main_id, t.sub_id, k);
      const double level = cfg->amplitude * std::pow(10.0, t.level_db / 20.0);
      for (int i = 0; i < kTiiCarriers; ++i) {
        const int lower = k[i & ~1];
        const int q = 2 * prs[lower < 0 ? lower + 768 : lower + 767];      // eighth turns
        tii_re[(k[i] + 2048) % 2048] += level * c8[q];
        tii_im[(k[i] + 2048) % 2048] += level * s8[q];
      }
    }
    fft2048(tii_re.data(), tii_im.data(), +1);
  }

  for (int tf = 0; tf < ntf; ++tf) {
    bits.next_tf(symbits.data());
    if (tii && ((tf + cfg->tii_phase) & 1) == 0)
      for (int n = 0; n < kNullSamples; ++n) emit(tii_re[(n + 2048 - 608) % 2048], tii_im[(n + 2048 - 608) % 2048]);
    else
      for (int n = 0; n < kNullSamples; ++n) emit(0, 0);
    for (int l = 0; l < kSymbolsPerTf; ++l) {
      if (l == 0) {
        for (int k = 0; k < kCarriers; ++k) phase[k] = static_cast<uint8_t>(2 * prs[k]);
      } else {
        const uint8_t* p = symbits.data() + static_cast<size_t>(l - 1) * kBitsPerSym;
        for (int k = 0; k < kCarriers; ++k) {
          const int n = qpsk_of_carrier[k];
          static const uint8_t inc[4] = {1, 3, 7, 5};   // (b0,b1): 00->45deg 10->135 01->315 11->225
          phase[k] = static_cast<uint8_t>((phase[k] + inc[p[n] | (p[1536 + n] << 1)]) & 7);
        }
      }
      std::fill(re.begin(), re.end(), 0.0);
      std::fill(im.begin(), im.end(), 0.0);
      for (int k = 0; k < kCarriers; ++k) {
        const int bin = k < 768 ? 1280 + k : k - 767;
        re[bin] = cfg->amplitude * c8[phase[k]];
        im[bin] = cfg->amplitude * s8[phase[k]];
      }
      fft2048(re.data(), im.data(), +1);
      for (int n = 2048 - kCpSamples; n < 2048; ++n) emit(re[n], im[n]);
      for (int n = 0; n < 2048; ++n) emit(re[n], im[n]);
    }
  }
  return static_cast<int64_t>(outpos);
}
