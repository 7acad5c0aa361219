// edi_units.cpp — the host-and-device header of the EDI stage (csrc/edi_plan.hpp) under ASan + UBSan, as a stand-alone program:
//   1. the size rule over every l in 13..7000, recover 0..5 and max_frag in {64, 65, 255, 1400, 1472}: z < c, k <= 207, f s >= B, f s - B < f,
//      floor(f s / (k + 48)) = c, s <= max_frag, and -- counted from the index map -- any `recover` fragments cover at most 48 bytes of any
//      one code word; for the l a frame can give (<= 6620), c <= 32 and f <= 132, the kernels' array sizes;
//   2. the CRC combine rule against the bytewise CRC for every split of messages of 1..300 bytes and 200 random splits of a 6.7 KB one, and
//      the 64-piece split and scan the assemble kernel makes, at every length;
//   3. with arguments `frames.eti mode recover max_frag seq0 out.edi`: one stream through the stage's steps on the host, the way the kernels
//      take them (plan, the FCTH / SEQ rule, the AF packet with the CRC of its 64 pieces, the parity by the feedback table, the gather a byte at a
//      time), every buffer on the heap at exactly its planned size; the test compares out.edi with the model's bytes.
// Prints "ok edi-units" and what it counted.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "../../dabtools_amd/csrc/edi_plan.hpp"

using namespace dabhip;

namespace {
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// the bytes of each code word that each fragment carries, from the index map: the most any m fragments cover of one code word
int worst_cover(const EdiPlan& p, int m)
{
  std::vector<int> count(static_cast<size_t>(p.c) * p.f, 0);
  for (int i = 0; i < p.f; ++i)
    for (int j = 0; j < p.s; ++j) {
      const int b = edi_block_index(p, i, j);
      if (b < p.B) ++count[static_cast<size_t>(b / (p.k + kEdiRsP)) * p.f + i];
    }
  int worst = 0;
  for (int w = 0; w < p.c; ++w) {
    std::vector<int> row(count.begin() + static_cast<size_t>(w) * p.f, count.begin() + static_cast<size_t>(w + 1) * p.f);
    std::sort(row.begin(), row.end(), [](int a, int b) { return a > b; });
    int sum = 0;
    for (int i = 0; i < m && i < p.f; ++i) sum += row[i];
    worst = std::max(worst, sum);
  }
  return worst;
}

long size_rule(int* max_f, int* max_cover)
{
  const int frags[5] = {64, 65, 255, 1400, 1472};
  std::set<std::tuple<int, int, int, int, int>> seen;
  long n = 0;
  for (int l = 13; l <= 7000; ++l)
    for (int m = 0; m <= 5; ++m)
      for (int F : frags) {
        CHECK(edi_plan_check(l, 2, m, F) == 0);
        const EdiPlan p = edi_plan(l, 2, m, F);
        CHECK(p.c == (l + 206) / 207 && p.k <= kEdiRsK && p.k >= 1 && p.z >= 0 && p.z < p.c && p.c * p.k - p.z == l);
        CHECK(p.B == p.c * (p.k + kEdiRsP) && p.f * p.s >= p.B && p.f * p.s - p.B < p.f);
        CHECK(p.f * p.s / (p.k + kEdiRsP) == p.c);
        CHECK(p.s <= F && p.s >= 1);
        if (l <= kEdiMaxL) {
          CHECK(p.c <= kEdiMaxChunks && p.f <= kEdiMaxFrags && l + p.z + 3 <= kEdiWorkStride);
          *max_f = std::max(*max_f, p.f);
        }
        if (seen.insert(std::make_tuple(p.c, p.k, p.f, p.s, m)).second) {
          const int cover = worst_cover(p, m);
          CHECK(cover <= kEdiRsP);
          *max_cover = std::max(*max_cover, cover);
        }
        // modes 0 and 1 on the same l
        const EdiPlan q = edi_plan(l, 1, 0, F), a = edi_plan(l, 0, 0, 0);
        CHECK(q.f == (l + F - 1) / F && q.s <= F && (q.f - 1) * q.s < l && q.f * q.s >= l && q.B == l && a.f == 1 && a.s == l);
        CHECK(edi_out_bytes(q, 1, l) == edi_packet_offset(q, 1, q.f - 1) + edi_packet_bytes(q, 1, l, q.f - 1));
        CHECK(edi_out_bytes(p, 2, l) == edi_packet_offset(p, 2, p.f - 1) + edi_packet_bytes(p, 2, l, p.f - 1));
        if (l <= kEdiMaxL) CHECK(q.f <= kEdiMaxFrags);
        ++n;
      }
  CHECK(edi_plan_check(12, 0, 0, 0) == 1 && edi_plan_check(kEdiPlanMaxL + 1, 0, 0, 0) == 1 && edi_plan_check(13, 3, 0, 0) == 2 && edi_plan_check(13, -1, 0, 0) == 2);
  CHECK(edi_plan_check(13, 2, 6, 64) == 3 && edi_plan_check(13, 2, -1, 64) == 3 && edi_plan_check(13, 1, 6, 64) == 0 && edi_plan_check(13, 1, 0, 63) == 4);
  CHECK(edi_plan_check(13, 2, 0, 1473) == 4 && edi_plan_check(13, 0, 9, 0) == 0);
  return n;
}

// the CRC the way the assemble kernel's wave takes it: 64 pieces that end at n, n - piece, ..., the start value as the complement of the first
// two bytes, and the prefix scan with a multiplier that squares from step to step
uint16_t wave_crc(const uint8_t* p, int n)
{
  const int piece = edi_crc_piece(n);
  uint16_t v[64], mult = edi_crc_run(1, std::vector<uint8_t>(static_cast<size_t>(piece), 0).data(), piece);
  CHECK(mult == edi_crc_shift(1, piece));
  for (int l = 0; l < 64; ++l) {
    const int e = n - (63 - l) * piece, a = std::max(e - piece, 0);
    v[l] = 0;
    for (int i = a; i < e; ++i) v[l] = edi_crc_byte(v[l], static_cast<uint8_t>(i < 2 ? p[i] ^ 0xFF : p[i]));
  }
  for (int d = 1; d < 64; d <<= 1) {
    for (int l = 63; l >= d; --l) v[l] = static_cast<uint16_t>(v[l] ^ edi_crc_mulmod(v[l - d], mult));
    mult = edi_crc_mulmod(mult, mult);
  }
  return static_cast<uint16_t>(~v[63]);
}

long crc_rule()
{
  const uint8_t check[9] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
  CHECK(edi_crc16(check, 9) == 0xD64E);
  std::mt19937 rng(7);
  long n = 0;
  const auto split_ok = [&](const uint8_t* msg, int len, int at) {
    const uint16_t whole = edi_crc_run(0xFFFF, msg, len);
    const uint16_t a = edi_crc_run(0xFFFF, msg, at), b = edi_crc_run(0, msg + at, len - at);
    CHECK(edi_crc_combine(a, b, len - at) == whole);
    // and the start value as a term of its own
    CHECK((edi_crc_shift(0xFFFF, len) ^ edi_crc_shift(edi_crc_run(0, msg, at), len - at) ^ b) == whole);
    ++n;
  };
  for (int len = 1; len <= 300; ++len) {
    uint8_t* msg = new uint8_t[len];
    for (int i = 0; i < len; ++i) msg[i] = static_cast<uint8_t>(rng());
    for (int at = 0; at <= len; ++at) split_ok(msg, len, at);
    delete[] msg;
  }
  const int big = 6700;
  uint8_t* msg = new uint8_t[big];
  for (int i = 0; i < big; ++i) msg[i] = static_cast<uint8_t>(rng());
  for (int i = 0; i < 200; ++i) split_ok(msg, big, static_cast<int>(rng() % (big + 1)));
  // the assemble kernel's split, at every length an AF packet can have and a few more
  for (int len = 2; len <= big; len += (len < 700 ? 1 : 37)) {
    CHECK(wave_crc(msg, len) == edi_crc16(msg, len));
    ++n;
  }
  delete[] msg;
  return n;
}

void rs_rule()
{
  uint8_t g[kEdiRsP + 1];
  edi_rs_generator(g);
  CHECK(g[kEdiRsP] == 1);
  uint8_t x = 1;
  for (int e = 0; e < 255; ++e) {                      // g(alpha^e) = 0 exactly for e < 48
    uint8_t v = 0;
    for (int i = kEdiRsP; i >= 0; --i) v = static_cast<uint8_t>(edi_gmul(v, x) ^ g[i]);
    CHECK((v == 0) == (e < kEdiRsP));
    x = edi_gmul(x, 2);
  }
  std::vector<uint8_t> table(256 * kEdiRsP);
  edi_rs_table_fill(table.data());
  uint8_t* chunk = new uint8_t[kEdiRsK]();
  uint8_t par[kEdiRsP];
  edi_rs_parity(table.data(), chunk, kEdiRsK, par);
  for (int j = 0; j < kEdiRsP; ++j) CHECK(par[j] == 0);
  chunk[kEdiRsK - 1] = 1;                              // x^48 mod g = g without its leading term
  edi_rs_parity(table.data(), chunk, kEdiRsK, par);
  for (int j = 0; j < kEdiRsP; ++j) CHECK(par[j] == g[kEdiRsP - 1 - j]);
  delete[] chunk;
}

std::vector<uint8_t> read_file(const char* path)
{
  std::vector<uint8_t> v;
  FILE* fp = std::fopen(path, "rb");
  CHECK(fp != nullptr);
  uint8_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, fp)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(fp);
  return v;
}

// one stream through the stage on the host
long host_stage(const char* in, int mode, int recover, int max_frag, int seq0, const char* outpath)
{
  CHECK(edi_plan_check(kEdiMinL, mode, recover, max_frag) == 0);
  const std::vector<uint8_t> all = read_file(in);
  CHECK(all.size() % kEdiEti == 0);
  std::vector<uint8_t> table(256 * kEdiRsP);
  edi_rs_table_fill(table.data());
  FILE* out = std::fopen(outpath, "wb");
  CHECK(out != nullptr);
  bool started = false;
  int last_fct = 0, fcth = 0, seq = seq0;
  long packets = 0;
  for (size_t at = 0; at < all.size(); at += kEdiEti) {
    uint8_t* f = new uint8_t[kEdiEti];                 // a frame alone on the heap: a read past it is seen
    std::memcpy(f, all.data() + at, kEdiEti);
    const EdiHead h = edi_parse(f);
    if (!h.valid) { delete[] f; continue; }
    if (started && h.fct < last_fct) fcth = (fcth + 1) % kEdiFcthMod;
    started = true;
    last_fct = h.fct;
    const EdiPlan p = edi_plan(h.l, mode, recover, max_frag);
    // assemble: l bytes and the z zeros behind them, no more
    uint8_t* pk = new uint8_t[h.l + p.z]();
    edi_put_af_head(pk, static_cast<uint32_t>(h.tag_bytes), static_cast<uint32_t>(seq));
    edi_put_ptr(pk + kEdiAfHead);
    edi_put_deti(pk + kEdiAfHead + kEdiPtrItem, h, fcth);
    int dst = kEdiAfHead + kEdiPtrItem + kEdiDetiHead, src = 12 + 4 * h.nst;
    if (h.ficf) {
      std::memcpy(pk + dst, f + src, kEdiFic);
      dst += kEdiFic;
      src += kEdiFic;
    }
    for (int i = 0; i < h.nst; ++i) {
      const int n = 8 * edi_stc_stl(f, i);
      edi_put_est(pk + dst, i + 1, f + 8 + 4 * i);
      std::memcpy(pk + dst + kEdiEstHead, f + src, static_cast<size_t>(n));
      dst += kEdiEstHead + n;
      src += n;
    }
    CHECK(dst + h.tag_pad + 2 == h.l && src <= kEdiMstEnd);
    CHECK(wave_crc(pk, h.l - 2) == edi_crc16(pk, h.l - 2));
    edi_put16(pk + h.l - 2, wave_crc(pk, h.l - 2));
    uint8_t* par = new uint8_t[std::max(1, p.c * kEdiRsP)];
    for (int ci = 0; ci < p.c; ++ci) edi_rs_parity(table.data(), pk + ci * p.k, p.k, par + ci * kEdiRsP);
    // fragment: every packet in a buffer of exactly its size
    const int hb = edi_pf_head_bytes(mode);
    long total = 0;
    for (int i = 0; i < p.f; ++i) {
      const int n = edi_packet_bytes(p, mode, h.l, i);
      CHECK(edi_packet_offset(p, mode, i) == total);
      uint8_t* o = new uint8_t[n];
      if (mode) CHECK(edi_put_pf(o, static_cast<uint32_t>(seq), static_cast<uint32_t>(i), static_cast<uint32_t>(p.f), mode == 2, static_cast<uint32_t>(n - hb),
                                 static_cast<uint32_t>(p.k), static_cast<uint32_t>(p.z)) == hb);
      for (int j = 0; j < n - hb; ++j) {
        uint8_t v;
        if (mode == 0) v = pk[j];
        else if (mode == 1) v = pk[i * p.s + j];
        else {
          const int b = edi_block_index(p, i, j), ci = b / (p.k + kEdiRsP), q = b % (p.k + kEdiRsP);
          v = b >= p.B ? 0 : q < p.k ? pk[ci * p.k + q] : par[ci * kEdiRsP + q - p.k];
        }
        o[hb + j] = v;
      }
      CHECK(std::fwrite(o, 1, static_cast<size_t>(n), out) == static_cast<size_t>(n));
      delete[] o;
      total += n;
      ++packets;
    }
    CHECK(total == edi_out_bytes(p, mode, h.l));
    delete[] par;
    delete[] pk;
    delete[] f;
    seq = (seq + 1) & 0xFFFF;
  }
  std::fclose(out);
  return packets;
}
}  // namespace

int main(int argc, char** argv)
{
  if (argc == 7) {
    const long n = host_stage(argv[1], std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), argv[6]);
    std::printf("ok edi-units\nstage: %ld packets\n", n);
    return 0;
  }
  int max_f = 0, max_cover = 0;
  const long sizes = size_rule(&max_f, &max_cover);
  const long splits = crc_rule();
  rs_rule();
  std::printf("ok edi-units\nsizes: %ld combinations, most fragments of a frame %d, widest cover %d; crc: %ld splits\n", sizes, max_f, max_cover, splits);
  return 0;
}
