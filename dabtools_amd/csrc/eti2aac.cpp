// eti2aac.cpp — the DAB+ counterpart of eti2mpa: reads ETI(NI) frames from stdin and writes the AUs of one DAB+ sub-channel as ADTS on stdout
//   dab2eti-hip capture.cu8 | eti2aac N > audio.aac
// Superframe sync, RS(120,110) correction and the AU CRCs run on the GPU (dabhip_dabplus_*).  Whatever whole frames are on hand after each
// read are pushed at once, so a live pipe keeps its latency.  Only AUs whose CRC is good are written, each behind a 7-byte ADTS header (AAC LC,
// the sampling index of the AAC core rate, 1 or 2 channels); --raw writes the bare AUs instead.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dabhip.h"
#include "eti_stdin.hpp"

namespace {
// ADTS fixed + variable header, MPEG-4, no CRC: AAC LC, core sampling rate (dac_rate 48 / 32 kHz, halved with SBR), 1 or 2 channels
void adts_header(uint8_t* h, int au_len, const dabhip_dabplus_sf& r)
{
  static const int sfi[2][2] = {{5, 8}, {3, 6}};   // [dac_rate][sbr_flag]: 32 kHz, 16 kHz; 48 kHz, 24 kHz
  const int idx = sfi[r.dac_rate & 1][r.sbr_flag & 1], ch = r.aac_channel_mode ? 2 : 1, flen = au_len + 7;
  h[0] = 0xff;
  h[1] = 0xf1;
  h[2] = static_cast<uint8_t>((1 << 6) | (idx << 2) | (ch >> 2));
  h[3] = static_cast<uint8_t>(((ch & 3) << 6) | ((flen >> 11) & 3));
  h[4] = static_cast<uint8_t>((flen >> 3) & 0xff);
  h[5] = static_cast<uint8_t>(((flen & 7) << 5) | 0x1f);
  h[6] = 0xfc;
}
}  // namespace

int main(int argc, char** argv)
{
  bool raw = false;
  int want = -1;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--raw")) raw = true;
    else want = std::atoi(argv[i]);
  }
  if (want < 0 || want > 63) {
    std::fprintf(stderr, "Usage: eti2aac [--raw] N   (N = DAB+ sub-channel id; ETI on stdin, ADTS -- or bare AUs with --raw -- on stdout)\n");
    return 1;
  }
  const int32_t id = want;
  dabhip_dabplus* d = dabhip_dabplus_create(0, 1, &id, 1);
  if (!d) { std::fprintf(stderr, "eti2aac: %s\n", dabhip_last_error()); return 2; }
  std::vector<uint8_t> aus;
  std::vector<dabhip_dabplus_sf> recs;
  long frames = 0;
  const int rc = for_eti_frames(0, 3, [&](const uint8_t* f, int64_t n) {
    if (dabhip_dabplus_push(d, f, &n, 0) < 0) { std::fprintf(stderr, "eti2aac: %s\n", dabhip_last_error()); return 2; }
    frames += n;
    const int64_t nsf = dabhip_dabplus_superframes(d, 0, 0, nullptr, 0);
    recs.resize(static_cast<size_t>(nsf));
    const int64_t nb = dabhip_dabplus_au_bytes(d, 0, 0, nullptr, 0);
    aus.resize(static_cast<size_t>(nb));
    if (nsf < 0 || nb < 0 || dabhip_dabplus_superframes(d, 0, 0, recs.data(), nsf) != nsf || dabhip_dabplus_au_bytes(d, 0, 0, aus.data(), nb) != nb) {
      std::fprintf(stderr, "eti2aac: %s\n", dabhip_last_error());
      return 2;
    }
    size_t off = 0;
    bool good = true;
    for (const dabhip_dabplus_sf& s : recs) {
      if (!s.layout_ok) continue;
      for (int k = 0; k < s.num_aus && good; ++k) {
        if (!(s.crc_ok >> k & 1)) continue;
        const int len = s.au_len[k] - 2;
        uint8_t h[7];
        adts_header(h, len, s);
        good = (raw || write_all(h, 7)) && write_all(aus.data() + off, static_cast<size_t>(len));
        off += static_cast<size_t>(len);
      }
    }
    return good ? 0 : 3;
  });
  int64_t c[7] = {0};
  dabhip_dabplus_stats(d, 0, 0, c);
  std::fprintf(stderr, "eti2aac: %ld frames, sub-channel %d: %lld superframes, %lld fire-code fails, %lld RS corrected bytes, %lld RS failed codewords, "
               "%lld AUs, %lld AU CRC fails, %lld sync losses\n", frames, want, static_cast<long long>(c[0]), static_cast<long long>(c[1]),
               static_cast<long long>(c[2]), static_cast<long long>(c[3]), static_cast<long long>(c[4]), static_cast<long long>(c[5]),
               static_cast<long long>(c[6]));
  dabhip_dabplus_destroy(d);
  return rc;
}
