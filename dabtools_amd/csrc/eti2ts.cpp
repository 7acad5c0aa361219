// eti2ts.cpp — the transport-stream counterpart of eti2pkt: reads ETI(NI) frames from stdin and writes the MPEG-2 TS packets of one stream-mode
// sub-channel (ETSI TS 102 427) on stdout
//   dab2eti-hip capture.cu8 | eti2ts N [--drop-failed] > out.ts
// Slot sync, the byte de-interleaver and RS(204,188) correction run on the GPU (dabhip_ts_*).  Whatever whole frames are on hand after each read
// are pushed at once, so a live pipe keeps its latency.  Every packet is written as its 188 bytes; one whose code word was beyond correction is
// written as received with the transport_error_indicator set (byte 1 |= 0x80), or left out with --drop-failed.  The eight counters go to stderr
// as one line at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dabhip.h"
#include "eti_stdin.hpp"

int main(int argc, char** argv)
{
  int want = -1;
  bool drop_failed = false, bad = false;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--drop-failed")) drop_failed = true;
    else if (argv[i][0] == '-') bad = true;
    else want = std::atoi(argv[i]);
  }
  if (bad || want < 0 || want > 63) {
    std::fprintf(stderr, "Usage: eti2ts N [--drop-failed]   (N = sub-channel id of an MPEG-2 TS sub-channel; ETI on stdin, 188-byte packets on stdout)\n");
    return 1;
  }
  const int32_t id = want;
  dabhip_ts* d = dabhip_ts_create(0, 1, &id, 1);
  if (!d) { std::fprintf(stderr, "eti2ts: %s\n", dabhip_last_error()); return 2; }
  constexpr int kPacket = 188;
  std::vector<uint8_t> data, out;
  std::vector<dabhip_ts_rec> recs;
  long frames = 0, written = 0;
  const int rc = for_eti_frames(0, 3, [&](const uint8_t* f, int64_t n) {
    const int64_t np = dabhip_ts_push(d, f, &n, 0);
    if (np < 0) { std::fprintf(stderr, "eti2ts: %s\n", dabhip_last_error()); return 2; }
    frames += n;
    recs.resize(static_cast<size_t>(np));
    data.resize(static_cast<size_t>(np) * kPacket);
    if (np > 0 && (dabhip_ts_records(d, 0, 0, recs.data(), np) != np || dabhip_ts_data(d, 0, 0, data.data(), np * kPacket) != np * kPacket)) {
      std::fprintf(stderr, "eti2ts: %s\n", dabhip_last_error());
      return 2;
    }
    out.clear();
    for (int64_t i = 0; i < np; ++i) {
      const bool failed = recs[static_cast<size_t>(i)].flags & DABHIP_TS_RS_FAILED;
      if (failed && drop_failed) continue;
      out.insert(out.end(), data.begin() + i * kPacket, data.begin() + (i + 1) * kPacket);
      if (failed) out[out.size() - kPacket + 1] |= 0x80;
      ++written;
    }
    return out.empty() || write_all(out.data(), out.size()) ? 0 : 3;
  });
  int64_t c[8] = {0};
  dabhip_ts_stats(d, 0, 0, c);
  std::fprintf(stderr, "eti2ts: %ld frames, sub-channel %d: %lld packets (%ld written), %lld from missed slots, %lld sync losses, %lld bytes skipped, "
               "%lld RS corrected bytes, %lld RS failed code words, %lld packets without 0x47, %lld null packets\n",
               frames, want, static_cast<long long>(c[0]), written, static_cast<long long>(c[1]), static_cast<long long>(c[2]), static_cast<long long>(c[3]),
               static_cast<long long>(c[4]), static_cast<long long>(c[5]), static_cast<long long>(c[6]), static_cast<long long>(c[7]));
  dabhip_ts_destroy(d);
  return rc;
}
