// edi2eti.cpp — EDI packets in, ETI(NI) frames out:
//   dab2eti-hip capture.cu8 | eti2edi --fec 2 | edi2eti [--depth N] [in.edi | -] > out.eti
// Reads the packets concatenated as eti2edi writes them and finds their ends by their own length fields: "AF" with LEN + 12, "PF" with a right
// HCRC and 14 or 16 + PLEN.  At a place that is neither it moves on byte by byte to the next that is, and counts the bytes skipped.  PFT
// reassembly, RS(255,207) erasure recovery, the CRCs and the rebuild of the frames run on the GPU (dabhip_edirx_*).  Whatever whole packets
// are on hand after each read are pushed at once, so a live pipe keeps its latency; the open groups are flushed at the end of input.  Stdout
// is the frames; the counters go to stderr as one line at the end.
#include <fcntl.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dabhip.h"
#include "edirx_plan.hpp"
#include "eti_stdin.hpp"

namespace {
bool number(const char* s, long lo, long hi, int* out)
{
  char* end = nullptr;
  const long v = std::strtol(s, &end, 10);
  if (!*s || *end || v < lo || v > hi) return false;
  *out = static_cast<int>(v);
  return true;
}

// The packet that begins at p with `have` bytes on hand: its length, 0 when more bytes are needed to tell, -1 when none begins here.
long packet_at(const uint8_t* p, size_t have, bool at_end)
{
  if (have < 2) return at_end ? -1 : 0;
  if (p[0] == 'A' && p[1] == 'F') {
    if (have < 10) return at_end ? -1 : 0;
    if ((p[8] & 0xF0) != 0x90 || p[9] != 'T') return -1;
    const long n = static_cast<long>(dabhip::edirx_get32(p + 2)) + 12;
    if (n > dabhip::kEdirxMaxPayload) return -1;       // no AF packet of a frame is that long: a chance "AF"
    return static_cast<size_t>(n) <= have ? n : at_end ? -1 : 0;
  }
  if (p[0] == 'P' && p[1] == 'F') {
    if (have < 12) return at_end ? -1 : 0;
    const unsigned word = dabhip::edirx_get16(p + 10);
    const size_t head = (word & 0x8000) ? 16 : 14;
    if (have < head) return at_end ? -1 : 0;
    if (dabhip::edi_crc16(p, static_cast<int64_t>(head) - 2) != dabhip::edirx_get16(p + head - 2)) return -1;
    const size_t n = head + (word & 0x3FFF);
    return n <= have ? static_cast<long>(n) : at_end ? -1 : 0;
  }
  return -1;
}
}  // namespace

int main(int argc, char** argv)
{
  int depth = 4, in = 0;
  bool bad = false;
  const char* path = nullptr;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    if (!std::strcmp(a, "--depth") && i + 1 < argc) bad |= !number(argv[++i], 1, 16, &depth);
    else if (!std::strcmp(a, "-")) path = nullptr;
    else if (a[0] == '-' || path) bad = true;
    else path = a;
  }
  if (bad) {
    std::fprintf(stderr, "Usage: edi2eti [--depth N] [in.edi | -]   (N = 1..16 packet sequence numbers kept open, default 4; EDI packets on stdin or from the "
                         "file, ETI frames on stdout)\n");
    return 1;
  }
  if (path && (in = open(path, O_RDONLY)) < 0) { std::fprintf(stderr, "edi2eti: cannot open %s\n", path); return 3; }
  dabhip_edirx* d = dabhip_edirx_create(0, 1, depth);
  if (!d) { std::fprintf(stderr, "edi2eti: %s\n", dabhip_last_error()); return 2; }
  std::vector<uint8_t> buf(1 << 20), out;
  std::vector<int32_t> lengths;
  size_t have = 0;
  long long skipped = 0, frames = 0;
  int rc = 0;
  const auto fetch = [&](int64_t n) {                  // the frames of the last push or flush to stdout
    if (n < 0) { std::fprintf(stderr, "edi2eti: %s\n", dabhip_last_error()); rc = 2; return false; }
    if (n == 0) return true;
    out.resize(static_cast<size_t>(n) * DABHIP_ETI_BYTES);
    if (dabhip_edirx_frames(d, 0, out.data(), static_cast<int64_t>(out.size())) != n) { std::fprintf(stderr, "edi2eti: %s\n", dabhip_last_error()); rc = 2; return false; }
    frames += n;
    if (!write_all(out.data(), out.size())) { rc = 3; return false; }
    return true;
  };
  for (bool at_end = false; !at_end && rc == 0;) {
    const ssize_t r = read(in, buf.data() + have, buf.size() - have);
    if (r < 0) { rc = 3; break; }
    have += static_cast<size_t>(r);
    at_end = r == 0;
    // the whole packets on hand, moved together to the front of the buffer; what is left behind them waits for more bytes
    size_t at = 0, packed = 0;
    lengths.clear();
    while (at < have) {
      const long n = packet_at(buf.data() + at, have - at, at_end);
      if (n == 0) break;
      if (n < 0) { ++at; ++skipped; continue; }
      std::memmove(buf.data() + packed, buf.data() + at, static_cast<size_t>(n));
      lengths.push_back(static_cast<int32_t>(n));
      packed += static_cast<size_t>(n);
      at += static_cast<size_t>(n);
    }
    const int64_t np = static_cast<int64_t>(lengths.size());
    if (np > 0 && !fetch(dabhip_edirx_push(d, buf.data(), lengths.data(), &np, 0))) break;
    std::memmove(buf.data(), buf.data() + at, have - at);
    have -= at;
  }
  if (rc == 0) fetch(dabhip_edirx_flush(d, 0));
  int64_t c[DABHIP_EDIRX_COUNTERS] = {0};
  dabhip_edirx_stats(d, 0, c, DABHIP_EDIRX_COUNTERS);
  std::fprintf(stderr, "edi2eti: %lld frames, %lld bytes skipped, %lld packets (%lld bad, %lld late, %lld duplicate, %lld mismatched, %lld missing), groups: %lld incomplete, "
                       "%lld RS failed, %lld CRC failed, %lld refused; %lld words and %lld bytes filled in, %lld items ignored, %lld with ATST\n",
               frames, skipped, (long long)c[0], (long long)c[1], (long long)c[2], (long long)c[3], (long long)c[4], (long long)c[5], (long long)c[6], (long long)c[7],
               (long long)c[8], (long long)c[9], (long long)c[10], (long long)c[11], (long long)c[12], (long long)c[13]);
  dabhip_edirx_destroy(d);
  if (path) close(in);
  return rc;
}
