// eti2edi.cpp — ETI(NI) frames in, EDI packets out (ETSI TS 102 693 over TS 102 821):
//   dab2eti-hip capture.cu8 | eti2edi [--pft | --fec M] [--max-frag N] [--seq0 N] [in.eti | -] > out.edi
// Without an option every frame is written as one AF packet; --pft cuts each into PFT fragments of at most N bytes (default 1400); --fec M adds
// RS(255,207) and interleaves so that M lost fragments (0..5) of a packet can be recovered.  TAG packing, the CRCs, the Reed-Solomon encoder
// and the interleaver run on the GPU (dabhip_edi_*).  Whatever whole frames are on hand after each read are pushed at once, 64 at most, so a
// live pipe keeps its latency.  Stdout is the packets concatenated; the six counters go to stderr as one line at the end.
#include <fcntl.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dabhip.h"
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
}  // namespace

int main(int argc, char** argv)
{
  int mode = 0, recover = 0, max_frag = 1400, seq0 = 0, in = 0;
  bool bad = false, pft = false, fec = false;
  const char* path = nullptr;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    if (!std::strcmp(a, "--pft")) pft = true;
    else if (!std::strcmp(a, "--fec") && i + 1 < argc) { fec = true; bad |= !number(argv[++i], 0, 5, &recover); }
    else if (!std::strcmp(a, "--max-frag") && i + 1 < argc) bad |= !number(argv[++i], 64, 1472, &max_frag);
    else if (!std::strcmp(a, "--seq0") && i + 1 < argc) bad |= !number(argv[++i], 0, 65535, &seq0);
    else if (!std::strcmp(a, "-")) path = nullptr;
    else if (a[0] == '-' || path) bad = true;
    else path = a;
  }
  if (bad || (pft && fec)) {
    std::fprintf(stderr, "Usage: eti2edi [--pft | --fec M] [--max-frag N] [--seq0 N] [in.eti | -]   (M = 0..5 lost fragments to recover, N = 64..1472 bytes per "
                         "fragment, default 1400; ETI on stdin or from the file, EDI packets on stdout)\n");
    return 1;
  }
  mode = fec ? 2 : pft ? 1 : 0;
  if (path && (in = open(path, O_RDONLY)) < 0) { std::fprintf(stderr, "eti2edi: cannot open %s\n", path); return 3; }
  dabhip_edi* d = dabhip_edi_create(0, 1, mode, recover, max_frag, seq0);
  if (!d) { std::fprintf(stderr, "eti2edi: %s\n", dabhip_last_error()); return 2; }
  std::vector<uint8_t> out;
  long frames = 0;
  const auto failed = [] { std::fprintf(stderr, "eti2edi: %s\n", dabhip_last_error()); return 2; };
  const int rc = for_eti_frames(in, 3, [&](const uint8_t* f, int64_t n) {
    if (dabhip_edi_push(d, f, &n, 0) < 0) return failed();
    frames += n;
    const int64_t nb = dabhip_edi_data(d, 0, nullptr, 0);
    if (nb < 0) return failed();
    out.resize(static_cast<size_t>(nb));
    if (nb > 0 && dabhip_edi_data(d, 0, out.data(), nb) != nb) return failed();
    return nb > 0 && !write_all(out.data(), out.size()) ? 3 : 0;
  });
  int64_t c[6] = {0};
  dabhip_edi_stats(d, 0, c);
  std::fprintf(stderr, "eti2edi: %ld frames (%lld skipped, %lld without FIC), %lld packets, %lld bytes, %lld RS chunks encoded\n", frames,
               static_cast<long long>(c[1]), static_cast<long long>(c[2]), static_cast<long long>(c[3]), static_cast<long long>(c[4]), static_cast<long long>(c[5]));
  dabhip_edi_destroy(d);
  if (path) close(in);
  return rc;
}
