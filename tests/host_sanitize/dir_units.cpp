// dir_units.cpp — the ensemble directory's rule header (dabtools_amd/csrc/dir_figs.hpp) run on the host under ASan + UBSan by
// tests/test_dir_model.py: a stand-alone program, no HIP, no library.
//   dir_units FILE     FILE = n x 32 bytes, FIBs
// Every FIB is copied into a heap buffer of exactly 32 bytes of its own, so a read past byte 31 is caught; its facts go to a heap array of
// exactly kDirFactSlots.  Per FIB the program folds (CRC ok, figs, truncated, ignored, facts; per fact: kind, P/D, key, the payload's
// dir_fact_len bytes) into an FNV-1a hash and prints one line per 1000 FIBs and the total, which the Python side compares with the
// model's.  It also holds dir_uep_row and dir_eep_multiple to dab_tables.hpp, and checks that a walk leaves the bytes past a payload's length zero.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../dabtools_amd/csrc/dab_tables.hpp"
#include "../../dabtools_amd/csrc/dir_figs.hpp"

using namespace dabhip;

namespace {
uint64_t h = 1469598103934665603ull;
void fold(unsigned b) { h = (h ^ (b & 0xff)) * 1099511628211ull; }
}  // namespace

int main(int argc, char** argv)
{
  if (argc != 2) { std::fprintf(stderr, "usage: dir_units FILE\n"); return 2; }
  for (int i = 0; i < 64; ++i) {
    int rate, size, level;
    dir_uep_row(i, &rate, &size, &level);
    const UepProfile& u = uep_table()[i];
    if (rate != u.bitrate || size != u.size_cu || level != u.protlevel) { std::printf("FAIL uep row %d\n", i); return 1; }
  }
  for (int p = 0; p < 8; ++p)
    if (dir_eep_multiple(p) != eep_size_multiple(p)) { std::printf("FAIL eep multiple %d\n", p); return 1; }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) { std::fprintf(stderr, "dir_units: cannot open %s\n", argv[1]); return 2; }
  std::vector<uint8_t> in(kDirFibBytes);
  long n = 0;
  while (std::fread(in.data(), 1, kDirFibBytes, fp) == static_cast<size_t>(kDirFibBytes)) {
    std::unique_ptr<uint8_t[]> fib(new uint8_t[kDirFibBytes]);
    std::memcpy(fib.get(), in.data(), kDirFibBytes);
    std::unique_ptr<DirFact[]> facts(new DirFact[kDirFactSlots]);
    const bool ok = dir_fib_crc_ok(fib.get());
    DirFibStat st = {0, 0, 0, 0};
    if (ok) st = dir_walk_fib(fib.get(), facts.get());
    if (st.nfacts > 28) { std::printf("FAIL FIB %ld gives %d facts\n", n, st.nfacts); return 1; }
    fold(ok); fold(st.figs); fold(st.truncated); fold(st.ignored); fold(st.nfacts);
    for (int i = 0; i < st.nfacts; ++i) {
      const DirFact& f = facts[i];
      const int len = dir_fact_len(f.kind);
      if (len <= 0) { std::printf("FAIL FIB %ld fact %d has kind %d\n", n, i, f.kind); return 1; }
      for (int k = len; k < kDirPayload; ++k)
        if (f.payload[k]) { std::printf("FAIL FIB %ld fact %d: byte %d past its payload is set\n", n, i, k); return 1; }
      fold(f.kind); fold(f.pd);
      for (int k = 0; k < 4; ++k) fold(f.key >> (8 * k));
      for (int k = 0; k < len; ++k) fold(f.payload[k]);
    }
    ++n;
    if (n % 1000 == 0) std::printf("%ld %016llx\n", n, static_cast<unsigned long long>(h));
  }
  std::fclose(fp);
  std::printf("total %ld %016llx\n", n, static_cast<unsigned long long>(h));
  return 0;
}
