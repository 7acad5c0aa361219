// scan_units.cpp — the block scan's host rule (csrc/scan_blocks.hpp) as a stand-alone program under -fsanitize=address,undefined
// (tests/test_scan_model.py builds and runs it).  The refusals; random pushes whose carry and input live in arrays of EXACTLY the planned sizes and
// are read the way the kernel's descriptors say (an index outside what the plan promised is an overrun the sanitizer reports), the segments' samples
// compared with the stream's own; and the detect rule on spectra of exactly 4096 bins with records of exactly `cap` entries: blocks made by hand,
// bins near 2^63 (the 128-bit products), all zeros, the raster's 38 names and the refusal of a 17th block.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../dabtools_amd/csrc/scan_blocks.hpp"

using namespace dabhip;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace {
// sample n out of (carry, src) as the descriptors place them
int32_t fetch(const ScanPush& p, const std::vector<int32_t>& carry, const std::vector<int32_t>& src, int64_t n)
{
  CHECK(n >= p.carry_from && n < p.end);
  return n < p.new_from ? carry.at(static_cast<size_t>(n - p.carry_from)) : src.at(static_cast<size_t>(n - p.new_from));
}

void pushes(std::mt19937_64& rng, int nsegments)
{
  const int64_t total = static_cast<int64_t>(nsegments) * kScanSize + 9000;
  std::vector<int32_t> stream(static_cast<size_t>(total));
  for (auto& v : stream) v = static_cast<int32_t>(rng());
  ScanStreamState st;
  std::vector<int32_t> carry;
  int64_t at = 0, seen = 0;
  const int64_t sizes[] = {0, 1, 4094, 1, 4097, 0, 4095, 8192};
  for (int k = 0; at < total; ++k) {
    const int64_t n = std::min<int64_t>(total - at, k < 8 ? sizes[k] : static_cast<int64_t>(rng() % 20000));
    const std::vector<int32_t> src(stream.begin() + at, stream.begin() + at + n);        // exactly this push's samples
    const ScanPush p = scan_plan_push(nsegments, st, n);
    CHECK(p.carry_from + static_cast<int64_t>(carry.size()) == p.new_from && p.new_from == at && p.end == at + n);
    CHECK(p.first_seg == seen && p.nseg >= 0 && p.keep >= 0 && p.keep < kScanSize && p.keep_from + p.keep == p.end);
    for (int64_t g = p.first_seg; g < p.first_seg + p.nseg; ++g)
      for (int i = 0; i < kScanSize; ++i) CHECK(fetch(p, carry, src, g * kScanSize + i) == stream[static_cast<size_t>(g * kScanSize + i)]);
    seen += p.nseg;
    CHECK(seen == std::min<int64_t>(nsegments, (at + n) / kScanSize));
    std::vector<int32_t> keep(static_cast<size_t>(p.keep));                               // exactly what is to be carried
    for (int64_t i = 0; i < p.keep; ++i) keep[static_cast<size_t>(i)] = fetch(p, carry, src, p.keep_from + i);
    if (seen == nsegments) CHECK(p.keep == 0);
    else CHECK(p.keep == (at + n) % kScanSize);
    carry.swap(keep);
    at += n;
  }
  CHECK(seen == nsegments);
}

struct Spectrum {
  std::unique_ptr<uint64_t[]> p{new uint64_t[kScanSize]};      // exactly 4096 bins
  explicit Spectrum(uint64_t floor_level) { for (int i = 0; i < kScanSize; ++i) p[i] = floor_level; }
  void set_shifted(int b, uint64_t v) { p[(b + kScanSize / 2) % kScanSize] = v; }
  // a block of 1.536 MHz centred f Hz from the capture's centre
  void block(int64_t rate, int64_t f, uint64_t level)
  {
    for (int b = 0; b < kScanSize; ++b) {
      const int64_t hz = static_cast<int64_t>(b - kScanSize / 2) * rate / kScanSize;
      if (hz >= f - 768000 && hz <= f + 768000) set_shifted(b, level);
    }
  }
};

int detect(const Spectrum& s, int64_t rate, int64_t center, int cap, std::vector<dabhip_scan_block>* out, std::string* why)
{
  std::unique_ptr<dabhip_scan_block[]> recs(cap ? new dabhip_scan_block[cap] : nullptr);      // exactly cap records
  const int n = scan_detect(s.p.get(), rate, center, recs.get(), cap, why);
  out->assign(recs.get(), recs.get() + (n < 0 ? 0 : std::min(n, cap)));
  return n;
}

void detections(std::mt19937_64& rng)
{
  std::vector<dabhip_scan_block> out;
  std::string why;
  for (const uint64_t unit : {uint64_t(1), uint64_t(1) << 40, uint64_t(1) << 56}) {      // 64 units near 2^62: sums of thousands of bins pass 2^64
    for (const int64_t rate : {int64_t(2048000), int64_t(4096000), int64_t(8000000), int64_t(10240000)}) {
      Spectrum s(unit);
      std::vector<int64_t> want;
      for (int64_t f = -rate / 2 + 900000 + static_cast<int64_t>(rng() % 50000); f + 900000 <= rate / 2; f += 1712000) {
        s.block(rate, f, unit * (16 + rng() % 48));
        want.push_back(f);
      }
      CHECK(detect(s, rate, 0, 16, &out, &why) == static_cast<int>(want.size()));
      for (size_t k = 0; k < want.size(); ++k) {
        CHECK(std::llabs(out[k].offset_hz - want[k]) <= 2 * rate / kScanSize + 1 && out[k].name[0] == 0);
        CHECK(out[k].width_hz >= kScanMinWidth && out[k].width_hz <= kScanMaxWidth && out[k].nin > 0 && out[k].ng > 0 && out[k].in > out[k].lo);
      }
      if (want.size() > 1) {                                       // fewer records than blocks: the count all the same, and no record written past cap
        CHECK(detect(s, rate, 0, 1, &out, &why) == static_cast<int>(want.size()) && out.size() == 1);
        CHECK(detect(s, rate, 0, 0, &out, &why) == static_cast<int>(want.size()));
      }
    }
  }
  Spectrum zero(0);
  CHECK(detect(zero, 4096000, 0, 16, &out, &why) == 0);
  Spectrum full(UINT64_MAX);
  CHECK(detect(full, 10240000, 0, 16, &out, &why) == 0);
  CHECK(detect(zero, 2047999, 0, 16, &out, &why) == -1 && why.find("outside") != std::string::npos);
  CHECK(detect(zero, 10240001, 0, 16, &out, &why) == -1 && detect(zero, 4096000, -1, 16, &out, &why) == -1);
  // the raster: a block at the centre of a 2.048 Msps capture, the capture's centre 10 kHz above each of the 38
  const ScanRaster r = scan_raster();
  Spectrum one(1);
  one.block(2048000, 0, 100);
  for (int k = 0; k < 38; ++k) {
    CHECK(detect(one, 2048000, r.hz[k] + 10000, 16, &out, &why) == 1);
    CHECK(out[0].offset_hz == -10000 && std::string(out[0].name) == r.name[k]);
    CHECK(detect(one, 2048000, r.hz[k] + 40000, 16, &out, &why) == 1 && out[0].name[0] == 0 && std::llabs(out[0].offset_hz) <= 1000);
  }
  // 17 detections in one block: the lower guard is a comb, so that every other centre bin is a candidate (ng = 201 is odd at 2.048 Msps: a window
  // holds 100 or 101 teeth, and 2 in-band units against a tooth of 1 put the threshold between the two)
  Spectrum comb(0);
  comb.block(2048000, 0, 2000);
  for (int b = 150; b < 450; b += 2) comb.set_shifted(b, 1000);
  CHECK(detect(comb, 2048000, 0, 16, &out, &why) == -1);
  CHECK(why.find("blocks found: more than 16") != std::string::npos && std::atoi(why.c_str()) > 16);
}
}  // namespace

int main()
{
  CHECK(scan_check(0, 2, 4096000, 64).find("nstreams") != std::string::npos && scan_check(65536, 2, 4096000, 64).find("nstreams") != std::string::npos);
  CHECK(scan_check(1, 4, 4096000, 64).find("unknown format") != std::string::npos && scan_check(1, -1, 4096000, 64).find("unknown format") != std::string::npos);
  CHECK(scan_check(1, 2, 2047999, 64).find("outside") != std::string::npos && scan_check(1, 2, 10240001, 64).find("outside") != std::string::npos);
  CHECK(scan_check(1, 2, 4096000, 0).find("nsegments") != std::string::npos && scan_check(1, 2, 4096000, 65537).find("nsegments") != std::string::npos);
  CHECK(scan_check(65535, 0, 2048000, 1).empty() && scan_check(1, 3, 10240000, 65536).empty());
  std::mt19937_64 rng(14);
  for (const int nsegments : {1, 2, 7, 64}) pushes(rng, nsegments);
  detections(rng);
  std::printf("ok scan-units\n");
  return 0;
}
