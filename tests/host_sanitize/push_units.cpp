// push_units.cpp — the front of dabhip_ingest_push and dabhip_scan_push (csrc/sample_push.hpp), the scan's upload clamp (csrc/scan_blocks.hpp) and
// the packed mixer table (csrc/ingest_plan.hpp) as a stand-alone program under -fsanitize=address,undefined (tests/test_scan_model.py builds and
// runs it).  src[] and nbytes[] are arrays of EXACTLY the stream count; the uploads are replayed as copies from buffers of exactly nbytes[b] into a
// staging buffer of exactly the planned total, so that an offset or a count beyond the plan is an overrun the sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../dabtools_amd/csrc/ingest_plan.hpp"
#include "../../dabtools_amd/csrc/sample_push.hpp"
#include "../../dabtools_amd/csrc/scan_blocks.hpp"

using namespace dabhip;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace {
const auto kAll = [](int, int64_t n) { return n; };              // ingest uploads every sample

// streams of 0, 1 and 4097 samples in every order: offsets in 16-byte steps, no overlap, every byte where the plan says
void staging(size_t sb)
{
  const size_t counts[3] = {0, 1, 4097};
  const int orders[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (const auto& order : orders) {
    std::vector<std::vector<uint8_t>> bytes(3);
    std::unique_ptr<const void*[]> src(new const void*[3]);
    std::unique_ptr<size_t[]> nbytes(new size_t[3]);
    for (int b = 0; b < 3; ++b) {
      bytes[b].assign(counts[order[b]] * sb, static_cast<uint8_t>(0x40 + b));
      src[b] = bytes[b].empty() ? nullptr : bytes[b].data();       // no bytes: no pointer is needed
      nbytes[b] = bytes[b].size();
      CHECK(nbytes[b] == 0 || nbytes[b] % 16 != 0);
    }
    for (const char* who : {"ingest_push", "scan_push"}) {
      const SamplePush p = plan_sample_push(who, sb, src.get(), nbytes.get(), false, 3, kAll);
      CHECK(p.refusal.empty() && p.nsamples.size() == 3 && p.upload.size() == 3 && p.offset.size() == 3);
      std::vector<uint8_t> stage(p.stage_total, 0);                // exactly the planned total
      size_t at = 0;
      for (size_t b = 0; b < 3; ++b) {
        CHECK(p.nsamples[b] == static_cast<int64_t>(counts[order[b]]) && p.upload[b] == nbytes[b]);
        CHECK(p.offset[b] % 16 == 0 && p.offset[b] == at);         // behind the stream before, rounded: no overlap
        at += (p.upload[b] + 15) / 16 * 16;
        if (p.upload[b]) std::memcpy(stage.data() + p.offset[b], src[b], p.upload[b]);
      }
      CHECK(at == p.stage_total && p.stage_total == (4097 * sb + 15) / 16 * 16 + 16);
      for (size_t b = 0; b < 3; ++b)
        for (size_t i = 0; i < p.upload[b]; ++i) CHECK(stage[p.offset[b] + i] == 0x40 + b);
    }
    // from device memory nothing is staged
    const SamplePush dev = plan_sample_push("ingest_push", sb, src.get(), nbytes.get(), true, 3, kAll);
    CHECK(dev.refusal.empty() && dev.stage_total == 0 && dev.upload == std::vector<size_t>(3, 0) && dev.nsamples[2] == static_cast<int64_t>(counts[order[2]]));
  }
}

void refusals(const std::string& who)
{
  alignas(16) static uint8_t buf[64];
  for (const size_t sb : {size_t(2), size_t(4), size_t(8)}) {
    const void* src[2] = {buf, buf};
    size_t nbytes[2] = {4 * sb, 3 * sb + 1};
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, false, 2, kAll).refusal ==
          who + ": stream 1: " + std::to_string(3 * sb + 1) + " bytes are no whole number of " + std::to_string(sb) + "-byte samples");
    nbytes[1] = 3 * sb;
    src[1] = nullptr;
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, false, 2, kAll).refusal == who + ": null input");
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, true, 2, kAll).refusal == who + ": null input");
    nbytes[1] = 0;                                                 // no bytes: no pointer is asked for
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, false, 2, kAll).refusal.empty());
    src[1] = buf + sb / 2;                                         // half a sample into it
    nbytes[1] = sb;
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, true, 2, kAll).refusal == who + ": a device input must be aligned to its sample size");
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, false, 2, kAll).refusal.empty());      // host memory may lie anywhere
    src[1] = buf + sb;
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, true, 2, kAll).refusal.empty());
    nbytes[1] = 0;                                                 // and the alignment of no bytes is nobody's business
    src[1] = buf + 1;
    CHECK(plan_sample_push(who.c_str(), sb, src, nbytes, true, 2, kAll).refusal.empty());
  }
}

// the scan's host path: a window of 2 segments, pushes that end before it, straddle its end and come after it
void scan_clamp()
{
  const int nseg = 2;
  const size_t sb = 4;
  const int64_t window = static_cast<int64_t>(nseg) * kScanSize;
  ScanStreamState st[2];
  const int64_t pushes[4][2] = {{4097, 0}, {4000, window}, {500, 1}, {7, 7}};       // stream 0 straddles in its third push, stream 1 fills the window at once
  const int64_t want[4][2] = {{4097, 0}, {4000, window}, {window - 8097, 0}, {0, 0}};
  for (int k = 0; k < 4; ++k) {
    std::vector<uint8_t> bytes[2];
    const void* src[2];
    size_t nbytes[2];
    for (int b = 0; b < 2; ++b) {
      bytes[b].assign(static_cast<size_t>(pushes[k][b]) * sb, 1);
      src[b] = bytes[b].data();
      nbytes[b] = bytes[b].size();
    }
    int calls = 0;
    const SamplePush p = plan_sample_push("scan_push", sb, src, nbytes, false, 2, [&](int b, int64_t n) { ++calls; return scan_upload_samples(nseg, st[b], n); });
    CHECK(p.refusal.empty() && calls == 2);                        // the clamp is computed once per stream
    std::vector<uint8_t> stage(p.stage_total);
    for (int b = 0; b < 2; ++b) {
      CHECK(p.nsamples[b] == pushes[k][b] && p.upload[b] == static_cast<size_t>(want[k][b]) * sb);
      if (p.upload[b]) std::memcpy(stage.data() + p.offset[b], src[b], p.upload[b]);
      const ScanPush plan = scan_plan_push(nseg, st[b], p.nsamples[b]);
      // what the kernels read of src lies within what was uploaded: the segments' samples and the samples kept
      const int64_t last = std::max(plan.nseg ? (plan.first_seg + plan.nseg) * kScanSize : 0, plan.keep ? plan.end : 0);
      CHECK(last <= plan.new_from + static_cast<int64_t>(p.upload[b] / sb));
    }
    if (k == 3) CHECK(p.stage_total == 0);
  }
  CHECK(st[0].done == nseg && st[1].done == nseg);
  ScanStreamState done;
  done.done = nseg;
  done.pushed = 5;                                                 // (no state of a real stream: `done` alone decides)
  CHECK(scan_upload_samples(nseg, done, 100) == 0 && scan_upload_samples(nseg, ScanStreamState{}, 100) == 100);
}
}  // namespace

int main()
{
  for (const size_t sb : {size_t(2), size_t(4), size_t(8)}) staging(sb);
  refusals("ingest_push");
  refusals("scan_push");
  scan_clamp();
  const std::vector<int16_t> cs = ingest_tune_nco();
  const std::vector<uint32_t> words = ingest_tune_nco_words();
  CHECK(words.size() == 4096 && cs.size() == 8192);
  for (size_t i = 0; i < 4096; ++i) CHECK(words[i] == (static_cast<uint16_t>(cs[2 * i]) | static_cast<uint32_t>(static_cast<uint16_t>(cs[2 * i + 1])) << 16));
  std::printf("ok push-units\n");
  return 0;
}
