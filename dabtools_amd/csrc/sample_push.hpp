// sample_push.hpp — the front of dabhip_ingest_push and dabhip_scan_push: what a push of raw samples is refused for, and where the host path
// puts each stream in the staging buffer.  Host-only, no GPU call (tests/host_sanitize/push_units.cpp runs it).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace dabhip {

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct SamplePush {
  std::string refusal;                             // "" = taken
  std::vector<int64_t> nsamples;                   // per stream
  std::vector<size_t> upload, offset;              // the host path: bytes of stream b that are uploaded, and where in the staging buffer (16-byte steps)
  size_t stage_total = 0;
};

// who: the entry's name, in front of a refusal.  upload_samples(b, n): how many of stream b's n samples the host path uploads.
template <class UploadSamples>
SamplePush plan_sample_push(const char* who, size_t sample_bytes, const void* const* src, const size_t* nbytes, bool on_device, int nstreams, UploadSamples upload_samples)
{
  SamplePush p;
  const size_t ns = static_cast<size_t>(nstreams), sb = sample_bytes;
  p.nsamples.assign(ns, 0);
  p.upload.assign(ns, 0);
  p.offset.assign(ns, 0);
  for (size_t b = 0; b < ns && p.refusal.empty(); ++b) {
    if (nbytes[b] % sb) p.refusal = std::string(who) + ": stream " + std::to_string(b) + ": " + std::to_string(nbytes[b]) + " bytes are no whole number of " + std::to_string(sb) + "-byte samples";
    else if (nbytes[b] && !src[b]) p.refusal = std::string(who) + ": null input";
    else if (on_device && nbytes[b] && reinterpret_cast<uintptr_t>(src[b]) % sb) p.refusal = std::string(who) + ": a device input must be aligned to its sample size";
    p.nsamples[b] = static_cast<int64_t>(nbytes[b] / sb);
    if (on_device) continue;
    p.upload[b] = static_cast<size_t>(upload_samples(static_cast<int>(b), p.nsamples[b])) * sb;
    p.offset[b] = p.stage_total;
    p.stage_total += round_up(p.upload[b], 16);
  }
  return p;
}

}  // namespace dabhip
