// ingest.hpp — what ingest.cpp (the host object) and k_ingest.hip (its kernels) share.  The arithmetic: include/dabhip.h; the host rule: ingest_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dabhip {

// One stream of one push.  Its input samples live in two places: [carry_from, new_from) in `carry` (what the push before kept), [new_from, end) in
// `src` (this push's samples, where the caller or the upload put them).  Positions are absolute sample indices of the stream.
struct IngestDesc {
  const void* carry;
  const void* src;
  uint8_t* out;          // this push's cu8: output first_out at out[0]
  void* keep;            // the carry of the next push: samples [keep_from, end)
  int64_t carry_from, new_from, end;
  int64_t first_out;
  int64_t keep_from;
  int32_t nout;
  uint32_t gain;
  int32_t energy_slot;   // >= 0: the gain window closes in this push, the energy of samples [0, W) goes to energy[energy_slot]
  int32_t pad;
};

// the table as the kernel wants it: L rows of T/2 + 1 words, pair j of row p = (taps[p][T-1-2j], taps[p][T-2-2j]) (low half first), last word 0
hipError_t launch_ingest_resample(int format, const IngestDesc* descs, int nstreams, int max_nout, const uint32_t* table, int L, int M, int T, hipStream_t stream);
hipError_t launch_ingest_energy(int format, const IngestDesc* descs, int nstreams, unsigned long long* energy, hipStream_t stream);
hipError_t launch_ingest_keep(int format, const IngestDesc* descs, int nstreams, int64_t max_keep, hipStream_t stream);

}  // namespace dabhip
