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
  uint32_t step;         // tuned mode: the NCO step of this output stream's channel (0 otherwise)
};

// the table as the kernel wants it: L rows of T/2 + 1 words, pair j of row p = (taps[p][T-1-2j], taps[p][T-2-2j]) (low half first), last word 0
hipError_t launch_ingest_resample(int format, const IngestDesc* descs, int nstreams, int max_nout, const uint32_t* table, int L, int M, int T, hipStream_t stream);
// the tuned mode: descs has one entry per output stream (nouts of them); nco: 4096 words (cos | sin << 16, int16 each).  energy != nullptr: the
// energy form -- sum(vI^2 + vQ^2) over outputs [0, W) of the descriptors with a slot is ADDED to energy[slot] (zero it first) and no byte is written
hipError_t launch_ingest_tune(int format, const IngestDesc* descs, int nouts, int max_nout, const uint32_t* table, const uint32_t* nco, unsigned long long* energy, int L, int M, int T,
                              hipStream_t stream);
hipError_t launch_ingest_energy(int format, const IngestDesc* descs, int nstreams, unsigned long long* energy, hipStream_t stream);
hipError_t launch_ingest_keep(int format, const IngestDesc* descs, int nstreams, int64_t max_keep, hipStream_t stream);

}  // namespace dabhip
