// edi.hpp — EDI out of ETI (ETSI TS 102 693 over TS 102 821): the device-side types of the kernels (k_edi.hip) and their launchers, shared with
// the host object (edi.cpp).  The rules are in edi_plan.hpp (free of HIP); dabhip.h has them in words; tests/edi_model.py restates them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dabhip.h"
#include "edi_plan.hpp"
#include "eti_push.hpp"

namespace dabhip {

// how the handle was created
struct EdiConfig {
  int32_t mode, recover, max_frag, seq0;
};

// per stream, carried from push to push
struct EdiState {
  int64_t frames;                           // frames since creation, skipped ones included: the next frame's number
  int32_t started;                          // an accepted frame has been seen since creation or reset
  int32_t last_fct;                         // of the latest accepted frame
  int32_t fcth;                             // of the latest accepted frame
  int32_t seq_next;
};
static_assert(sizeof(EdiState) == 24, "EdiState layout");

// one frame of the push, at its place among all frames of the push (base[s] + v)
struct EdiFrame {
  int32_t valid;                            // plan
  int32_t l;
  EdiPlan p;
  int32_t stream;
  int32_t fcth, seq;                        // scan
  int32_t pkt_local;                        // its first packet among its stream's packets of this push
  int64_t byte_local;                       // its first byte among its stream's bytes of this push
  int64_t number;                           // since creation
};
static_assert(sizeof(EdiFrame) == 64, "EdiFrame layout");

enum EdiCounter : int { kEdiCntFrames, kEdiCntSkipped, kEdiCntNoFic, kEdiCntPackets, kEdiCntBytes, kEdiCntChunks, kEdiCntN = 6 };

constexpr int kEdiScanWaves = 4;            // streams (waves) per workgroup of the scan kernel
constexpr int kEdiRsWaves = 4;              // waves per workgroup of the rs kernel, each on one frame at a time
constexpr int kEdiRsFrames = kEdiRsWaves;

// plan: a thread per (stream, new frame) -> EdiFrame.valid, l, p, stream.  scan: a wave per stream -> fcth, seq, pkt_local, byte_local, number,
// the stream's state and counters, its packets and bytes of this push (sums[2 s], sums[2 s + 1]); then one workgroup: exclusive prefix sums of
// those over the streams -> bases[2 s], bases[2 s + 1], the totals at s = nstreams.
hipError_t launch_edi_plan(const EtiFrames& fr, EdiConfig cfg, int nstreams, int maxv, EdiFrame* out, hipStream_t stream);
hipError_t launch_edi_scan(const EtiFrames& fr, EdiConfig cfg, int nstreams, EdiFrame* frames, EdiState* state, int64_t* counters, int64_t* sums, int64_t* bases,
                           hipStream_t stream);
// assemble: a workgroup per frame -> its AF packet at work + g kEdiWorkStride, zeros behind it.  rs: a lane per chunk -> parity + (32 g + chunk) 48.
// fragment: a workgroup per frame -> its packets at out + bases[2 s + 1] + byte_local and their records at recs + bases[2 s] + pkt_local.
hipError_t launch_edi_assemble(const EtiFrames& fr, int64_t nframes, const EdiFrame* frames, uint8_t* work, hipStream_t stream);
hipError_t launch_edi_rs(int64_t nframes, const EdiFrame* frames, const uint8_t* table, const uint8_t* work, uint8_t* parity, hipStream_t stream);
hipError_t launch_edi_fragment(EdiConfig cfg, int64_t nframes, const EdiFrame* frames, const int64_t* bases, const uint8_t* work, const uint8_t* parity, uint8_t* out,
                               dabhip_edi_rec* recs, hipStream_t stream);

}  // namespace dabhip
