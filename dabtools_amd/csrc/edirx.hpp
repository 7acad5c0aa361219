// edirx.hpp — EDI in (AF packets and PFT fragments back to ETI frames): the device-side types of the kernels (k_edirx.hip) and their launchers,
// shared with the host object (edirx.cpp).  The rules are in edirx_plan.hpp (free of HIP); dabhip.h has them in words; tests/edirx_model.py
// restates them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dabhip.h"
#include "edirx_plan.hpp"

namespace dabhip {

// A group that a stream touched in this push (a packet joined it, or it left the window), at slot[s] + EdirxGroup::local, where slot[s] =
// (packets in front of stream s) + s depth: a stream touches at most depth + its packets groups, so the slots are fixed and no order is raced for.
struct EdirxMeta {
  EdirxGroup g;
  int32_t status;                           // 0: still open at the end of the push, 1: left ready (a candidate frame), 2: lost
  int32_t stream;
  int32_t cand;                             // status 1: its place among its stream's candidates of this push, in the order they left
  int32_t entry;                            // its place in EdirxStream::open, and so in the carry
};
static_assert(sizeof(EdirxMeta) == 96, "EdirxMeta layout");

// the packets of a push: stream after stream, first[s] the first packet of stream s, npk[s] its count; packet p is at data + off[p]
struct EdirxPush {
  const uint8_t* data;
  const int64_t* off;                       // npackets + 1
  const int32_t* first;
  const int32_t* npk;
  int nstreams, depth, npackets;
  int flush;                                // -2: none, -1: every stream, else that stream, after its packets
};

// a candidate frame, at its place among all candidates of the push (bases[2 s + 1] + EdirxMeta::cand)
struct EdirxCand {
  int32_t slot;                             // of its EdirxMeta
  int32_t work;                             // its group's bytes: work + this kEdirxStride
};

// what the frame kernel leaves per candidate
struct EdirxVerdict {
  int32_t status;                           // 0: a frame, 1: RS failed, 2: "AF", LEN or CRC failed, 3: refused by the TAG walk
  int32_t items_ignored, with_atst;
  int32_t words, erasures;
  int32_t fcth, fct, pad;
};

// parse: a thread per packet -> hdr[p].  window: a lane per stream walks its packets (edirx_window_step) and then flushes if asked: the
// stream's state and counters, meta, fin (the slots' local numbers of the candidates in order), joined[p] (the meta slot packet p joined, -1:
// dropped), sums[2 s] groups touched, sums[2 s + 1] candidates; then one workgroup: their exclusive prefix sums -> bases, the totals last.
hipError_t launch_edirx_parse(const EdirxPush& p, EdirxHdr* hdr, hipStream_t stream);
hipError_t launch_edirx_window(const EdirxPush& p, const EdirxHdr* hdr, EdirxStream* state, int64_t* counters, EdirxMeta* meta, int32_t* fin, int32_t* joined,
                               int64_t* sums, int64_t* bases, hipStream_t stream);
// gather: the carried bytes of the touched groups into the (cleared) work buffer, then a wave per packet scatters its payload to its place.
hipError_t launch_edirx_gather(const EdirxPush& p, int64_t ntouched, const EdirxHdr* hdr, const EdirxMeta* meta, const int32_t* joined, const int64_t* bases,
                               const uint8_t* carry, uint8_t* work, hipStream_t stream);
// rs: the candidates' places (cands), the erasures of every code word (ers[32 C + w]) and the list of the words that have any; then a wave per
// listed word fills its erasures in the work buffer; rsfail[C] = 1 when a filled word keeps a syndrome.
hipError_t launch_edirx_rs(const EdirxPush& p, int64_t ncand, const EdirxMeta* meta, const int32_t* fin, const int64_t* bases, const uint8_t* gf, EdirxCand* cands,
                           uint8_t* ers, int32_t* list, int32_t* nlist, int32_t* rsfail, uint8_t* work, hipStream_t stream);
// frame: a workgroup per candidate: the AF packet out of its group's bytes, "AF" / LEN / CRC, the TAG walk, the ETI frame -> candframes, verdict.
hipError_t launch_edirx_frame(int64_t ncand, const EdirxMeta* meta, const EdirxCand* cands, const uint8_t* ers, const int32_t* rsfail, const uint8_t* work,
                              uint8_t* candframes, EdirxVerdict* verdict, hipStream_t stream);
// emit: a lane per stream ranks its frames among its candidates (counters, records, nframes[s]); then a workgroup per frame copies it to its
// place: stream s has its frames at out + bases[2 s + 1] 6144 and its records at recs + bases[2 s + 1].
hipError_t launch_edirx_emit(const EdirxPush& p, int64_t ncand, const EdirxMeta* meta, const EdirxCand* cands, const EdirxVerdict* verdict, const int64_t* bases,
                             const uint8_t* candframes, int64_t* counters, int32_t* outmap, int32_t* nframes, dabhip_edirx_rec* recs, uint8_t* out, hipStream_t stream);
// carry: the groups still open keep their bytes: work -> carry + (s depth + entry) kEdirxStride.
hipError_t launch_edirx_carry(const EdirxPush& p, int64_t ntouched, const EdirxMeta* meta, const int64_t* bases, const uint8_t* work, uint8_t* carry, hipStream_t stream);

}  // namespace dabhip
