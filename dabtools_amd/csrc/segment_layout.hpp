// segment_layout.hpp — where the transmission frames of one decode() / one segment of a session go, and what a session carries from segment to segment.
//
// No GPU call and no HIP type in here (like worklist.hpp): pure integer arithmetic, run by the CPU suite under ThreadSanitizer / AddressSanitizer / UBSan
// (tests/host_sanitize).  It is the contract of every kernel of the OFDM stage, the carry-over copies, read_demapped_tf (engine_msc.cpp) and complete_deferred (engine_ofdm.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace dabhip {

constexpr int kRowLead = 15;                              // logical rows before a stream's CIF 0 (interleaver depth - 1)
constexpr int kCarrySlots = 4;                            // TF slots of a stream that a session's next segment still needs (with the rows kRowLead before them)
// time de-interleaver: bit plane r of a transmitted CIF lives this many logical rows before that CIF's own
constexpr int kPlaneRowsBack[16] = {0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15};

struct IntPair { int x, y; };                             // int2 without the HIP header: K1's {status, ordinal} per call, the frame list's {stream, call}

// One decode's frame layout.  Slots and logical CIF rows of a stream: first the ones carried over from the previous segment of a session (the last
// <= kCarrySlots TFs), then this segment's.  Stream b owns TF slots [tf_base[b], tf_base[b + 1]) and the rows from row_base[b] - kRowLead on; its CIF 0
// is row row_base[b], FIB block fib_base[b].  The frame list is stream-major within each of its two parts: [0, nmsc) the frames whose MSC symbols are
// demodulated, [nmsc, ntf) the deferred ones (lock-in skip: the first ndefer_of[b] new TFs of each stream).
struct SegmentLayout {
  std::vector<int> tf_base, row_base, fib_base, nnew, ndefer_of;
  int next_row = 0, ntf = 0, nmsc = 0;
};

// what a session carries between segments, per stream (a fresh decode starts from reset())
struct StreamCarry {
  int keep = 0, prev_used = 0;                            // slots the next segment carries over (the newest ones) out of the prev_used of the last layout
  int calls_done = 0, ord_done = 0;                       // calls scanned / TFs demodulated so far: K1 numbers calls and ordinals through the session
  int prev_tf_base = 0, prev_row_base = 0;                // the stream's place in the last layout
  int last_keep = 0;                                      // carried slots at the front of the last layout
  std::vector<uint8_t> msc_missing;                       // per slot of the last layout: its MSC rows were never written (deferred then, or when it was new)
  void reset() { *this = StreamCarry(); }
  // the segment laid out as `seg` has been decoded: what the next one starts from
  void advance(const SegmentLayout& seg, int stream)
  {
    const int nnew = seg.nnew[static_cast<size_t>(stream)];
    // carried slots keep their flag (a deferred TF of an earlier segment cannot be completed any more), this segment's deferred ones get theirs
    msc_missing.resize(static_cast<size_t>(prev_used), 0);
    msc_missing.erase(msc_missing.begin(), msc_missing.end() - keep);
    msc_missing.resize(static_cast<size_t>(keep + nnew), 0);
    std::fill(msc_missing.begin() + keep, msc_missing.begin() + keep + seg.ndefer_of[static_cast<size_t>(stream)], uint8_t(1));
    last_keep = keep;
    prev_used = keep + nnew;
    keep = std::min(kCarrySlots, prev_used);
    ord_done += nnew;
    prev_tf_base = seg.tf_base[static_cast<size_t>(stream)];
    prev_row_base = seg.row_base[static_cast<size_t>(stream)];
  }
};

// The layout of a segment from the scan's records: info[b * max_calls + k] = {status, ordinal} of call k of stream b (status 2: a TF was demodulated),
// ncalls[b] <= max_calls calls of stream b in this segment, defer_max[b] = leading new TFs of stream b that cannot be locked (at most; control_plane.hpp:
// lockin_deferred).  Fills `out` and, per frame of the list, frames[i] = {stream, call}, frame_slot[i], frame_row[i] (ntf <= streams x max_calls entries each).
// Slots and rows are what they would be without the skip; no reader of the list relies on its order (every kernel goes from the list entry to stream,
// call, slot and row; the guard's entries carry list indices of the launch that wrote them).
inline bool layout_segment(const IntPair* info, int max_calls, const int* ncalls, const std::vector<StreamCarry>& carry, const int* defer_max, SegmentLayout& out,
                           IntPair* frames, int* frame_slot, int* frame_row, std::string* error)
{
  const size_t nstreams = carry.size();
  out.tf_base.assign(nstreams + 1, 0);
  for (std::vector<int>* v : {&out.row_base, &out.fib_base, &out.nnew, &out.ndefer_of}) v->assign(nstreams, 0);
  out.next_row = out.ntf = 0;
  int ndefer = 0;
  for (size_t b = 0; b < nstreams; ++b) {
    int n = 0;
    for (int k = 0; k < ncalls[b]; ++k) n += info[b * max_calls + k].x == 2 ? 1 : 0;
    out.nnew[b] = n;
    out.ndefer_of[b] = std::max(0, std::min(defer_max[b], n));
    out.ntf += n;
    ndefer += out.ndefer_of[b];
  }
  out.nmsc = out.ntf - ndefer;
  int at_msc = 0, at_defer = out.nmsc;
  for (size_t b = 0; b < nstreams; ++b) {
    const int keep = carry[b].keep;
    out.row_base[b] = out.next_row + kRowLead;            // each stream gets 15 lead-in rows for the scatter of its first CIFs
    int seen = 0;
    for (int k = 0; k < ncalls[b]; ++k) {
      const IntPair d = info[b * max_calls + k];
      if (d.x != 2) continue;
      if (d.y - carry[b].ord_done != seen) {              // K1 numbers a stream's demodulated TFs densely: anything else would leave the stream's slots
        if (error) *error = "decode: the calls' ordinals do not number this segment's transmission frames";
        return false;
      }
      const int local = keep + seen, at = seen < out.ndefer_of[b] ? at_defer++ : at_msc++;
      ++seen;
      frames[at] = IntPair{static_cast<int>(b), k};
      frame_slot[at] = out.tf_base[b] + local;
      frame_row[at] = out.row_base[b] + 4 * local;
    }
    out.tf_base[b + 1] = out.tf_base[b] + keep + out.nnew[b];
    out.fib_base[b] = 4 * out.tf_base[b];
    out.next_row += kRowLead + 4 * (keep + out.nnew[b]);
  }
  return true;
}

}  // namespace dabhip
