// session_windows.hpp — the device windows of a streaming session (session.cpp applies it): per stream and segment, how much of the stream's past is
// kept, where it lands in front of the new segment, when a window must grow, and where the stream's byte 0 would lie.  Host-only, no GPU call
// (tests/host_sanitize replays a session on byte arrays sized exactly as planned: a wrong offset there is an overrun under ASan, here it would be an
// out-of-bounds device read).
//
// Segment k of a stream is uploaded to window k % 3 at offset `reserve`; the bytes of earlier segments the front end may still read are then copied
// in front of it from window (k - 1) % 3, so that the window holds the stream's bytes [need, avail) in one piece.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace dabhip {

// what a session knows of one stream between two feeds
struct WindowBook {
  int64_t base = 0, avail = 0;     // first stream byte still held, bytes received (fed) so far
  size_t org = 0;                  // offset, in the newest fed window, of stream byte `base`
};

// oldest byte a later segment may still read (need_from: Engine::stream_need_from): everything below may go
inline int64_t window_need_from(bool first, int64_t need_from, int64_t avail) { return first ? 0 : std::min(need_from, avail); }
// what a window is reserved with before a segment of nbytes is uploaded to it at offset `reserve`
inline size_t window_bytes(size_t reserve, size_t nbytes) { return reserve + std::max<size_t>(nbytes, 16); }
// the gather kernels' descriptors (CopyDesc) carry 32-bit sizes: a longer segment goes by copy commands, a longer history is refused
inline bool gather_fits(size_t nbytes) { return nbytes < (size_t(1) << 32); }

struct WindowPlan {
  const char* refused = nullptr;   // why this feed cannot be made (the other fields are not to be used then)
  int64_t need = 0;                // first stream byte the window will hold
  size_t kept = 0;                 // bytes [need, avail) of the stream's past that move in front of the segment
  bool grow = false;               // more history than the reserve holds: the segment moves to a window of grow_bytes first (from `reserve` to `at`)
  size_t grow_bytes = 0;
  size_t at = 0;                   // where the segment starts in the (grown) window
  size_t move_from = 0, move_to = 0;   // the history: `kept` bytes from offset move_from of the previous window to offset move_to of this one
  int64_t virtual_base = 0;        // stream byte x lives at window + virtual_base + x (negative once `need` has passed the history's offset)
  WindowBook book;                 // the stream's book once the feed is through
};

inline WindowPlan plan_window(const WindowBook& b, bool first, int64_t need_from, size_t nbytes, size_t reserve)
{
  WindowPlan p;
  p.need = window_need_from(first, need_from, b.avail);
  p.kept = static_cast<size_t>(b.avail - p.need);
  if (!gather_fits(p.kept)) { p.refused = "stream_feed: more than 4 GiB of a stream's past still referenced"; return p; }
  p.grow = p.kept > reserve;       // (not seen in practice)
  p.grow_bytes = p.grow ? p.kept + std::max<size_t>(nbytes, 16) : 0;
  p.at = p.grow ? p.kept : reserve;
  p.move_from = b.org + static_cast<size_t>(p.need - b.base);      // stream byte x of the bytes still held lives at org + (x - base)
  p.move_to = p.at - p.kept;
  p.virtual_base = static_cast<int64_t>(p.move_to) - p.need;
  p.book.org = p.move_to;
  p.book.base = p.need;
  p.book.avail = b.avail + static_cast<int64_t>(nbytes);
  return p;
}

}  // namespace dabhip
