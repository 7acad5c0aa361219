// eti_stdin.hpp — what the tools that read ETI(NI) frames from a pipe share (eti2aac, eti2pkt, eti2ts, eti2info, eti2edi): the read loop that hands
// on whatever whole frames are on hand after each read, so a live pipe keeps its latency, and the write to stdout (edi2eti's too).
#pragma once

#include <unistd.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dabhip.h"

inline bool write_all(const uint8_t* p, size_t n)
{
  size_t done = 0;
  while (done < n) {
    const ssize_t w = write(1, p + done, n - done);
    if (w <= 0) return false;
    done += static_cast<size_t>(w);
  }
  return true;
}

// Reads fd to its end through a buffer of 64 frames.  batch(frames, n) gets the n >= 1 whole frames on hand after a read and returns 0 to go
// on; what else it returns ends the loop and is returned, a negative value as 0 (a tool that has seen enough).  read_failed: returned when a
// read fails.  Bytes behind the last whole frame at the end of the input are dropped.
template <class Batch>
int for_eti_frames(int fd, int read_failed, Batch batch)
{
  std::vector<uint8_t> buf(64 * DABHIP_ETI_BYTES);
  size_t have = 0;
  for (;;) {
    const ssize_t r = read(fd, buf.data() + have, buf.size() - have);
    if (r < 0) return read_failed;
    have += static_cast<size_t>(r);
    const int64_t n = static_cast<int64_t>(have / DABHIP_ETI_BYTES);
    if (n > 0) {
      const int rc = batch(static_cast<const uint8_t*>(buf.data()), n);
      if (rc) return rc < 0 ? 0 : rc;
      have -= static_cast<size_t>(n) * DABHIP_ETI_BYTES;
      std::memmove(buf.data(), buf.data() + n * DABHIP_ETI_BYTES, have);
    }
    if (r == 0) return 0;
  }
}
