// engine_detail.hpp — what the engine's source files (engine*.cpp) share beside the class itself.  Private to them.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "engine.hpp"
#include "fifo_view.hpp"
#include "kernels.hpp"

namespace dabhip {

constexpr int kFicWords = kFicBits / 32;                  // 288
constexpr int kMscWords = kMscBits / 32;                  // 6912
constexpr int kCifWords = kCifBits / 32;                  // 1728 words per (logical) CIF row

inline StreamState initial_state()
{
  StreamState st;
  std::memset(&st, 0, sizeof st);
  fifo_reset(st);                                         // empty FIFO, calloc'ed frame buffer (fifo_view.hpp)
  return st;
}

inline float ms_since(std::chrono::steady_clock::time_point a) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - a).count(); }

// DABHIP_TRACE_HOST: a line on stderr (fmt: the mark's name, the milliseconds since t0)
inline void host_mark(const char* fmt, const char* what, std::chrono::steady_clock::time_point t0)
{
  static const bool trace_host = std::getenv("DABHIP_TRACE_HOST") != nullptr;
  if (trace_host) std::fprintf(stderr, fmt, what, ms_since(t0));
}

}  // namespace dabhip
