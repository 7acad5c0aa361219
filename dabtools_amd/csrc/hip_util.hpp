// hip_util.hpp — the small HIP helpers every host object shares: the blocking copy that keeps the runtime's books bounded, the grow-only device
// buffer and the event.  Included by engine.hpp and, without the engine's other headers, by the side stages (stage_frame.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

namespace dabhip {

void set_error(const std::string& msg);

// The HIP runtime keeps its records of a stream's finished commands until somebody synchronises THAT STREAM: an event or a blocking copy that waits
// for the command itself does not let them go (tools/hip_retained_commands.py, ROCm 7.2: 970 bytes of heap per hipMemcpy into pageable memory on the
// null stream, 2.0 KB per asynchronous copy + event record + event synchronise on a stream of its own, for ever; nothing with a stream synchronise
// now and then).  A receiver that runs for weeks makes millions of such calls, so every path that is called once per buffer, frame or segment and
// does not end in a stream synchronise anyway either goes through the helper below or synchronises its stream every kReapEvery uses (the ETI fetches,
// the sessions' prefetch stream): bounded books, and a wait that is free when the stream is idle.
constexpr uint32_t kReapEvery = 32;
inline bool reap_enabled()             // DABHIP_NO_REAP=1: the behaviour before (for tools/soak_cli.py's "before" column only)
{
  static const bool on = std::getenv("DABHIP_NO_REAP") == nullptr;
  return on;
}
inline hipError_t blocking_copy(void* dst, const void* src, size_t nbytes, hipMemcpyKind kind)      // hipMemcpy on the null stream
{
  static std::atomic<uint32_t> calls{0};
  const hipError_t e = hipMemcpy(dst, src, nbytes, kind);
  if (e == hipSuccess && calls.fetch_add(1, std::memory_order_relaxed) % kReapEvery == kReapEvery - 1 && reap_enabled()) (void)hipStreamSynchronize(nullptr);
  return e;
}

// grow-only device allocation; contents are NOT preserved on growth
template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }
  bool reserve(size_t n)
  {
    if (n <= cap_) return true;
    release();
    if (hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T)) != hipSuccess) {
      p_ = nullptr;
      set_error("hipMalloc of " + std::to_string(n * sizeof(T)) + " bytes failed");
      return false;
    }
    cap_ = n;
    return true;
  }
  void release()
  {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  bool upload(const T* src, size_t n, hipStream_t s)
  {
    if (!reserve(n ? n : 1)) return false;
    return n == 0 || hipMemcpyAsync(p_, src, n * sizeof(T), hipMemcpyHostToDevice, s) == hipSuccess;
  }
  template <class A>
  bool upload(const std::vector<T, A>& v, hipStream_t s) { return upload(v.data(), v.size(), s); }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// a HIP event, created on demand (with or without timing) and destroyed with its owner
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  hipError_t create(bool timing = true) { return timing ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, hipEventDisableTiming); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace dabhip
