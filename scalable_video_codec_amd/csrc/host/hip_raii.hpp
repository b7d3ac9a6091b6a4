// hip_raii.hpp -- what every host driver (clip_encoder.cpp, stream_encoder.cpp, stream_decoder.cpp) needs of the HIP runtime,
// once: the two error helpers, device and pinned buffers, and move-only owners of a stream and an event.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "svc_hip.h"

// Hidden: libsvc_motion.so exports the drivers, not their plumbing.
namespace svc {
namespace host __attribute__((visibility("hidden"))) {

// The driver a failure is reported for: Who{"svc::StreamDecoder"}.Hip(e, "hipMalloc") throws "svc::StreamDecoder: hipMalloc: <HIP's text>".
struct Who {
  const char* name;
  void Hip(hipError_t e, const char* what) const {
    if (e != hipSuccess) throw std::runtime_error(std::string(name) + ": " + what + ": " + hipGetErrorString(e));
  }
  void Abi(int rc, const char* what) const {
    if (rc) throw std::runtime_error(std::string(name) + ": " + what + ": " + svc_hip_last_error());
  }
  // an event that has not completed yet is "not ready"; any other status is an error of an earlier launch and is reported HERE, where it
  // is first seen, not swallowed as "no news yet"
  bool Ready(hipEvent_t e) const {
    const hipError_t q = hipEventQuery(e);
    if (q == hipErrorNotReady) return false;
    Hip(q, "hipEventQuery");
    return true;
  }
};

// n elements of device memory or (kPinned) of pinned host memory; at least one is allocated, so p is never null after Alloc
template <typename T, bool kPinned> struct HipBuf {
  T* p = nullptr;
  size_t n = 0;
  HipBuf() = default;
  HipBuf(const HipBuf&) = delete;
  HipBuf& operator=(const HipBuf&) = delete;
  ~HipBuf() { Free(); }
  void Alloc(const Who& who, size_t count) { who.Hip(Malloc(count), kPinned ? "hipHostMalloc" : "hipMalloc"); }
  bool TryAlloc(size_t count) {  // false, with HIP's error cleared (it is not sticky), where the memory is not there
    if (Malloc(count) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
  }
  void Free() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; n = 0;
  }
  uint64_t bytes() const { return (uint64_t)n * sizeof(T); }

 private:
  hipError_t Malloc(size_t count) {  // what the buffer held is freed first
    Free();
    const size_t size = std::max<size_t>(count, 1) * sizeof(T);
    void** q = reinterpret_cast<void**>(&p);
    const hipError_t e = kPinned ? hipHostMalloc(q, size, hipHostMallocDefault) : hipMalloc(q, size);
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
};
template <typename T> struct DevBuf : HipBuf<T, false> {};
template <typename T> struct PinBuf : HipBuf<T, true> {};

// A non-blocking stream.  Its destructor synchronises before it destroys: an owner that declares its streams AFTER its buffers and
// events lets go of those only once nothing on the device uses them.
class Stream {
 public:
  Stream() = default;
  explicit Stream(const Who& who) { who.Hip(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking), "hipStreamCreate"); }
  Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept { std::swap(s_, o.s_); return *this; }
  ~Stream() {
    if (s_) { (void)hipStreamSynchronize(s_); (void)hipStreamDestroy(s_); }
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

// An event: for ordering only (hipEventDisableTiming), or one hipEventElapsedTime accepts.
class Event {
 public:
  Event() = default;
  explicit Event(const Who& who, bool timing = false) {
    who.Hip(timing ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, hipEventDisableTiming), "hipEventCreate");
  }
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace host
}  // namespace svc
