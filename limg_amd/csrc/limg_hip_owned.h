// limg_hip_owned.h -- what a context holds on the GPU, as types that release what they own: device buffers, pinned host buffers, lazily created streams and events.
// A member of one of these types is written down once, where it is declared: nothing else has to list it for it to be freed or counted.  None can be copied or moved.
// Needs the HIP runtime API, the C ABI's result codes and the standard library only: a host compiler builds it on its own (tests/helpers/owned_check.cpp).
#ifndef LIMG_HIP_OWNED_H
#define LIMG_HIP_OWNED_H

#include <hip/hip_runtime_api.h>
#include "../../include/limg_hip.h"

#include <atomic>
#include <stdio.h>
#include <vector>

#define HIP_TRY(expr)                                                                                                     \
  do                                                                                                                      \
  {                                                                                                                       \
    const hipError_t e_ = (expr);                                                                                         \
    if (e_ != hipSuccess)                                                                                                 \
    {                                                                                                                     \
      fprintf(stderr, "limg_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__);            \
      return limg_hip_error_Generic;                                                                                      \
    }                                                                                                                     \
  } while (0)

#ifdef LIMG_HIP_TEST_HOOKS
// liblimg_hip_test.so only: what is alive in the whole process, counted where a create call succeeded and where a destroy call is made (limg_hip_test_live_resources)
namespace limg_hip_live { enum { kDevBufs, kDevBytes, kHostBufs, kStreams, kEvents, kCounts }; inline std::atomic<uint64_t> count[kCounts]; }
#define LIMG_HIP_LIVE(what, n) (void)(limg_hip_live::count[limg_hip_live::what] += (uint64_t)(n))
#else
#define LIMG_HIP_LIVE(what, n) ((void)0)
#endif

struct Owned { Owned() = default; Owned(const Owned &) = delete; Owned &operator=(const Owned &) = delete; };

// device memory; `deviceBytes` is the owner's running total (limg_hip_context_device_bytes): always the sum of the `cap`s counted into it.  Atomic, relaxed: the
// merged-block encoder's worker thread and its calling thread both hold the context.
struct DevBuf : Owned
{
  void *p = nullptr;
  size_t cap = 0;
  explicit DevBuf(std::atomic<size_t> &deviceBytes) : total(deviceBytes) {}
  ~DevBuf() { release(); }
  limg_hip_result ensure(size_t bytes)
  {
    if (bytes <= cap) return limg_hip_success;
    release();
    if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return limg_hip_error_MemoryAllocationFailure; }
    cap = bytes;
    total.fetch_add(bytes, std::memory_order_relaxed);
    LIMG_HIP_LIVE(kDevBufs, 1); LIMG_HIP_LIVE(kDevBytes, bytes);
    return limg_hip_success;
  }
  void release()
  {
    if (p) { (void)hipFree(p); LIMG_HIP_LIVE(kDevBufs, -1); LIMG_HIP_LIVE(kDevBytes, 0 - cap); }
    total.fetch_sub(cap, std::memory_order_relaxed);
    p = nullptr; cap = 0;
  }
private:
  std::atomic<size_t> &total;
};

// pinned host memory (staging of the host stages: no zero fill, full-rate PCIe copies); not counted in the device bytes
struct HostBuf : Owned
{
  void *p = nullptr;
  size_t cap = 0;
  ~HostBuf() { release(); }
  limg_hip_result ensure(size_t bytes)
  {
    if (bytes <= cap) return limg_hip_success;
    release();
    const size_t want = bytes + bytes / 4; // grow with slack: sizes depend on the image content
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { p = nullptr; return limg_hip_error_MemoryAllocationFailure; }
    cap = want;
    LIMG_HIP_LIVE(kHostBufs, 1);
    return limg_hip_success;
  }
  void release() { if (p) { (void)hipHostFree(p); LIMG_HIP_LIVE(kHostBufs, -1); } p = nullptr; cap = 0; }
};

// a non-blocking stream, created by the first get()
struct Stream : Owned
{
  ~Stream() { if (s) { (void)hipStreamDestroy(s); LIMG_HIP_LIVE(kStreams, -1); } }
  limg_hip_result get(hipStream_t &out)
  {
    if (!s) { HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); LIMG_HIP_LIVE(kStreams, 1); }
    out = s;
    return limg_hip_success;
  }
  operator hipStream_t() const { return s; }
private:
  hipStream_t s = nullptr;
};

// a list of events that only grows: ensure(n, flags) creates the ones up to n that are not there yet.  Nothing it does throws (no exception may cross the extern "C" boundary).
struct Events : Owned
{
  ~Events() { for (hipEvent_t e : v) { (void)hipEventDestroy(e); LIMG_HIP_LIVE(kEvents, -1); } }
  limg_hip_result ensure(size_t n, unsigned flags)
  {
    while (v.size() < n)
    {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, flags));
      LIMG_HIP_LIVE(kEvents, 1);
      try { v.push_back(e); }
      catch (...) { (void)hipEventDestroy(e); LIMG_HIP_LIVE(kEvents, -1); return limg_hip_error_MemoryAllocationFailure; }
    }
    return limg_hip_success;
  }
  hipEvent_t operator[](size_t i) const { return v[i]; }
  size_t size() const { return v.size(); }
  hipEvent_t *data() { return v.data(); }
private:
  std::vector<hipEvent_t> v;
};

// one event, created by the first ensure()
struct Event : Owned
{
  ~Event() { if (e) { (void)hipEventDestroy(e); LIMG_HIP_LIVE(kEvents, -1); } }
  limg_hip_result ensure(unsigned flags) { if (!e) { HIP_TRY(hipEventCreateWithFlags(&e, flags)); LIMG_HIP_LIVE(kEvents, 1); } return limg_hip_success; }
  operator hipEvent_t() const { return e; }
private:
  hipEvent_t e = nullptr;
};

#endif
