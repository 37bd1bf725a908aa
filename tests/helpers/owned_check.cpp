// owned_check.cpp -- limg_amd/csrc/limg_hip_owned.h on a machine without a GPU: the HIP entry points the header calls are defined here on top of malloc / free, with a
// "fail the next calls" switch and live counts of their own.  Built with -fsanitize=address,undefined and run by tests/test_context_owned_cpu.py; no HIP runtime is
// linked.  Exit status 0: every check held (and LeakSanitizer found nothing on the way out).
#define LIMG_HIP_TEST_HOOKS 1 // the header's own live counts: they must agree with the fakes'
#include "../../limg_amd/csrc/limg_hip_owned.h"

#include <stdlib.h>
#include <type_traits>

namespace
{
  long liveDev = 0, liveHost = 0, liveStreams = 0, liveEvents = 0, created = 0;
  int skipCalls = 0, failCalls = 0; // the next `skipCalls` create calls succeed, the `failCalls` after them fail
  void fail_after(int skip, int fail) { skipCalls = skip; failCalls = fail; }
  bool refuse()
  {
    if (skipCalls > 0) { skipCalls--; return false; }
    if (failCalls > 0) { failCalls--; return true; }
    return false;
  }
  template <class T> hipError_t make(T *out, long &live, hipError_t error)
  {
    if (refuse()) return error;
    *out = (T)malloc(16);
    live++; created++;
    return hipSuccess;
  }
  template <class T> hipError_t drop(T p, long &live) { free((void *)p); live--; return hipSuccess; }

  int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "owned_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

  uint64_t hook(int what) { return limg_hip_live::count[what].load(); }
  // the fakes' counts, the header's counts under LIMG_HIP_TEST_HOOKS and the device-byte total all say the same
  void check_live(long dev, long host, long streams, long events, size_t bytes, const std::atomic<size_t> &total)
  {
    CHECK(liveDev == dev && liveHost == host && liveStreams == streams && liveEvents == events);
    CHECK(hook(limg_hip_live::kDevBufs) == (uint64_t)dev && hook(limg_hip_live::kHostBufs) == (uint64_t)host);
    CHECK(hook(limg_hip_live::kStreams) == (uint64_t)streams && hook(limg_hip_live::kEvents) == (uint64_t)events);
    CHECK(total.load() == bytes && hook(limg_hip_live::kDevBytes) == (uint64_t)bytes);
  }
}

extern "C"
{
  hipError_t hipMalloc(void **p, size_t) { return make(p, liveDev, hipErrorOutOfMemory); }
  hipError_t hipFree(void *p) { return drop(p, liveDev); }
  hipError_t hipHostMalloc(void **p, size_t, unsigned) { return make(p, liveHost, hipErrorOutOfMemory); }
  hipError_t hipHostFree(void *p) { return drop(p, liveHost); }
  hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return make(s, liveStreams, hipErrorInvalidValue); }
  hipError_t hipStreamDestroy(hipStream_t s) { return drop(s, liveStreams); }
  hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make(e, liveEvents, hipErrorInvalidValue); }
  hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
  hipError_t hipEventDestroy(hipEvent_t e) { return drop(e, liveEvents); }
  const char *hipGetErrorString(hipError_t) { return "refused by owned_check"; } // (HIP_TRY's message)
}

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_move_constructible<DevBuf>::value && !std::is_default_constructible<DevBuf>::value, "DevBuf");
static_assert(!std::is_copy_constructible<HostBuf>::value && !std::is_move_constructible<HostBuf>::value, "HostBuf");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_move_constructible<Stream>::value, "Stream");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_move_constructible<Event>::value, "Event");
static_assert(!std::is_copy_constructible<Events>::value && !std::is_move_constructible<Events>::value, "Events");
static_assert(!std::is_copy_assignable<DevBuf>::value && !std::is_copy_assignable<HostBuf>::value && !std::is_copy_assignable<Stream>::value &&
              !std::is_copy_assignable<Event>::value && !std::is_copy_assignable<Events>::value, "assignment");

int main()
{
  std::atomic<size_t> total{ 0 };
  { // a device buffer that grows twice: one live allocation, the total follows; a size it already holds: nothing happens
    DevBuf a(total), b(total);
    CHECK(a.ensure(100) == limg_hip_success && a.cap == 100 && a.p);
    CHECK(a.ensure(1000) == limg_hip_success && a.cap == 1000);
    CHECK(a.ensure(5000) == limg_hip_success && a.cap == 5000);
    const long before = created;
    CHECK(a.ensure(4000) == limg_hip_success && a.cap == 5000 && created == before);
    check_live(1, 0, 0, 0, 5000, total);
    CHECK(b.ensure(24) == limg_hip_success);
    check_live(2, 0, 0, 0, 5024, total);
    // a failing allocation: the old one is gone (free, then allocate), nothing is left, the total drops by the old capacity
    fail_after(0, 1);
    CHECK(a.ensure(6000) == limg_hip_error_MemoryAllocationFailure && a.p == nullptr && a.cap == 0);
    check_live(1, 0, 0, 0, 24, total);
    CHECK(a.ensure(10) == limg_hip_success && a.cap == 10); // and it can be used again
    b.release();
    CHECK(b.p == nullptr && b.cap == 0);
    check_live(1, 0, 0, 0, 10, total);
  }
  check_live(0, 0, 0, 0, 0, total);
  { // pinned memory: the same, with a quarter of slack and outside the device total
    HostBuf h;
    CHECK(h.ensure(100) == limg_hip_success && h.cap == 125);
    CHECK(h.ensure(125) == limg_hip_success && h.cap == 125);
    CHECK(h.ensure(1000) == limg_hip_success && h.cap == 1250);
    check_live(0, 1, 0, 0, 0, total);
    fail_after(0, 1);
    CHECK(h.ensure(2000) == limg_hip_error_MemoryAllocationFailure && h.p == nullptr && h.cap == 0);
    check_live(0, 0, 0, 0, 0, total);
    CHECK(h.ensure(8) == limg_hip_success && h.cap == 10);
  }
  check_live(0, 0, 0, 0, 0, total);
  { // a stream: nothing until the first get(), one stream however often it is asked for; a failed creation is reported and tried again by the next get()
    Stream s;
    CHECK((hipStream_t)s == nullptr);
    check_live(0, 0, 0, 0, 0, total);
    hipStream_t x = nullptr, y = nullptr;
    fail_after(0, 1);
    CHECK(s.get(x) == limg_hip_error_Generic && (hipStream_t)s == nullptr);
    CHECK(s.get(x) == limg_hip_success && x != nullptr && s.get(y) == limg_hip_success && x == y && (hipStream_t)s == x);
    check_live(0, 0, 1, 0, 0, total);
  }
  check_live(0, 0, 0, 0, 0, total);
  { // a list of events: grows, never shrinks; when creation number k fails the k - 1 before it stay (and go with the list)
    Events ev;
    CHECK(ev.ensure(3, hipEventDisableTiming) == limg_hip_success && ev.size() == 3 && ev[0] && ev[2] && ev.data()[1] == ev[1]);
    CHECK(ev.ensure(2, hipEventDisableTiming) == limg_hip_success && ev.size() == 3);
    const hipEvent_t first = ev[0];
    fail_after(3, 1); // of the 5 missing ones the 4th fails
    CHECK(ev.ensure(8, hipEventDefault) == limg_hip_error_Generic && ev.size() == 6 && ev[0] == first);
    check_live(0, 0, 0, 6, 0, total);
    CHECK(ev.ensure(8, hipEventDefault) == limg_hip_success && ev.size() == 8);
    Event one;
    CHECK((hipEvent_t)one == nullptr);
    fail_after(0, 1);
    CHECK(one.ensure(hipEventDisableTiming) == limg_hip_error_Generic && (hipEvent_t)one == nullptr);
    CHECK(one.ensure(hipEventDisableTiming) == limg_hip_success && (hipEvent_t)one != nullptr);
    const hipEvent_t e = one;
    CHECK(one.ensure(hipEventDisableTiming) == limg_hip_success && (hipEvent_t)one == e);
    check_live(0, 0, 0, 9, 0, total);
  }
  check_live(0, 0, 0, 0, 0, total);
  { // members of a struct, as a context holds them: nothing is written for their release
    struct Slot { HostBuf host; DevBuf dev; Event done; Slot(std::atomic<size_t> &n) : dev(n) {} };
    struct { Slot slots[2]; Stream s; Events ev; } group{ { total, total } };
    hipStream_t s;
    CHECK(group.slots[1].host.ensure(64) == limg_hip_success && group.slots[1].dev.ensure(64) == limg_hip_success && group.slots[0].dev.ensure(1) == limg_hip_success);
    CHECK(group.slots[1].done.ensure(hipEventDisableTiming) == limg_hip_success && group.s.get(s) == limg_hip_success && group.ev.ensure(2, hipEventDefault) == limg_hip_success);
    check_live(2, 1, 1, 3, 65, total);
  }
  check_live(0, 0, 0, 0, 0, total);
  if (failures) fprintf(stderr, "owned_check: %d check(s) failed\n", failures);
  else printf("owned_check ok: %ld resources created and released\n", created);
  return failures ? 1 : 0;
}
