// limg_hip_api.hip -- host side of liblimg_hip.so: context life cycle, options, device status, statistics, profiling, compare and synthesis entries of the C ABI
// (include/limg_hip.h).  The encode paths live in limg_hip_encode.hip (8x8 path), limg_hip_host_entry.hip (host pointers), limg_hip_stream_api.hip and
// limg_hip_stream_encode_api.hip (compact stream; version 1's encode family), limg_hip_blocked_api.hip (merged-block encoder) and limg_hip_multi.hip (RCCL); the noise table in limg_hip_noise_table.hip.
// Mirrors the reference's driver (src/limg.cpp:2175-2265 threshold/flag setup, :2105-2138 strip partition).
#include "limg_hip_context.h"

#include <math.h>

using namespace limg_hip;

namespace limg_hip
{
  void mark(limg_hip_context *c, hipStream_t stream)
  {
    if (!c->enc.profiling) return;
    if (c->enc.events.ensure(c->enc.eventsUsed + 1, hipEventDefault) != limg_hip_success) return;
    (void)hipEventRecord(c->enc.events[c->enc.eventsUsed++], stream);
  }
}

extern "C"
{
  const char *limg_hip_version(void) { return "limg_hip 0.1 (gfx950)"; }

  // limg_hip_options is versioned by its size (limg_hip.h): a caller compiled against an earlier, shorter header hands over fewer bytes
  void limg_hip_default_options_sized(limg_hip_options *o, size_t structSize)
  {
    if (!o || structSize < sizeof(uint32_t)) return;
    limg_hip_options d;
    memset(&d, 0, sizeof(d));
    d.forced_shift[0] = d.forced_shift[1] = d.forced_shift[2] = -1;
    const size_t n = structSize < sizeof(d) ? structSize : sizeof(d);
    d.struct_size = (uint32_t)n;
    memcpy(o, &d, n);
  }

#ifdef LIMG_HIP_TEST_HOOKS
  void limg_hip_default_test_options_sized(limg_hip_test_options *o, size_t structSize)
  {
    if (!o || structSize < sizeof(uint32_t)) return;
    limg_hip_test_options d;
    memset(&d, 0, sizeof(d));
    const size_t n = structSize < sizeof(d) ? structSize : sizeof(d);
    d.struct_size = (uint32_t)n;
    memcpy(o, &d, n);
  }

  limg_hip_result limg_hip_set_test_options(limg_hip_context *c, const limg_hip_test_options *o)
  {
    if (!c || !o) return limg_hip_error_ArgumentNull;
    const size_t n = o->struct_size;
    if (n < sizeof(uint32_t) || (n & 3u) != 0) return limg_hip_error_InvalidParameter;
    limg_hip_test_options full;
    limg_hip_default_test_options_sized(&full, sizeof(full));
    memcpy(&full, o, n < sizeof(full) ? n : sizeof(full));
    full.struct_size = (uint32_t)sizeof(full);
    c->topt = full;
    return limg_hip_success;
  }

  void limg_hip_test_live_resources(uint64_t out[5])
  {
    for (int i = 0; out && i < limg_hip_live::kCounts; i++) out[i] = limg_hip_live::count[i].load();
  }
#endif

  limg_hip_result limg_hip_init(int device, limg_hip_context **ppCtx)
  {
    if (!ppCtx) return limg_hip_error_ArgumentNull;
    *ppCtx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    {
      fprintf(stderr, "limg_hip: no HIP device available -- this library has no CPU fallback\n");
      return limg_hip_error_Generic;
    }
    if (device < 0) HIP_TRY(hipGetDevice(&device));
    if (device >= count) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(device));
    limg_hip_context *c = new (std::nothrow) limg_hip_context();
    if (!c) return limg_hip_error_MemoryAllocationFailure;
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->enc.persistentWorkgroups = 5 * prop.multiProcessorCount;
    limg_hip_default_options_sized(&c->opt, sizeof(c->opt));
#ifdef LIMG_HIP_TEST_HOOKS
    limg_hip_default_test_options_sized(&c->topt, sizeof(c->topt));
#endif
    *ppCtx = c;
    return limg_hip_success;
  }

  void limg_hip_shutdown(limg_hip_context **ppCtx)
  {
    if (!ppCtx || !*ppCtx) return;
    delete *ppCtx; // (an idle device first: ~limg_hip_context)
    *ppCtx = nullptr;
  }

  limg_hip_result limg_hip_set_options(limg_hip_context *c, const limg_hip_options *o)
  {
    if (!c || !o) return limg_hip_error_ArgumentNull;
    const size_t n = o->struct_size;
    if (n < offsetof(limg_hip_options, forced_shift) + sizeof(o->forced_shift) || (n & 3u) != 0) return limg_hip_error_InvalidParameter;
    limg_hip_options full;
    limg_hip_default_options_sized(&full, sizeof(full)); // members the caller's header did not have keep their defaults
    memcpy(&full, o, n < sizeof(full) ? n : sizeof(full));
    full.struct_size = (uint32_t)sizeof(full);
    c->opt = full;
    return limg_hip_success;
  }

  limg_hip_result limg_hip_get_options(const limg_hip_context *c, limg_hip_options *o)
  {
    if (!c || !o) return limg_hip_error_ArgumentNull;
    size_t n = o->struct_size; // the room the caller has
    if (n < sizeof(uint32_t) || (n & 3u) != 0) return limg_hip_error_InvalidParameter;
    if (n > sizeof(c->opt)) n = sizeof(c->opt);
    memcpy(o, &c->opt, n);
    o->struct_size = (uint32_t)n;
    return limg_hip_success;
  }

  // Blocks until the device is idle and reports a look-back timeout of the persistent kernel as limg_hip_error_Generic.  Observed once, in round 4: a build whose
  // workgroups took their first strip from blockIdx instead of the ticket dead-locked two contexts' kernels against each other until the bound fired;
  // with every strip id drawn from the ticket a look-back cannot wait on a workgroup that is not running.  The bound stays as the safety net, and a timeout is loud:
  // the strips behind it store nothing chain-dependent (limg_hip_lookback.h "decoupled look-back").
  limg_hip_result limg_hip_check_device_status(limg_hip_context *c)
  {
    if (!c) return limg_hip_error_ArgumentNull;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    if (c->enc.devStatus.p)
    {
      uint32_t word = 0;
      HIP_TRY(hipMemcpy(&word, c->enc.devStatus.p, 4, hipMemcpyDeviceToHost));
      if (word != 0)
      {
        HIP_TRY(hipMemset(c->enc.devStatus.p, 0, 4)); // sticky until reported once
        fprintf(stderr, "limg_hip: look-back timeout in the fused encode kernel\n");
        return limg_hip_error_Generic;
      }
      HIP_TRY(hipMemcpy(&word, (const uint8_t *)c->enc.devStatus.p + 4, 4, hipMemcpyDeviceToHost));
      if (word != 0)
      {
        HIP_TRY(hipMemset((uint8_t *)c->enc.devStatus.p + 4, 0, 4));
        fprintf(stderr, "limg_hip: a rank of the communicator aborted a single-chain encode; this rank's planes of that encode were not written\n");
        return limg_hip_error_Generic;
      }
    }
    if (c->stream.status.p)
    {
      uint32_t word = 0;
      HIP_TRY(hipMemcpy(&word, c->stream.status.p, 4, hipMemcpyDeviceToHost));
      if (word != 0)
      {
        HIP_TRY(hipMemset(c->stream.status.p, 0, 4));
        fprintf(stderr, "limg_hip: stream refused by the decode kernel (%s)\n", (word & 1u) ? "header mismatch" : "inconsistent payload offsets");
        return limg_hip_error_InvalidParameter;
      }
    }
    return limg_hip_success;
  }

  limg_hip_result limg_hip_last_stats(limg_hip_context *c, uint64_t *pCounters30, uint64_t *pPixels)
  {
    if (!c || !pCounters30) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry); // (the host-pointer entries write this state under the same lock)
    if (c->stats.state == 0) return limg_hip_error_InvalidParameter; // no encode with limg_hip_options.collect_stats since the last reset
    if (c->stats.state == 1)
    {
      HIP_TRY(hipSetDevice(c->device));
      HIP_TRY(hipMemcpyAsync(c->stats.host, c->stats.counters.p, 30 * 8, hipMemcpyDeviceToHost, c->stats.stream));
      HIP_TRY(hipStreamSynchronize(c->stats.stream));
      c->stats.state = 2;
    }
    memcpy(pCounters30, c->stats.host, 30 * 8);
    if (pPixels) *pPixels = c->stats.pixels;
    return limg_hip_success;
  }

  limg_hip_result limg_hip_profile_begin(limg_hip_context *c)
  {
    if (!c) return limg_hip_error_ArgumentNull;
    c->enc.profiling = true;
    c->enc.eventsUsed = 0;
    return limg_hip_success;
  }

  // Stops profiling, waits for the recorded work and writes, per profiled encode, {fit_search, scan (+ host chain walk for ragged
  // images), dither_store} milliseconds into pMs[3 * i ...].  Returns the number of encodes written (<= maxEncodes), or -1.
  int limg_hip_profile_end(limg_hip_context *c, float *pMs, int maxEncodes)
  {
    if (!c || !pMs) return -1;
    c->enc.profiling = false;
    const int n = (int)(c->enc.eventsUsed / 4);
    int written = 0;
    for (int i = 0; i < n && i < maxEncodes; i++, written++)
    {
      if (hipEventSynchronize(c->enc.events[4 * i + 3]) != hipSuccess) return -1;
      for (int k = 0; k < 3; k++)
        if (hipEventElapsedTime(&pMs[3 * i + k], c->enc.events[4 * i + k], c->enc.events[4 * i + k + 1]) != hipSuccess) return -1;
    }
    c->enc.eventsUsed = 0;
    return written;
  }

  size_t limg_hip_context_device_bytes(const limg_hip_context *c)
  {
    return c ? c->deviceBytes.load(std::memory_order_relaxed) : 0;
  }

  double limg_hip_compare_device(limg_hip_context *c, const uint32_t *a, const uint32_t *b, size_t sizeX, size_t sizeY, int hasAlpha, double *pMse, double *pMax, void *stream)
  {
    if (!c || !a || !b || sizeX == 0 || sizeY == 0) return NAN;
    if (hipSetDevice(c->device) != hipSuccess) return NAN;
    if (c->enc.cmp.ensure(8) != limg_hip_success) return NAN;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(c->enc.cmp.p, 0, 8, s) != hipSuccess) return NAN;
    launch_compare(a, b, (uint64_t)sizeX * sizeY, hasAlpha ? 4 : 3, (unsigned long long *)c->enc.cmp.p, s);
    unsigned long long err = 0;
    if (hipMemcpyAsync(&err, c->enc.cmp.p, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return NAN;
    // maxError = limg_color_error(min, max): red diff 255^2 >= 0x4000 => factors {3,4,2,3}
    const double maxError = 255.0 * 255.0 * (hasAlpha ? 12.0 : 9.0);
    const double mse = (double)err / (double)(sizeX * sizeY);
    if (pMse) *pMse = mse;
    if (pMax) *pMax = maxError;
    return 10.0 * log10(maxError / mse);
  }

  double limg_hip_compare(limg_hip_context *c, const uint32_t *a, const uint32_t *b, size_t sizeX, size_t sizeY, int hasAlpha, double *pMse, double *pMax)
  {
    if (!c || !a || !b || sizeX == 0 || sizeY == 0) return NAN;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (hipSetDevice(c->device) != hipSuccess) return NAN;
    const size_t bytes = sizeX * sizeY * 4;
    if (c->host.in.ensure(bytes) != limg_hip_success || c->host.planes.ensure(bytes) != limg_hip_success) return NAN;
    if (hipMemcpy(c->host.in.p, a, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(c->host.planes.p, b, bytes, hipMemcpyHostToDevice) != hipSuccess) return NAN;
    return limg_hip_compare_device(c, (const uint32_t *)c->host.in.p, (const uint32_t *)c->host.planes.p, sizeX, sizeY, hasAlpha, pMse, pMax, nullptr);
  }

  limg_hip_result limg_hip_synth_random_gradient_device(uint32_t *pOut, size_t width, size_t height, uint64_t seed, int opaque, size_t y0, void *stream)
  {
    if (!pOut) return limg_hip_error_ArgumentNull;
    launch_synth_random_gradient(pOut, (uint32_t)width, (uint32_t)height, seed, opaque, (uint32_t)y0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  limg_hip_result limg_hip_synth_photo_noise_device(uint32_t *pOut, size_t width, size_t height, uint64_t seed, size_t y0, void *stream)
  {
    if (!pOut) return limg_hip_error_ArgumentNull;
    launch_synth_photo_noise(pOut, (uint32_t)width, (uint32_t)height, seed, (uint32_t)y0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }
}
