// limg_hip_shim.hpp -- header-only C++ shim that re-exposes the reference's own signatures (src/limg.h:27-48, incl. limg_blocked_encode3d_test) on top of
// the C ABI of liblimg_hip.so, so a caller written against limg.h relinks unchanged -- the reference's own src/main.cpp compiles against it as it is
// (tests/test_shim_ref_main.py does exactly that):
//
//     #include "limg_hip_shim.hpp"      // instead of "limg.h"
//     limg_encode3d_test(pIn, sizeX, sizeY, hasAlpha, &info, errorFactor, pThreadPool, fastBitCrushing);
//
// The reference's thread pool only matters for its dither-chain partition (one chain per row strip, src/limg.cpp:2114-2134):
// the shim carries the thread count in an opaque `limg_thread_pool` so the GPU reproduces the same partition.
#ifndef LIMG_HIP_SHIM_HPP
#define LIMG_HIP_SHIM_HPP

#include <inttypes.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <functional>
#include <thread>
#include <vector>

#include "limg_hip.h"

enum limg_result
{
  limg_success = 0,
  limg_error_Generic = 100,
  limg_error_InvalidParameter,
  limg_error_ArgumentNull,
  limg_error_OutOfBounds,
  limg_error_MemoryAllocationFailure,
};

// The whole of src/limg_threading.h:9-17.  On the GPU a pool is only the name of a dither-chain partition, so it owns no threads: tasks given to
// `limg_thread_pool_add` are kept and run by the caller in `limg_thread_pool_await` (upstream's await also drains the queue on the calling thread,
// src/limg_threading.cpp:129-161).
struct limg_thread_pool { size_t threads; std::vector<std::function<void(void)>> tasks; };
inline limg_thread_pool *limg_thread_pool_new(const size_t threads) { return new limg_thread_pool{ threads, {} }; }
inline void limg_thread_pool_destroy(limg_thread_pool **pp) { if (pp && *pp) { delete *pp; *pp = nullptr; } }
inline size_t limg_thread_pool_thread_count(limg_thread_pool *p) { return (p == nullptr || p->threads == 0) ? 1 : p->threads; } // src/limg_threading.cpp:110-116
inline void limg_thread_pool_add(limg_thread_pool *p, const std::function<void(void)> &func) { p->tasks.push_back(func); }
inline void limg_thread_pool_await(limg_thread_pool *p)
{
  while (!p->tasks.empty())
  {
    std::vector<std::function<void(void)>> run;
    run.swap(p->tasks); // a task may add tasks
    for (auto &f : run) f();
  }
}
inline size_t limg_threading_max_threads() { return std::thread::hardware_concurrency(); } // src/limg_threading.cpp:163-166

namespace limg_hip_shim
{
  // pool -> the C ABI's `poolThreads` (0 = no pool = one dither chain; a pool of T threads = 4 T row strips, src/limg.cpp:2114-2134)
  inline int pool_threads(limg_thread_pool *p) { return p ? (int)limg_thread_pool_thread_count(p) : 0; }
}

struct limg_encode3d_info
{
  uint32_t *pDecoded, *pShiftABCX, *pColAMin, *pColAMax, *pColBMin, *pColBMax, *pColCMin, *pColCMax;
  uint8_t *pFactorsA, *pFactorsB, *pFactorsC;
};

struct limg_blocked_encode3d_info // src/limg.h:39-44
{
  uint32_t *pDecoded;
  uint8_t *pFactorsA, *pFactorsB, *pFactorsC, *pBlockError, *pBitsPerPixel;
  uint32_t *pShiftABCX, *pColAMin, *pColAMax, *pColBMin, *pColBMax, *pColCMin, *pColCMax, *pBlockIndex;
};

namespace limg_hip_shim
{
  // The reference keeps no state, so its entry points may be called from any number of threads at once (src/limg.cpp:1890-1891: scratch on the stack).  The shim's
  // callers get the same: ONE process-wide context, created on first use by whichever thread gets there first (a function-local static: initialisation is
  // thread-safe since C++11) and shut down when the process exits (the holder's destructor, registered after the HIP runtime's own exit handlers and therefore
  // run before them); the blocking host-pointer entries of the C ABI that the functions below call serialise on a mutex inside the context
  // (include/limg_hip.h "Thread safety").  Concurrent callers are correct, one encode at a time runs on the GPU.
  struct context_holder
  {
    limg_hip_context *ctx = nullptr;
    context_holder() { if (limg_hip_init(-1, &ctx) != limg_hip_success) ctx = nullptr; }
    ~context_holder() { limg_hip_shutdown(&ctx); }
    context_holder(const context_holder &) = delete;
    context_holder &operator=(const context_holder &) = delete;
  };
  inline limg_hip_context *context()
  {
    static context_holder holder;
    return holder.ctx;
  }

  // Upstream's limg_encode3d_test and limg_blocked_encode3d_test print their bit statistics themselves (src/limg.cpp:2232-2248, PRINT_TEST_OUTPUT is always defined);
  // the library is silent.  A caller that wants upstream's console output switches it on once -- limg_hip_shim::print_stats(true) -- and the two functions below then
  // print the same block, from the counters the GPU reduced (limg_hip_last_stats), after each encode.
  // The flag is the shim's own (an atomic: any thread may flip it); no option of the shared context is touched -- the two functions below ask for the counters of
  // THEIR encode through limg_hip_encode3d_stats / limg_hip_blocked_encode3d_stats, which encode and fetch under the context's mutex, so a thread always prints its own
  // call's block, like upstream (counters on the call's stack, src/limg.cpp:1975-1976).
  inline std::atomic<bool> &stats_flag() { static std::atomic<bool> on(false); return on; }
  inline void print_stats(const bool on) { stats_flag().store(on); }
  inline void print_stats_block(const uint64_t *a, const uint64_t pixels)
  {
    if (pixels == 0) return;
    const double t = (double)pixels;
    // one buffer, one write: blocks of concurrent callers do not interleave line by line
    char buf[1024];
    int n = snprintf(buf, sizeof(buf), "\nAverage Block Bits: %5.3f (A: %5.3f | B: %5.3f | C: %5.3f)\n\n", (a[0] + a[1] + a[2]) / t, a[0] / t, a[1] / t, a[2] / t);
    for (size_t i = 0; i < 9; i++) n += snprintf(buf + n, sizeof(buf) - (size_t)n, " %" PRIu64 " bit   ", (uint64_t)(8 - i));
    for (size_t f = 0; f < 3; f++)
    {
      n += snprintf(buf + n, sizeof(buf) - (size_t)n, "\n");
      for (size_t j = 0; j < 9; j++) n += snprintf(buf + n, sizeof(buf) - (size_t)n, "%7.4f  ", a[3 + f * 9 + j] * 100.0 / t);
    }
    n += snprintf(buf + n, sizeof(buf) - (size_t)n, "\n\n");
    fwrite(buf, 1, (size_t)n, stdout);
  }
}

inline limg_result limg_encode3d_test(const uint32_t *pIn, const size_t sizeX, const size_t sizeY, const bool hasAlpha, limg_encode3d_info *pInfo, const uint32_t errorFactor,
                                      limg_thread_pool *pThreadPool, const bool fastBitCrushing)
{
  static_assert(sizeof(limg_encode3d_info) == sizeof(limg_hip_encode3d_info), "layout");
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!limg_hip_shim::stats_flag().load())
    return (limg_result)limg_hip_encode3d(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, reinterpret_cast<limg_hip_encode3d_info *>(pInfo), errorFactor,
                                          limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0);
  uint64_t counters[30], pixels = 0;
  const limg_result r = (limg_result)limg_hip_encode3d_stats(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, reinterpret_cast<limg_hip_encode3d_info *>(pInfo), errorFactor,
                                                             limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0, counters, &pixels);
  if (r == limg_success) limg_hip_shim::print_stats_block(counters, pixels);
  return r;
}

inline limg_result limg_encode3d_test_perf(const uint32_t *pIn, const size_t sizeX, const size_t sizeY, const bool hasAlpha, const uint32_t errorFactor, limg_thread_pool *pThreadPool,
                                           const bool fastBitCrushing)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_encode3d_perf(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, errorFactor, limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0);
}

// src/limg.h:46.  The pool only splits upstream's first pass and cannot change the result; it is accepted and ignored.
inline limg_result limg_blocked_encode3d_test(const uint32_t *pIn, const size_t sizeX, const size_t sizeY, const bool hasAlpha, limg_blocked_encode3d_info *pInfo, const uint32_t errorFactor,
                                              limg_thread_pool * /* pThreadPool */, const bool fastBitCrushing)
{
  static_assert(sizeof(limg_blocked_encode3d_info) == sizeof(limg_hip_blocked_encode3d_info), "layout");
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!limg_hip_shim::stats_flag().load())
    return (limg_result)limg_hip_blocked_encode3d(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, reinterpret_cast<limg_hip_blocked_encode3d_info *>(pInfo), errorFactor, fastBitCrushing ? 1 : 0);
  uint64_t counters[30], pixels = 0;
  const limg_result r = (limg_result)limg_hip_blocked_encode3d_stats(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, reinterpret_cast<limg_hip_blocked_encode3d_info *>(pInfo), errorFactor,
                                                                     fastBitCrushing ? 1 : 0, counters, &pixels);
  if (r == limg_success) limg_hip_shim::print_stats_block(counters, pixels);
  return r;
}

inline double limg_compare(const uint32_t *pImageA, const uint32_t *pImageB, const size_t sizeX, const size_t sizeY, const bool hasAlpha, double *pMeanSquaredError,
                           double *pMaxPossibleSquaredError)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return 0.0;
  return limg_hip_compare(c, pImageA, pImageB, sizeX, sizeY, hasAlpha ? 1 : 0, pMeanSquaredError, pMaxPossibleSquaredError);
}

// `limg_encode` / `limg_decode`: named by the north-star, absent upstream (src/limg.h declares no such pair).  Build-defined wrappers over the
// compact "LMG3" stream of limg_hip.h: limg_decode(limg_encode(image)) == the pDecoded plane of limg_encode3d_test, bit for bit.
inline size_t limg_encode_bound(const size_t sizeX, const size_t sizeY) { return limg_hip_stream_bound(sizeX, sizeY); }

inline limg_result limg_encode(const uint32_t *pIn, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *pOut, const size_t outCapacity, size_t *pOutSize,
                               const uint32_t errorFactor = 100, limg_thread_pool *pThreadPool = nullptr, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_encode_stream(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, pOut, outCapacity, pOutSize, errorFactor, limg_hip_shim::pool_threads(pThreadPool),
                                             fastBitCrushing ? 1 : 0);
}

// limg_encode to a byte budget (limg_hip.h "stream encode to a byte budget"): the stream of limg_encode at the error factor a search over
// [minErrorFactor, maxErrorFactor] (even, 0 = 2 / 1024) chose for maxBytes.  *pErrorFactor, *pOutSize: what was chosen and what it takes; *pWithinBudget (may be NULL):
// false where even maxErrorFactor's stream is longer than maxBytes -- that stream is then what is written, and the call succeeds; *pProbes (may be NULL): sizes measured.
inline limg_result limg_encode_budget(const uint32_t *pIn, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *pOut, const size_t outCapacity, size_t *pOutSize,
                                      const size_t maxBytes, uint32_t *pErrorFactor, bool *pWithinBudget = nullptr, uint32_t *pProbes = nullptr,
                                      const uint32_t minErrorFactor = 0, const uint32_t maxErrorFactor = 0, limg_thread_pool *pThreadPool = nullptr, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!pOutSize || !pErrorFactor) return limg_error_ArgumentNull;
  limg_hip_budget_result res = { sizeof(limg_hip_budget_result), 0, 0, 0, 0 };
  const limg_result r = (limg_result)limg_hip_encode_stream_budget(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, pOut, outCapacity, maxBytes, minErrorFactor, maxErrorFactor,
                                                                   limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0, &res);
  if (r != limg_success && r != limg_error_OutOfBounds) return r;
  *pOutSize = (size_t)res.bytes; *pErrorFactor = res.errorFactor;
  if (pWithinBudget) *pWithinBudget = res.withinBudget != 0;
  if (pProbes) *pProbes = res.probes;
  return r;
}

// `count` images of one shape in one call (limg_hip.h "batched stream encode"): pOutSizes[i] bytes at ppOut[i] are what limg_encode writes for ppIn[i]; every ppOut[i]
// has room for outCapacityEach >= limg_encode_bound(sizeX, sizeY) bytes
inline limg_result limg_encode_batch(const uint32_t *const *ppIn, const size_t count, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *const *ppOut,
                                     const size_t outCapacityEach, size_t *pOutSizes, const uint32_t errorFactor = 100, limg_thread_pool *pThreadPool = nullptr,
                                     const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_encode_stream_batch(c, count, ppIn, sizeX, sizeY, hasAlpha ? 1 : 0, ppOut, outCapacityEach, pOutSizes, errorFactor,
                                                   limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0);
}

// limg_encode_batch with one error factor per image (limg_hip.h "each image at its own error factor"): pOutSizes[i] bytes at ppOut[i] are what limg_encode writes
// for ppIn[i] at pErrorFactors[i]
inline limg_result limg_encode_batch_ef(const uint32_t *const *ppIn, const size_t count, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *const *ppOut,
                                        const size_t outCapacityEach, size_t *pOutSizes, const uint32_t *pErrorFactors, limg_thread_pool *pThreadPool = nullptr,
                                        const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_encode_stream_batch_ef(c, count, ppIn, sizeX, sizeY, hasAlpha ? 1 : 0, ppOut, outCapacityEach, pOutSizes, pErrorFactors,
                                                      limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0);
}

// limg_encode_batch to byte budgets (limg_hip.h "budgeted stream encode of a list"): image i gets the stream limg_encode_budget writes for it with pMaxBytes[i], every
// image on a search of its own over the shared [minErrorFactor, maxErrorFactor].  pOutSizes[i], pErrorFactors[i]: what was chosen and what it takes; pWithinBudget[i],
// pProbes[i] (arrays of `count`, may be NULL) as limg_encode_budget's.  outCapacityEach below some pOutSizes[i]: limg_error_OutOfBounds with all sizes filled and
// nothing written to any ppOut[i].
inline limg_result limg_encode_budget_batch(const uint32_t *const *ppIn, const size_t count, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *const *ppOut,
                                            const size_t outCapacityEach, size_t *pOutSizes, const size_t *pMaxBytes, uint32_t *pErrorFactors, bool *pWithinBudget = nullptr,
                                            uint32_t *pProbes = nullptr, const uint32_t minErrorFactor = 0, const uint32_t maxErrorFactor = 0,
                                            limg_thread_pool *pThreadPool = nullptr, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!pOutSizes || !pErrorFactors) return limg_error_ArgumentNull;
  const limg_hip_budget_result blank = { sizeof(limg_hip_budget_result), 0, 0, 0, 0 };
  std::vector<limg_hip_budget_result> res(count ? count : 1, blank);
  const limg_result r = (limg_result)limg_hip_encode_stream_budget_batch(c, count, ppIn, sizeX, sizeY, hasAlpha ? 1 : 0, ppOut, outCapacityEach, pMaxBytes, minErrorFactor,
                                                                         maxErrorFactor, limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0, res.data());
  if (r != limg_success && r != limg_error_OutOfBounds) return r;
  for (size_t i = 0; i < count; i++)
  {
    pOutSizes[i] = (size_t)res[i].bytes; pErrorFactors[i] = res[i].errorFactor;
    if (pWithinBudget) pWithinBudget[i] = res[i].withinBudget != 0;
    if (pProbes) pProbes[i] = res[i].probes;
  }
  return r;
}

// limg_compare of an image with a stream's decode, without the decoded image (limg_hip.h "stream error inside the decode"): the value, *pMeanSquaredError and
// *pMaxPossibleSquaredError of limg_compare(pOriginal, limg_decode(pIn), ...) with the size and channel count of the stream's header; either stream version.
// `pixels`: of pOriginal, which must be the header's sizeX * sizeY.  NaN where the stream is refused.
inline double limg_compare_stream(const uint8_t *pIn, const size_t size, const uint32_t *pOriginal, const size_t pixels, double *pMeanSquaredError = nullptr,
                                  double *pMaxPossibleSquaredError = nullptr)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return NAN;
  return limg_hip_stream_compare(c, pIn, size, pOriginal, pixels, pMeanSquaredError, pMaxPossibleSquaredError);
}

// limg_encode to a quality target (limg_hip.h "stream encode to a quality target"): the stream of limg_encode at the coarsest error factor a search over
// [minErrorFactor, maxErrorFactor] (even, 0 = 2 / 1024) finds whose limg_compare PSNR against pIn is at least minPsnr dB.  *pErrorFactor, *pOutSize: what was chosen and
// what it takes; *pPsnr (may be NULL): the PSNR of the stream written; *pWithinTarget (may be NULL): false where even minErrorFactor's stream misses the target -- that
// stream is then what is written, and the call succeeds; *pProbes (may be NULL): errors measured.  A NaN minPsnr: limg_error_InvalidParameter.
inline limg_result limg_encode_quality(const uint32_t *pIn, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *pOut, const size_t outCapacity, size_t *pOutSize,
                                       const double minPsnr, uint32_t *pErrorFactor, double *pPsnr = nullptr, bool *pWithinTarget = nullptr, uint32_t *pProbes = nullptr,
                                       const uint32_t minErrorFactor = 0, const uint32_t maxErrorFactor = 0, limg_thread_pool *pThreadPool = nullptr, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!pOutSize || !pErrorFactor) return limg_error_ArgumentNull;
  if (minPsnr != minPsnr) return limg_error_InvalidParameter; // NaN names no target (limg_hip_error_sum_for_psnr would make it 0, the lossless one)
  limg_hip_quality_result res = { sizeof(limg_hip_quality_result), 0, 0, 0, 0, 0 };
  const limg_result r = (limg_result)limg_hip_encode_stream_quality(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, pOut, outCapacity,
                                                                    limg_hip_error_sum_for_psnr(sizeX, sizeY, hasAlpha ? 1 : 0, minPsnr), minErrorFactor, maxErrorFactor,
                                                                    limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0, &res);
  if (r != limg_success && r != limg_error_OutOfBounds) return r;
  *pOutSize = (size_t)res.bytes; *pErrorFactor = res.errorFactor;
  if (pPsnr) *pPsnr = 10.0 * log10(255.0 * 255.0 * (hasAlpha ? 12.0 : 9.0) * (double)sizeX * (double)sizeY / (double)res.errorSum); // limg_compare's, from the sum
  if (pWithinTarget) *pWithinTarget = res.withinTarget != 0;
  if (pProbes) *pProbes = res.probes;
  return r;
}

// limg_encode_quality of `count` images of one shape in one call: image i gets the stream limg_encode_quality writes for it with pMinPsnr[i], every image on a search
// of its own over the shared [minErrorFactor, maxErrorFactor].  pOutSizes[i], pErrorFactors[i]: what was chosen and what it takes; pPsnr[i], pWithinTarget[i],
// pProbes[i] (arrays of `count`, may be NULL) as limg_encode_quality's.  outCapacityEach below some pOutSizes[i]: limg_error_OutOfBounds with all sizes filled and
// nothing written to any ppOut[i].
inline limg_result limg_encode_quality_batch(const uint32_t *const *ppIn, const size_t count, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *const *ppOut,
                                             const size_t outCapacityEach, size_t *pOutSizes, const double *pMinPsnr, uint32_t *pErrorFactors, double *pPsnr = nullptr,
                                             bool *pWithinTarget = nullptr, uint32_t *pProbes = nullptr, const uint32_t minErrorFactor = 0, const uint32_t maxErrorFactor = 0,
                                             limg_thread_pool *pThreadPool = nullptr, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!pOutSizes || !pErrorFactors || !pMinPsnr) return limg_error_ArgumentNull;
  for (size_t i = 0; i < count; i++)
    if (pMinPsnr[i] != pMinPsnr[i]) return limg_error_InvalidParameter; // NaN names no target, as in limg_encode_quality
  const limg_hip_quality_result blank = { sizeof(limg_hip_quality_result), 0, 0, 0, 0, 0 };
  std::vector<limg_hip_quality_result> res(count ? count : 1, blank);
  std::vector<uint64_t> limits(count ? count : 1, 0);
  for (size_t i = 0; i < count; i++) limits[i] = limg_hip_error_sum_for_psnr(sizeX, sizeY, hasAlpha ? 1 : 0, pMinPsnr[i]);
  const limg_result r = (limg_result)limg_hip_encode_stream_quality_batch(c, count, ppIn, sizeX, sizeY, hasAlpha ? 1 : 0, ppOut, outCapacityEach, limits.data(), minErrorFactor,
                                                                          maxErrorFactor, limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0, res.data());
  if (r != limg_success && r != limg_error_OutOfBounds) return r;
  for (size_t i = 0; i < count; i++)
  {
    pOutSizes[i] = (size_t)res[i].bytes; pErrorFactors[i] = res[i].errorFactor;
    if (pPsnr) pPsnr[i] = 10.0 * log10(255.0 * 255.0 * (hasAlpha ? 12.0 : 9.0) * (double)sizeX * (double)sizeY / (double)res[i].errorSum);
    if (pWithinTarget) pWithinTarget[i] = res[i].withinTarget != 0;
    if (pProbes) pProbes[i] = res[i].probes;
  }
  return r;
}

// limg_encode of `count` images of ANY shapes in one call (limg_hip.h "stream encode of a list of mixed shapes"): pOutSizes[i] bytes at ppOut[i] are what limg_encode
// writes for ppIn[i] (pSizesX[i] x pSizesY[i]) at pErrorFactors[i].  pOutCapacities[i] below some pOutSizes[i]: limg_error_OutOfBounds with all sizes filled and nothing
// written to any ppOut[i].
inline limg_result limg_encode_list(const uint32_t *const *ppIn, const size_t count, const size_t *pSizesX, const size_t *pSizesY, const bool hasAlpha, uint8_t *const *ppOut,
                                    const size_t *pOutCapacities, size_t *pOutSizes, const uint32_t *pErrorFactors, limg_thread_pool *pThreadPool = nullptr,
                                    const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!ppIn || !pSizesX || !pSizesY || !ppOut || !pOutCapacities || !pErrorFactors) return limg_error_ArgumentNull;
  std::vector<limg_hip_stream_list_item> items(count ? count : 1);
  for (size_t i = 0; i < count; i++)
  {
    if (pSizesX[i] > 0xFFFFFFFFull || pSizesY[i] > 0xFFFFFFFFull) return limg_error_InvalidParameter;
    const limg_hip_stream_list_item it = { ppIn[i], ppOut[i], (uint64_t)pOutCapacities[i], (uint32_t)pSizesX[i], (uint32_t)pSizesY[i], pErrorFactors[i], 0u };
    items[i] = it;
  }
  return (limg_result)limg_hip_encode_stream_list(c, count, items.data(), sizeof(limg_hip_stream_list_item), hasAlpha ? 1 : 0, pOutSizes, limg_hip_shim::pool_threads(pThreadPool),
                                                  fastBitCrushing ? 1 : 0);
}

// limg_encode_quality of `count` images of ANY shapes in one call: image i gets the stream limg_encode_quality writes for it with pMinPsnr[i]; the outputs as
// limg_encode_quality_batch's, the capacities per image as limg_encode_list's.
inline limg_result limg_encode_quality_list(const uint32_t *const *ppIn, const size_t count, const size_t *pSizesX, const size_t *pSizesY, const bool hasAlpha,
                                            uint8_t *const *ppOut, const size_t *pOutCapacities, size_t *pOutSizes, const double *pMinPsnr, uint32_t *pErrorFactors,
                                            double *pPsnr = nullptr, bool *pWithinTarget = nullptr, uint32_t *pProbes = nullptr, const uint32_t minErrorFactor = 0,
                                            const uint32_t maxErrorFactor = 0, limg_thread_pool *pThreadPool = nullptr, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!ppIn || !pSizesX || !pSizesY || !ppOut || !pOutCapacities || !pOutSizes || !pErrorFactors || !pMinPsnr) return limg_error_ArgumentNull;
  const limg_hip_quality_result blank = { sizeof(limg_hip_quality_result), 0, 0, 0, 0, 0 };
  std::vector<limg_hip_quality_result> res(count ? count : 1, blank);
  std::vector<uint64_t> limits(count ? count : 1, 0);
  std::vector<limg_hip_stream_list_item> items(count ? count : 1);
  for (size_t i = 0; i < count; i++)
  {
    if (pMinPsnr[i] != pMinPsnr[i]) return limg_error_InvalidParameter; // NaN names no target, as in limg_encode_quality
    if (pSizesX[i] > 0xFFFFFFFFull || pSizesY[i] > 0xFFFFFFFFull) return limg_error_InvalidParameter;
    const limg_hip_stream_list_item it = { ppIn[i], ppOut[i], (uint64_t)pOutCapacities[i], (uint32_t)pSizesX[i], (uint32_t)pSizesY[i], 0u, 0u };
    items[i] = it;
    limits[i] = limg_hip_error_sum_for_psnr(pSizesX[i], pSizesY[i], hasAlpha ? 1 : 0, pMinPsnr[i]);
  }
  const limg_result r = (limg_result)limg_hip_encode_stream_quality_list(c, count, items.data(), sizeof(limg_hip_stream_list_item), hasAlpha ? 1 : 0, limits.data(), minErrorFactor,
                                                                         maxErrorFactor, limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0, res.data());
  if (r != limg_success && r != limg_error_OutOfBounds) return r;
  for (size_t i = 0; i < count; i++)
  {
    pOutSizes[i] = (size_t)res[i].bytes; pErrorFactors[i] = res[i].errorFactor;
    if (pPsnr) pPsnr[i] = 10.0 * log10(255.0 * 255.0 * (hasAlpha ? 12.0 : 9.0) * (double)pSizesX[i] * (double)pSizesY[i] / (double)res[i].errorSum);
    if (pWithinTarget) pWithinTarget[i] = res[i].withinTarget != 0;
    if (pProbes) pProbes[i] = res[i].probes;
  }
  return r;
}

// limg_encode_budget of `count` images of ANY shapes in one call (limg_hip.h "byte budget and size probe for a list of mixed shapes"): image i gets the stream
// limg_encode_budget writes for it with pMaxBytes[i]; the outputs as limg_encode_budget_batch's, the capacities per image as limg_encode_list's.
inline limg_result limg_encode_budget_list(const uint32_t *const *ppIn, const size_t count, const size_t *pSizesX, const size_t *pSizesY, const bool hasAlpha,
                                           uint8_t *const *ppOut, const size_t *pOutCapacities, size_t *pOutSizes, const size_t *pMaxBytes, uint32_t *pErrorFactors,
                                           bool *pWithinBudget = nullptr, uint32_t *pProbes = nullptr, const uint32_t minErrorFactor = 0, const uint32_t maxErrorFactor = 0,
                                           limg_thread_pool *pThreadPool = nullptr, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!ppIn || !pSizesX || !pSizesY || !ppOut || !pOutCapacities || !pOutSizes || !pErrorFactors || !pMaxBytes) return limg_error_ArgumentNull;
  const limg_hip_budget_result blank = { sizeof(limg_hip_budget_result), 0, 0, 0, 0 };
  std::vector<limg_hip_budget_result> res(count ? count : 1, blank);
  std::vector<limg_hip_stream_list_item> items(count ? count : 1);
  for (size_t i = 0; i < count; i++)
  {
    if (pSizesX[i] > 0xFFFFFFFFull || pSizesY[i] > 0xFFFFFFFFull) return limg_error_InvalidParameter;
    const limg_hip_stream_list_item it = { ppIn[i], ppOut[i], (uint64_t)pOutCapacities[i], (uint32_t)pSizesX[i], (uint32_t)pSizesY[i], 0u, 0u };
    items[i] = it;
  }
  const limg_result r = (limg_result)limg_hip_encode_stream_budget_list(c, count, items.data(), sizeof(limg_hip_stream_list_item), hasAlpha ? 1 : 0, pMaxBytes, minErrorFactor,
                                                                        maxErrorFactor, limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0, res.data());
  if (r != limg_success && r != limg_error_OutOfBounds) return r;
  for (size_t i = 0; i < count; i++)
  {
    pOutSizes[i] = (size_t)res[i].bytes; pErrorFactors[i] = res[i].errorFactor;
    if (pWithinBudget) pWithinBudget[i] = res[i].withinBudget != 0;
    if (pProbes) pProbes[i] = res[i].probes;
  }
  return r;
}

// The sizes limg_encode would give `count` images of ANY shapes at each of `factorCount` error factors, without encoding: pOutSizes[i * factorCount + k] for image i
// at pErrorFactors[k].
inline limg_result limg_stream_sizes_list(const uint32_t *const *ppIn, const size_t count, const size_t *pSizesX, const size_t *pSizesY, const bool hasAlpha,
                                          const uint32_t *pErrorFactors, const size_t factorCount, size_t *pOutSizes, limg_thread_pool *pThreadPool = nullptr,
                                          const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (!ppIn || !pSizesX || !pSizesY || !pErrorFactors || !pOutSizes) return limg_error_ArgumentNull;
  std::vector<limg_hip_stream_list_item> items(count ? count : 1);
  for (size_t i = 0; i < count; i++)
  {
    if (pSizesX[i] > 0xFFFFFFFFull || pSizesY[i] > 0xFFFFFFFFull) return limg_error_InvalidParameter;
    const limg_hip_stream_list_item it = { ppIn[i], nullptr, 0u, (uint32_t)pSizesX[i], (uint32_t)pSizesY[i], 0u, 0u };
    items[i] = it;
  }
  return (limg_result)limg_hip_stream_sizes_list(c, count, items.data(), sizeof(limg_hip_stream_list_item), hasAlpha ? 1 : 0, pErrorFactors, factorCount, pOutSizes,
                                                 limg_hip_shim::pool_threads(pThreadPool), fastBitCrushing ? 1 : 0);
}

// either version of the stream: version 1 (limg_encode) or version 2 (limg_blocked_encode)
inline limg_result limg_decode_info(const uint8_t *pIn, const size_t size, size_t *pSizeX, size_t *pSizeY, bool *pHasAlpha)
{
  int alpha = 0;
  limg_result r = (limg_result)limg_hip_stream_info(pIn, size, pSizeX, pSizeY, &alpha, nullptr);
  if (r != limg_success) r = (limg_result)limg_hip_blocked_stream_info(pIn, size, pSizeX, pSizeY, &alpha, nullptr, nullptr);
  if (pHasAlpha) *pHasAlpha = alpha != 0;
  return r;
}

inline limg_result limg_decode(const uint8_t *pIn, const size_t size, uint32_t *pOut, const size_t outPixelCapacity)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_decode_stream(c, pIn, size, pOut, outPixelCapacity);
}

// `limg_blocked_encode` / `limg_blocked_decode`: the same pair for what limg_blocked_encode3d_test computes (version 2 of the stream: rectangles of merged blocks):
// limg_blocked_decode(limg_blocked_encode(image)) == the pDecoded plane of limg_blocked_encode3d_test, bit for bit.
inline size_t limg_blocked_encode_bound(const size_t sizeX, const size_t sizeY) { return limg_hip_blocked_stream_bound(sizeX, sizeY); }

inline limg_result limg_blocked_encode(const uint32_t *pIn, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *pOut, const size_t outCapacity, size_t *pOutSize,
                                       const uint32_t errorFactor = 100, const bool fastBitCrushing = true)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_blocked_encode_stream(c, pIn, sizeX, sizeY, hasAlpha ? 1 : 0, pOut, outCapacity, pOutSize, errorFactor, fastBitCrushing ? 1 : 0);
}

// the stream of the LAST limg_blocked_encode3d_test / limg_blocked_encode of this process's context, without encoding again (single-threaded callers)
inline limg_result limg_blocked_last_encode(uint8_t *pOut, const size_t outCapacity, size_t *pOutSize)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_blocked_last_stream(c, pOut, outCapacity, pOutSize);
}

inline limg_result limg_blocked_decode(const uint8_t *pIn, const size_t size, uint32_t *pOut, const size_t outPixelCapacity)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_blocked_decode_stream(c, pIn, size, pOut, outPixelCapacity);
}

// A pixel rectangle of either version of the stream (as limg_decode_info accepts either): pOut[r * outStridePixels + c] = pixel (x + c, y + r) of what the version's
// full decoder gives, and nothing else is written (limg_hip.h "window decode").
inline limg_result limg_decode_window(const uint8_t *pIn, const size_t size, const size_t x, const size_t y, const size_t w, const size_t h, uint32_t *pOut, const size_t outStridePixels)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (limg_hip_blocked_stream_info(pIn, size, nullptr, nullptr, nullptr, nullptr, nullptr) == limg_hip_success)
    return (limg_result)limg_hip_blocked_decode_stream_window(c, pIn, size, x, y, w, h, pOut, outStridePixels);
  return (limg_result)limg_hip_decode_stream_window(c, pIn, size, x, y, w, h, pOut, outStridePixels);
}

// `count` windows of one stream of either version in one call: the stream is uploaded once and all windows decode in one batched launch (limg_hip.h "batched window
// decode"); a stream refused for any window leaves every pOut untouched.
inline limg_result limg_decode_windows(const uint8_t *pIn, const size_t size, const limg_hip_window *pWindows, const size_t count)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (limg_hip_blocked_stream_info(pIn, size, nullptr, nullptr, nullptr, nullptr, nullptr) == limg_hip_success)
    return (limg_result)limg_hip_blocked_decode_stream_windows(c, pIn, size, pWindows, count);
  return (limg_result)limg_hip_decode_stream_windows(c, pIn, size, pWindows, count);
}

// ... into planar float tensors (limg_hip.h "batched window decode into planar float tensors"): element (c, r, col) of window i = byte c of the pixel * scale[c] + bias[c]
inline limg_result limg_decode_windows_tensor(const uint8_t *pIn, const size_t size, const limg_hip_tensor_window *pWindows, const size_t count, const limg_hip_tensor_format *pFormat)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (limg_hip_blocked_stream_info(pIn, size, nullptr, nullptr, nullptr, nullptr, nullptr) == limg_hip_success)
    return (limg_result)limg_hip_blocked_decode_stream_windows_tensor(c, pIn, size, pWindows, count, pFormat);
  return (limg_result)limg_hip_decode_stream_windows_tensor(c, pIn, size, pWindows, count, pFormat);
}

// ... at reduced scale (limg_hip.h "reduced-scale window decode"): every window carries its level log2Scale = 0 .. 3 and is stated in that level's coordinates; pixel
// (X, Y) of level L is the rounded mean of the (1 << L)^2 box at ((X << L), (Y << L)).  All levels of a pyramid come from one upload and one batched call.
inline limg_result limg_decode_windows_scaled(const uint8_t *pIn, const size_t size, const limg_hip_scaled_window *pWindows, const size_t count)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (limg_hip_blocked_stream_info(pIn, size, nullptr, nullptr, nullptr, nullptr, nullptr) == limg_hip_success)
    return (limg_result)limg_hip_blocked_decode_stream_windows_scaled(c, pIn, size, pWindows, count);
  return (limg_result)limg_hip_decode_stream_windows_scaled(c, pIn, size, pWindows, count);
}

inline limg_result limg_decode_windows_scaled_tensor(const uint8_t *pIn, const size_t size, const limg_hip_scaled_tensor_window *pWindows, const size_t count,
                                                     const limg_hip_tensor_format *pFormat)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (limg_hip_blocked_stream_info(pIn, size, nullptr, nullptr, nullptr, nullptr, nullptr) == limg_hip_success)
    return (limg_result)limg_hip_blocked_decode_stream_windows_scaled_tensor(c, pIn, size, pWindows, count, pFormat);
  return (limg_result)limg_hip_decode_stream_windows_scaled_tensor(c, pIn, size, pWindows, count, pFormat);
}

// ... resized (limg_hip.h "resized window decode"): every window names a source rectangle in full-resolution pixels and the size of its output, which is resampled
// bilinearly from the level log2Scale = 0 .. 3 or LIMG_HIP_RESIZE_AUTO and mirrored where flags has LIMG_HIP_RESIZE_FLIP_X: a thumbnail, a viewer tile, a loader's sample.
inline limg_result limg_decode_windows_resized(const uint8_t *pIn, const size_t size, const limg_hip_resized_window *pWindows, const size_t count)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (limg_hip_blocked_stream_info(pIn, size, nullptr, nullptr, nullptr, nullptr, nullptr) == limg_hip_success)
    return (limg_result)limg_hip_blocked_decode_stream_windows_resized(c, pIn, size, pWindows, count);
  return (limg_result)limg_hip_decode_stream_windows_resized(c, pIn, size, pWindows, count);
}

inline limg_result limg_decode_windows_resized_tensor(const uint8_t *pIn, const size_t size, const limg_hip_resized_tensor_window *pWindows, const size_t count,
                                                      const limg_hip_tensor_format *pFormat)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  if (limg_hip_blocked_stream_info(pIn, size, nullptr, nullptr, nullptr, nullptr, nullptr) == limg_hip_success)
    return (limg_result)limg_hip_blocked_decode_stream_windows_resized_tensor(c, pIn, size, pWindows, count, pFormat);
  return (limg_result)limg_hip_decode_stream_windows_resized_tensor(c, pIn, size, pWindows, count, pFormat);
}

// Streams from streams, version 1, without decoding (limg_hip.h "stream splice"): the result decodes to the sources' pixels bit for bit.
// The stream of the w x h window at (x, y): x, y multiples of 8, x + w and y + h multiples of 8 or the image's edge.
inline limg_result limg_crop_stream(const uint8_t *pIn, const size_t size, const size_t x, const size_t y, const size_t w, const size_t h, uint8_t *pOut, const size_t outCapacity,
                                    size_t *pOutSize)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_stream_crop(c, pIn, size, x, y, w, h, pOut, outCapacity, pOutSize);
}

// the stream of the sizeX x sizeY image whose block grid the pieces -- rectangles of blocks of other streams -- cover exactly once
inline limg_result limg_splice_streams(const limg_hip_splice_piece *pPieces, const size_t count, const size_t sizeX, const size_t sizeY, const bool hasAlpha, uint8_t *pOut,
                                       const size_t outCapacity, size_t *pOutSize, const uint32_t errorFactor = 0, const uint32_t flags = 0)
{
  limg_hip_context *c = limg_hip_shim::context();
  if (!c) return limg_error_Generic;
  return (limg_result)limg_hip_stream_splice(c, pPieces, count, sizeof(limg_hip_splice_piece), sizeX, sizeY, hasAlpha ? 1 : 0, errorFactor, flags, pOut, outCapacity, pOutSize);
}

#endif // LIMG_HIP_SHIM_HPP
