// limg_hip_rate_step.h -- the search of the budgeted stream encode (limg_hip_encode_stream_budget*) as ONE function for the host and the device: k_rate_step
// (limg_hip_rate.hip) calls it between two size probes, the fallback host loop (limg_hip_stream_encode_api.hip) between two stream encodes, and a host compiler builds it on
// its own (tests/helpers/rate_step_check.cpp).  Plain C++: no HIP types, no library.
//
// The search runs over h = errorFactor / 2 (the thresholds depend on errorFactor through errorFactor / 2 only) in [hLo, hHi] and asks for size(h), the stream's
// length in bytes at errorFactor 2 h, one value at a time:
//
//   if size(hHi) > budget:            result = hHi, within = 0
//   elif size(hLo) <= budget:         result = hLo, within = 1
//   else: lo, hi = hLo, hHi           # size(lo) > budget >= size(hi)
//         while hi - lo > 1:
//             mid = (lo + hi) // 2
//             if size(mid) <= budget: hi = mid
//             else: lo = mid
//         result = hi, within = 1
//
// (hLo == hHi asks for that one size once.)  At most 2 + ceil(log2(hHi - hLo)) values are asked for.
//
// What the result is: with within = 1 a value whose size was ASKED FOR and found to fit -- the stream is never longer than the budget.  It is the smallest fitting h
// only where size() is non-increasing on [hLo, hHi], and the shift search is greedy, so it need not be: a block can take more bits at a larger error factor.  The
// search may therefore return a larger h than the smallest that fits, and may refuse (within = 0) a budget that some h below hHi would have met.
#ifndef LIMG_HIP_RATE_STEP_H
#define LIMG_HIP_RATE_STEP_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LIMG_RATE_HD __host__ __device__
#else
#define LIMG_RATE_HD
#endif

namespace limg_hip
{
  enum : uint32_t { kRateProbeHi = 0, kRateProbeLo = 1, kRateBisect = 2 };

  struct RateState
  {
    uint32_t lo, hi;    // the bracket: size(lo) > budget >= size(hi) once phase == kRateBisect
    uint32_t next;      // the h whose size rate_step wants next; once done: the result
    uint32_t phase;     // kRateProbeHi, kRateProbeLo, kRateBisect: what `next` is
    uint32_t probes;    // sizes taken so far
    uint32_t done;      // the search is over: next = result
    uint32_t within;    // done: size(result) <= budget
    uint32_t reserved;
    uint64_t bestBytes; // size(hi) as far as it is known; once done: size(result)
    uint64_t budget;
  };

  // the state before the first probe: hLo <= hHi
  LIMG_RATE_HD inline RateState rate_begin(uint32_t hLo, uint32_t hHi, uint64_t budget)
  {
    RateState s = { hLo, hHi, hHi, kRateProbeHi, 0u, 0u, 0u, 0u, 0ull, budget };
    return s;
  }

  // probes the whole search makes at most: what a caller that cannot look at the state between two probes has to enqueue
  LIMG_RATE_HD inline uint32_t rate_max_probes(uint32_t hLo, uint32_t hHi)
  {
    uint32_t n = hHi > hLo ? 2u : 1u;
    for (uint64_t span = 1; span < (uint64_t)hHi - hLo; span <<= 1) n++; // ceil(log2(hHi - hLo)) bisection steps
    return n;
  }

  // bytesOfNext = size(s.next).  Afterwards s.done, or s.next is the next h to measure.
  LIMG_RATE_HD inline void rate_step(RateState &s, uint64_t bytesOfNext)
  {
    if (s.done) return;
    s.probes++;
    const bool fits = bytesOfNext <= s.budget;
    if (s.phase == kRateProbeHi)
    {
      s.bestBytes = bytesOfNext;
      if (!fits || s.lo == s.hi) { s.done = 1u; s.within = fits ? 1u : 0u; return; } // (next == hi already)
      s.phase = kRateProbeLo; s.next = s.lo;
      return;
    }
    if (s.phase == kRateProbeLo)
    {
      if (fits) { s.bestBytes = bytesOfNext; s.done = 1u; s.within = 1u; return; } // (next == lo)
      s.phase = kRateBisect;
    }
    else if (fits) { s.hi = s.next; s.bestBytes = bytesOfNext; }
    else s.lo = s.next;
    if (s.hi - s.lo > 1u) { s.next = s.lo + (s.hi - s.lo) / 2u; return; }
    s.next = s.hi; s.done = 1u; s.within = 1u;
  }
}

#endif
