// limg_hip_quality_step.h -- the search of the stream encode to a quality target (limg_hip_encode_stream_quality*) for the host and the device: the budget search of
// limg_hip_rate_step.h on the mirrored axis, with the error sum in the size's place.  Nothing of rate_step is restated here.  Plain C++: no HIP types, no library; a host
// compiler builds it on its own (tests/helpers/quality_step_check.cpp).
//
// The search runs over h = errorFactor / 2 in [hLo, hHi] and asks for E(h), the error sum of the stream at errorFactor 2 h against its own image (the sum of
// limg_hip_decode_stream_windows_error over the whole image), one value at a time.  It looks for a LARGE h -- the coarsest stream that is still good enough:
//
//   if E(hLo) > limit:                result = hLo, within = 0
//   elif E(hHi) <= limit:             result = hHi, within = 1
//   else: lo, hi = hLo, hHi           # E(lo) <= limit < E(hi)
//         while hi - lo > 1:
//             mid = hi - (hi - lo) // 2
//             if E(mid) <= limit: lo = mid
//             else: hi = mid
//         result = lo, within = 1
//
// With m = hLo + hHi - h this is rate_step's algorithm word for word: "size(m) <= budget" is "E(h) <= limit", its probe of the upper end is E(hLo), its probe of the
// lower end E(hHi), and its midpoint lo' + (hi' - lo') / 2 mirrors to hi - (hi - lo) / 2.  So the probe bound is rate_max_probes(hLo, hHi), every value is asked for
// once, and hLo == hHi asks once.
//
// What the result is: with within = 1 a value whose error was MEASURED and found to meet the limit.  It is the largest such h only where E() rises monotonically on
// [hLo, hHi], and it need not: the shift search is greedy and the dither differs between error factors, so a coarser stream can come out closer to the image.  The
// search may therefore return a smaller h than the largest that meets the limit.
#ifndef LIMG_HIP_QUALITY_STEP_H
#define LIMG_HIP_QUALITY_STEP_H

#include "limg_hip_rate_step.h"

namespace limg_hip
{
  struct QualityState
  {
    RateState mirrored; // the budget search over m = hLo + hHi - h; budget = the limit, bestBytes = E at its upper bracket end
    uint64_t axis;      // hLo + hHi (64 bits: any pair of bounds)
  };

  // the state before the first probe: hLo <= hHi
  LIMG_RATE_HD inline QualityState quality_begin(uint32_t hLo, uint32_t hHi, uint64_t limit)
  {
    QualityState s = { rate_begin(hLo, hHi, limit), (uint64_t)hLo + hHi };
    return s;
  }

  // the h whose error sum quality_step wants next; once done: the result
  LIMG_RATE_HD inline uint32_t quality_next(const QualityState &s) { return (uint32_t)(s.axis - s.mirrored.next); }
  LIMG_RATE_HD inline bool quality_done(const QualityState &s) { return s.mirrored.done != 0u; }
  // done: E(result) <= limit; the probes made; E(result)
  LIMG_RATE_HD inline uint32_t quality_within(const QualityState &s) { return s.mirrored.within; }
  LIMG_RATE_HD inline uint32_t quality_probes(const QualityState &s) { return s.mirrored.probes; }
  LIMG_RATE_HD inline uint64_t quality_error_sum(const QualityState &s) { return s.mirrored.bestBytes; }

  // errorSumOfNext = E(quality_next(s)).  Afterwards quality_done(s), or quality_next(s) is the next h to measure.
  LIMG_RATE_HD inline void quality_step(QualityState &s, uint64_t errorSumOfNext) { rate_step(s.mirrored, errorSumOfNext); }
}

#endif
