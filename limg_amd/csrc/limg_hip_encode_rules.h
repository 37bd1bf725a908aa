// limg_hip_encode_rules.h -- three rules of the 8x8 encode that the host units and one kernel file state alike, each written ONCE for the host and the device:
// the bit-crush thresholds of an error factor (encode_params, the merged-block encoder's set_up, k_rate_begin / k_rate_step), the forced shift triple (every
// parameter block with a `forced` member) and the images of one launch pair of a list (limg_hip_encode3d_batch_device, the batched and the budgeted stream
// encode).  A host compiler builds it on its own (tests/helpers/encode_rules_check.cpp).  Plain C++: no HIP types, no library.
#ifndef LIMG_HIP_ENCODE_RULES_H
#define LIMG_HIP_ENCODE_RULES_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/limg_hip.h" // limg_hip_block_record: what a block of a launch pair costs

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LIMG_RULES_HD __host__ __device__
#else
#define LIMG_RULES_HD
#endif

namespace limg_hip
{
  // thresholds and flags of an error factor, src/limg.cpp:2186-2212 (the merged-block encoder: 2343-2368, the same values)
  struct Thresholds
  {
    uint32_t maxPixel32;     // min(maxPixelBitCrushError, 2^32 - 1)
    uint32_t blockLimitFull; // min(ceil(maxBlock * 64 / 16), 2^32 - 1): what a full block's error sum is compared with (be * 16 < maxBlock * n)
    uint64_t maxBlock;       // maxBlockBitCrushError
    uint32_t crushBits;
  };
  LIMG_RULES_HD inline Thresholds thresholds(uint32_t errorFactor)
  {
    const uint64_t maxPixel = (uint64_t)0x6 * (errorFactor / 2) * 7, maxBlock = (uint64_t)0x4 * (errorFactor / 2) * 7;
    const uint64_t lim = (maxBlock * 64ull + 15ull) >> 4;
    Thresholds t;
    t.maxPixel32 = maxPixel > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)maxPixel;
    t.blockLimitFull = lim > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)lim;
    t.maxBlock = maxBlock;
    t.crushBits = errorFactor != 0 ? 1u : 0u;
    return t;
  }

  // The packed trial weights a pixel's squared differences (2, 4, 3) while dR^2 < 0x4000 and (3, 4, 2) otherwise (src/limg_bit_crush_simd.h; trial_pixel_error,
  // limg_hip_search.h).  Below a pixel limit of 0x8000 the second form never decides anything, and a launch whose host knows the limit takes a trial without it:
  //  * a pixel with dR^2 >= 0x4000 has the error 3 dR^2 + 4 dG^2 + 2 dB^2 >= 49152, and its first-form value 2 dR^2 + 4 dG^2 + 3 dB^2 is >= 32768: with
  //    maxPixel32 <= 32767 it fails the pixel test (err > maxPixel32) under either form;
  //  * a pixel with dR^2 < 0x4000 has the same value under both.
  // So the pixel-failure ballot of a trial is the same; the block sum is only read where no pixel failed, i.e. where every pixel has dR^2 < 0x4000 and every
  // summand is the same, so the sum verdict and every block error the accurate search compares are the same too.  The bound is tight: at a limit of 32768 the
  // pixel (|dR|, |dG|, |dB|) = (128, 0, 0) passes under the first form (32768) and fails under the second (49152).  maxPixel32 = 42 * (errorFactor / 2) stays
  // below 0x8000 exactly for errorFactor <= 1561 (1562: 32802).  tests/test_red_select_cpu.py walks all 256^3 difference triples.
  LIMG_RULES_HD inline bool red_select_dead(uint32_t maxPixel32) { return maxPixel32 < 0x8000u; }

  // limg_hip_options.forced_shift -> the kernels' `forced`: the triple if all three are in 0..8, else {-1, -1, -1} (the shift search runs)
  LIMG_RULES_HD inline void forced_shifts(const int32_t forced_shift[3], int32_t forced[3])
  {
    const bool all = forced_shift[0] >= 0 && forced_shift[0] <= 8 && forced_shift[1] >= 0 && forced_shift[1] <= 8 && forced_shift[2] >= 0 && forced_shift[2] <= 8;
    for (int i = 0; i < 3; i++) forced[i] = all ? forced_shift[i] : -1;
  }

  // Images of one shape that go into ONE launch pair: the per-block scratch of a launch pair is bounded (1 GiB of records) and strip ids are 32 bits; at least one.
  // hook: the test build's batch_chunk, 0 = none -- fewer images per pair, never more than the bounds allow.  blocks, strips: of one image, both > 0.  These are the
  // chunks list_chunk_end (limg_hip_list_plan.h) gives on a list of that one shape: tests/test_list_plan_cpu.py.
  LIMG_RULES_HD inline size_t list_chunk(size_t blocks, size_t strips, size_t hook)
  {
    size_t chunk = (size_t)(1ull << 30) / (blocks * sizeof(limg_hip_block_record));
    if (chunk * strips > 0x7FFFFFFFull) chunk = 0x7FFFFFFFull / strips;
    if (hook > 0 && hook < chunk) chunk = hook;
    return chunk < 1 ? 1 : chunk;
  }
}

#endif
