// Host side of the merged-block encoder: the facts the GPU's similarity kernel and the host's merge share, and the host stages (the greedy raster merge,
// limg_hip_blocked_host.cpp; the dither chain walk, limg_hip_noise.cpp).  No HIP: the host-only units include it as it is, the rest through limg_hip_internal.h.
#ifndef LIMG_HIP_BLOCKED_HOST_H
#define LIMG_HIP_BLOCKED_HOST_H

#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "../../include/limg_hip.h"

namespace limg_hip
{
  // similarity bits are precomputed for candidate offsets dx, dy in [-kMatchLo, +kMatchHi] blocks around every seed: rectangles grow right / down from
  // their seed (far), and up / left only in the second attempt from the centre third (near); measured on the synthetic workloads, this window answers
  // 99.7 % of the merge's queries (the rest is evaluated on the host)
  constexpr int kMatchLo = 5, kMatchHi = 12;
  constexpr int kMatchSide = kMatchLo + kMatchHi + 1;   // 18
  constexpr int kMatchCells = kMatchSide * kMatchSide;  // 324
  constexpr int kMatchWords = (kMatchCells + 63) / 64;  // 6 x 64 bits per seed

  struct HostRegion { uint32_t ox, oy, rx, ry, keep; };

  void blocked_merge(const limg_hip_block_record *pass1, const unsigned long long *matchBits, uint32_t blocksX, uint32_t blocksY, int channels, std::vector<HostRegion> &out,
                     const std::function<void(size_t)> *progress = nullptr, const std::function<void(uint32_t)> *needSeedRow = nullptr, const uint8_t *seedFlags = nullptr,
                     const std::function<void()> *needRecords = nullptr);
  bool blocked_matches_host(int channels, const limg_hip_block_record &seed, const limg_hip_block_record &cand);
  uint64_t chain_walk_batch(uint64_t h, size_t count, const uint8_t *shiftWords, size_t stride, const uint32_t *npx, unsigned long long *noiseBase, unsigned long long *callState,
                            unsigned long long *callOff, uint32_t *callPx, uint64_t &noiseOff, size_t &callCount, size_t maxCalls, bool pcg); // limg_hip_noise.cpp
}

#endif
