// limg_hip_lookback.h -- decoupled look-back over the per-strip dither-call counts of the persistent kernel.
// Included by limg_hip_kernels.hip only, which stays one translation unit (its per-source compile flags cover this code).
#ifndef LIMG_HIP_LOOKBACK_H
#define LIMG_HIP_LOOKBACK_H

#include "limg_hip_device.h"

namespace limg_hip
{
  namespace
  {
    // ---- decoupled look-back over the per-strip dither-call counts (fused path) ------------------------------------------
    // One 8-byte descriptor per work strip: value in the low word, status in the high word (0 = nothing yet, 1 = this strip's
    // own count, 2 = inclusive count of the chain up to and including this strip; the inclusive VALUE kBasePoison = a look-back
    // gave up here or earlier in the chain).  Written and read with relaxed agent-scope 8-byte atomics only: value and status travel in one granule, so no other ordering is needed.
    // Progress: EVERY strip id is drawn from the atomic ticket by a workgroup that is already running (k_encode_persistent), so
    // the holders of all smaller ids are resident whatever else shares the GPU -- other contexts' persistent kernels included --
    // and each of them publishes its count at the end of an E step, which never waits.  A look-back therefore terminates
    // without any assumption about how many workgroups of the grid are resident.  (Reference: strips on a thread pool always
    // complete and the entry points are re-entrant, src/limg.cpp:1890-1893, :2131-2136.)
    // The spin is bounded all the same (a protocol bug must not hang the GPU).  A timeout is LOUD: the strip raises the
    // context's sticky status word, publishes the poison value as its inclusive count and stores none of its chain-dependent planes;
    // every later strip of the chain finds the poison at once (no second spin), hands it on and stores nothing either.  (A poison STATUS of
    // its own, tested with one more ballot per poll, cost the 4-channel kernel two spilled VGPRs at its 80-register limit; the value does not.)  The host-pointer entries and
    // limg_hip_check_device_status then return limg_hip_error_Generic.
    constexpr uint32_t kDescAggregate = 1u, kDescInclusive = 2u;
    constexpr uint32_t kBasePoison = 0xFFFFFFFFu; // (a chain has < 2^26 dither calls: 3 per block)

    __device__ __forceinline__ void desc_store(unsigned long long *d, uint32_t status, uint32_t value)
    {
      __hip_atomic_store(d, ((unsigned long long)status << 32) | value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ unsigned long long desc_load(unsigned long long *d)
    {
      return __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // bound of one look-back wait, in polls (~seconds); fault injection (a shorter bound, a strip that never publishes) exists in the test build only
    template <class P>
    __device__ __forceinline__ uint32_t lookback_spin_bound(const P &p)
    {
#ifdef LIMG_HIP_TEST_HOOKS
      return p.lookbackSpins;
#else
      (void)p;
      return 1u << 22;
#endif
    }
    template <class P>
    __device__ __forceinline__ bool publishes(const P &p, uint32_t id)
    {
#ifdef LIMG_HIP_TEST_HOOKS
      return id != p.testSkipStrip;
#else
      (void)p; (void)id;
      return true;
#endif
    }

    // called by all 64 lanes of one wave; returns the number of dither calls of the chain before strip `id`, or kBasePoison
    template <class P>
    __device__ __forceinline__ uint32_t lookback_base(const P &p, uint32_t id, uint32_t headId, uint32_t agg, int lane)
    {
      if (id == headId) return 0u;
      uint32_t base = 0;
      int hi = (int)id - 1; // nearest predecessor not yet accounted for
      for (;;)
      {
        const int j = hi - lane; // lane 0 looks at the nearest one
        const bool inrange = j >= (int)headId;
        unsigned long long d = ((unsigned long long)kDescInclusive << 32); // before the chain head: inclusive 0
        uint32_t spins = 0;
        for (;;)
        {
          if (inrange) d = desc_load(p.desc + j);
          const uint64_t incl = __builtin_amdgcn_ballot_w64((uint32_t)(d >> 32) == kDescInclusive);
          const uint64_t none = __builtin_amdgcn_ballot_w64((uint32_t)(d >> 32) == 0u);
          // every strip nearer than the nearest inclusive one must have published at least its own count
          const uint64_t nearer = incl ? ((incl & (0ull - incl)) - 1ull) : ~0ull;
          if ((none & nearer) == 0ull)
          {
            const uint32_t v = (uint32_t)d;
            if (incl)
            {
              const int fl = __builtin_ctzll(incl);
              const uint32_t vi = (uint32_t)__builtin_amdgcn_readlane((int)v, fl);
              base += wave_sum(lane <= fl ? v : 0u);
              return vi == kBasePoison ? kBasePoison : base; // (a poisoned predecessor publishes "inclusive, kBasePoison")
            }
            base += wave_sum(v);
            break;
          }
          if (++spins > lookback_spin_bound(p))
          {
            if (lane == 0) atomicExch(p.timeout, 1u);
            return kBasePoison;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        hi -= 64;
      }
    }
  } // namespace
} // namespace limg_hip

#endif
