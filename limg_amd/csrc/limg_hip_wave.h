// limg_hip_wave.h -- the wave / instruction helpers every kernel file uses: lane id, LDS fence, inclusive wave scan, the 24-bit multiply family and the other
// one-instruction wrappers, and the re-expansion multiplier of a shift.  Light on purpose: no float stage, no tables (those are limg_hip_device.h, which includes
// this file); the stream files include it directly.  Anonymous namespace: each including translation unit gets its own copy.
#ifndef LIMG_HIP_WAVE_H
#define LIMG_HIP_WAVE_H

#include "limg_hip_internal.h"

namespace limg_hip
{
  namespace
  {
    __device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

    // LDS traffic between the lanes of one wave: what was written before is visible after
    __device__ __forceinline__ void wave_lds_fence()
    {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }

    // inclusive prefix sum over the wave (32- or 64-bit values).  (k_stream_pack_strips scans halves of the wave with a loop of its own.)
    template <typename T>
    __device__ __forceinline__ T wave_scan_inclusive(T v, int lane)
    {
#pragma unroll
      for (int off = 1; off < 64; off <<= 1)
      {
        const T up = __shfl_up(v, off, 64);
        if (lane >= off) v += up;
      }
      return v;
    }

    // 24-bit integer multiplies (full rate; v_mul_lo_u32 is quarter rate).  Operands always fit: see kRecordLimit.
    __device__ __forceinline__ int mul_i24(int a, int b) { int r; asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
    __device__ __forceinline__ uint32_t mul_u24(uint32_t a, uint32_t b) { uint32_t r; asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
    // same with a wave-uniform factor straight from its SGPR (src0 of the VOP2 form): no v_mov to bring it into a VGPR first
    __device__ __forceinline__ uint32_t mul_u24_uniform(uint32_t a, uint32_t uniformB) { uint32_t r; asm("v_mul_u32_u24 %0, %2, %1" : "=v"(r) : "v"(a), "s"(uniformB)); return r; }
    __device__ __forceinline__ int med3_i32(int a, int b, int c) { int r; asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
    __device__ __forceinline__ int mad_i24(int a, int b, int c) { int r; asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
    __device__ __forceinline__ int add3(int a, int b, int c) { int r; asm("v_add3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
    __device__ __forceinline__ uint32_t bfe(uint32_t v, uint32_t off, uint32_t width) { uint32_t r; asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(off), "v"(width)); return r; }
    __device__ __forceinline__ uint32_t lshl_or(uint32_t a, uint32_t sh, uint32_t b) { uint32_t r; asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(sh), "v"(b)); return r; }

    // (1 << s) + decode_bias(s)  (src/limg_bit_crush_simd.h:611-619 / src/limg_decode.h:172-178): 1,2,4,8,17,36,85,255,256
    // (packed-constant form, for s <= 8 only; k_stream_decode keeps a chain of selects of its own)
    __device__ __forceinline__ uint32_t shift_mul(uint32_t s)
    {
      const uint64_t biasPacked = (1ull << 28) | (4ull << 35) | (21ull << 42) | (127ull << 49); // 7 bits per shift value
      return (1u << s) + (uint32_t)((biasPacked >> (7 * s)) & 127u);
    }
  }
}

#endif
