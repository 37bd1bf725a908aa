// limg_hip_fit_tpb.hip -- the float stage (a4-a6: channel sums, 3/4-pass direction fit, extrema, record) with ONE LANE PER 8x8 BLOCK.
//
// reference: limg_encode_sum_to_decomposition_state src/limg.cpp:466-497, limg_encode_get_block_factors_accurate_from_state_3d_{3,4}
// src/limg_factorization.h:382-576 / :578-794, record rounding :764-790.
//
// Why a second mapping.  With lane == pixel (limg_hip_float_pixel.h) every per-block quantity of the fit is a wave reduction: two channel sums, six extrema and --
// the expensive one, because the reference accumulates in pixel order -- three direction sums that have to be parked in LDS and walked by 16 lanes.  The float
// stage is a chain of four passes whose per-pixel arithmetic is tiny next to that bookkeeping (~510 of the kernel's ~1060 VALU instructions per block).  With
// lane == block the same per-pixel arithmetic is issued once per pixel for 64 blocks (identical cost per block), and every reduction disappears: a direction sum
// is four plain `v_add_f32` per pixel in the natural loop order (which IS the reference's order), extrema are `v_min/v_max` in the loop, per-block "uniform" values
// are ordinary registers.  No barrier, no DPP, no readlane: a workgroup is one wave that owns 64 adjacent blocks (512 x 8 pixels).
// The per-pixel helpers (unit4, dp4: DPPS order, captured RSQRTPS table, no contraction) are the very functions of limg_hip_device.h, so the records are
// bit-identical to the lane == pixel path's -- the parity tests run both.  Only whole 8x8 blocks: images with partial edge blocks keep the other path.
//
// LDS (only when the input rows are not 16-byte aligned; see DIRECT below): the 64 blocks' pixels, block-major with a stride of 68 dwords (16-byte aligned rows; 68 = 4 mod 64 makes every 16-lane group of a ds_read_b128 hit 64
// distinct banks).  17 KiB per wave.  The passes re-read the pixels from LDS (2 x ds_read_b128 per row).
#include "limg_hip_device.h"

#include <string.h>

namespace limg_hip
{
  namespace
  {
    constexpr int kTpbStride = 68;

    // DIRECT (input rows 16-byte aligned, the normal case): every lane reads its block's rows straight from global memory (two 16-byte loads per row and pass;
    // the rows are re-read from L2 by passes 2-4) -- no LDS but the RSQRTPS table (8 KiB per workgroup of four waves), so the registers (166 => 3 waves per SIMD
    // = 12 per CU) set the occupancy.  Otherwise the 64 blocks' pixels are staged in LDS first (dword loads), 17 KiB per wave, two waves per workgroup
    // (2 x 17 + 8 KiB => 3 workgroups = 6 waves per CU).  Occupancy is not what the kernel lacks: forced down to 61 VGPRs (8 waves per SIMD) it runs at the same
    // speed -- it is issue-bound on its instruction count.
    template <bool DIRECT> constexpr int tpb_waves() { return DIRECT ? 4 : 2; } // waves per workgroup: they share one copy of the table

    // The eight rows of a lane's block, two per iteration, the NEXT two already requested: a pass is a chain of (load 32 bytes, 8 pixels of arithmetic) per row, and
    // with few waves on a SIMD -- a 4096^2 image is one round of 4 waves per SIMD, the sub-batch pipeline leaves this kernel one -- nothing else covers the load's
    // latency.  (The last iteration re-requests rows 6 and 7: harmless, and the loop stays free of a branch.)
    template <class BODY>
    __device__ __forceinline__ void for_rows(const uint32_t *my, const uint32_t pitch, BODY &&body)
    {
      uint4 u0 = *reinterpret_cast<const uint4 *>(my), w0 = *reinterpret_cast<const uint4 *>(my + 4);
      uint4 u1 = *reinterpret_cast<const uint4 *>(my + pitch), w1 = *reinterpret_cast<const uint4 *>(my + pitch + 4);
#pragma unroll 1
      for (int r = 0; r < 8; r += 2)
      {
        const uint32_t *nx = my + (r + 2 < 8 ? r + 2 : 6) * pitch;
        const uint4 nu0 = *reinterpret_cast<const uint4 *>(nx), nw0 = *reinterpret_cast<const uint4 *>(nx + 4);
        const uint4 nu1 = *reinterpret_cast<const uint4 *>(nx + pitch), nw1 = *reinterpret_cast<const uint4 *>(nx + pitch + 4);
        {
          const uint32_t q[8] = { u0.x, u0.y, u0.z, u0.w, w0.x, w0.y, w0.z, w0.w };
          body(r, q);
        }
        {
          const uint32_t q[8] = { u1.x, u1.y, u1.z, u1.w, w1.x, w1.y, w1.z, w1.w };
          body(r + 1, q);
        }
        u0 = nu0; w0 = nw0; u1 = nu1; w1 = nw1;
      }
    }

    template <int CH, bool FAST, bool DIRECT>
    // (8 waves per SIMD asked for explicitly: left to itself the compiler settles on 61 registers or on 132 depending on details of the epilogue; measured equal in
    //  speed on large images -- the kernel is issue-bound -- but a 4096^2 image is a single round of 4096 waves, where residency is what there is)
    __global__ __launch_bounds__(64 * tpb_waves<DIRECT>(), DIRECT ? 5 : 1) void k_fit_tpb(const EncodeParams p)
    {
      constexpr int kTpbWaves = tpb_waves<DIRECT>();
      __shared__ __attribute__((aligned(16))) uint32_t s_pxAll[kTpbWaves][DIRECT ? 4 : 64 * kTpbStride];
      // the RSQRTPS table in LDS: a per-lane gather of 64 unrelated 2-byte entries costs the texture path ~64 address cycles per wave instruction from global
      // memory, but only a few LDS cycles (random banks)
      // 8 KiB: T[j] = table[j ^ 0x400] << 11, the form unit4<..., TAB32> reads (entry in mantissa position, no index flip)
      __shared__ __attribute__((aligned(16))) uint32_t s_tab[FAST ? 4 : 2048];
      const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
      // Next to a persistent kernel (sub-batch pipeline) this kernel has ONE wave per SIMD against the other's five: at equal priority it would get a sixth of the
      // issue slots and become the pipeline's critical path.  Raised above the E step's priority, its one wave takes what a single wave can issue.
      if (p.fitPrio == 3) __builtin_amdgcn_s_setprio(3);
      else if (p.fitPrio == 2) __builtin_amdgcn_s_setprio(2);
      else if (p.fitPrio == 1) __builtin_amdgcn_s_setprio(1);
#define LIMG_FIT_TPB_TABLE
#include "limg_hip_fit_tpb_body.inc"
#undef LIMG_FIT_TPB_TABLE
      uint32_t *s_px = s_pxAll[wave];
      const uint32_t unitsX = (p.blocksX + 63u) / 64u;
      const uint32_t unitId = blockIdx.x * kTpbWaves + wave;
      if (unitId >= unitsX * p.blocksY * p.batchCount) return; // whole wave; after the only barrier
      const uint32_t unit = unitId % unitsX, byS = unitId / unitsX; // byS: block row counted through all images of a batch (= row in the per-block scratch)
      const uint32_t img = p.batchCount > 1 ? byS / p.blocksY : 0u, by = byS - img * p.blocksY;
      const uint32_t *const pin = p.batchCount > 1 ? p.batch[img].in : p.io.in;
      const uint32_t bx0 = unit * 64u, x0 = bx0 * kBlock, y0 = by * kBlock;
      const uint32_t nBlocks = min(p.blocksX - bx0, 64u), widthPx = nBlocks * kBlock;
      if (p.zeroLookback)
      { // this wave's 64 blocks are two work strips of the persistent kernel: clear their look-back descriptors (and, once, the ticket) instead of a memset launch
        if ((uint32_t)lane < 2u && unit * 2u + (uint32_t)lane < p.stripsX) p.desc[(size_t)byS * p.stripsX + unit * 2u + (uint32_t)lane] = 0ull;
        if (unitId == 0 && lane < 4) p.ticket[lane] = 0u;
      }

#include "limg_hip_fit_tpb_body.inc"
    }

    // ---- the float stage of a list whose images differ in shape (limg_hip_encode_stream_list*; layout: limg_hip_list_plan.h) ----
    // The same body over the chunk's concatenated unit list.  A unit is up to 64 adjacent blocks of one block row of ONE image; which image, a wave finds by a
    // binary search over the unit prefix (wave-uniform, scalar loads), and what the body reads of `p` is that image's: its width, its pixels, and its slice of
    // the records and invN, offset to its first block.  The tables were written by launches that precede this one on the stream: constant address space.
    struct FitUnitView
    {
      uint32_t sizeX, blocksX;
      int32_t vecIn;
      limg_hip_block_record *records;
      float *invN;
    };
    // (entry of a uint32 prefix of n entries that holds x: base[i] <= x < base[i + 1])
    __device__ __forceinline__ uint32_t find_prefix(const uint32_t *base, uint32_t n, uint32_t x)
    {
      const __attribute__((address_space(4))) uint32_t *b = (const __attribute__((address_space(4))) uint32_t *)(uintptr_t)base;
      uint32_t lo = 0, hi = n;
      while (hi - lo > 1u)
      {
        const uint32_t mid = (lo + hi) >> 1;
        if (b[mid] <= x) lo = mid; else hi = mid;
      }
      return (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    }

    template <int CH, bool FAST, bool DIRECT>
    __global__ __launch_bounds__(64 * tpb_waves<DIRECT>(), DIRECT ? 5 : 1) void k_fit_tpb_list(const FitListParams lp)
    {
      constexpr int kTpbWaves = tpb_waves<DIRECT>();
      __shared__ __attribute__((aligned(16))) uint32_t s_pxAll[kTpbWaves][DIRECT ? 4 : 64 * kTpbStride];
      __shared__ __attribute__((aligned(16))) uint32_t s_tab[FAST ? 4 : 2048];
      const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#define LIMG_FIT_TPB_TABLE
#include "limg_hip_fit_tpb_body.inc"
#undef LIMG_FIT_TPB_TABLE
      uint32_t *s_px = s_pxAll[wave];
      const uint32_t unitId = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kTpbWaves + wave));
      if (unitId >= lp.nUnits) return; // whole wave; after the only barrier
      const uint32_t img = find_prefix(lp.firstUnit, lp.nImages, unitId);
      typedef const __attribute__((address_space(4))) ListImage KernImage;
      typedef const __attribute__((address_space(4))) ImageIO KernIO;
      KernImage *const im = (KernImage *)(uintptr_t)lp.images + img;
      const uint32_t unitsX = (im->blocksX + 63u) / 64u, localUnit = unitId - im->firstUnit;
      const uint32_t unit = localUnit % unitsX, by = localUnit / unitsX, byS = by; // (the image's slices start at its first block: its rows count from 0)
      const uint32_t *const pin = (const uint32_t *)(const __attribute__((address_space(1))) uint32_t *)((KernIO *)(uintptr_t)lp.batch + img)->in;
      FitUnitView p;
      p.sizeX = im->sizeX; p.blocksX = im->blocksX; p.vecIn = (im->vec & kListVecIn) ? 1 : 0;
      p.records = lp.records + im->firstBlock; p.invN = lp.invN + 4 * im->firstBlock;
      const uint32_t bx0 = unit * 64u, x0 = bx0 * kBlock, y0 = by * kBlock;
      const uint32_t nBlocks = min(p.blocksX - bx0, 64u), widthPx = nBlocks * kBlock;
      { // this wave's 64 blocks are two work strips of the persistent launch that follows: their look-back descriptors, and (once) the ticket
        const uint32_t stripsX = im->stripsX;
        if ((uint32_t)lane < 2u && unit * 2u + (uint32_t)lane < stripsX) lp.desc[(size_t)im->firstStrip + (size_t)by * stripsX + unit * 2u + (uint32_t)lane] = 0ull;
        if (unitId == 0 && lane < 4) lp.ticket[lane] = 0u;
      }

#include "limg_hip_fit_tpb_body.inc"
    }
  }

  void launch_fit_tpb_list(const FitListParams &p, int channels, bool floatFast, bool direct, hipStream_t s)
  {
    with_flags([&](auto rgba, auto FAST, auto DIRECT)
               { hipLaunchKernelGGL((k_fit_tpb_list<rgba ? 4 : 3, FAST, DIRECT>), dim3((p.nUnits + tpb_waves<DIRECT>() - 1) / tpb_waves<DIRECT>()), dim3(64 * tpb_waves<DIRECT>()), 0, s, p); },
               channels == 4, floatFast, direct);
  }

  namespace
  {
    // any table of a list call, as 32-bit words through kernel arguments (as k_set_batch_table: stream-ordered, and the host array may die right away)
    struct WordChunk { uint32_t n; uint32_t w[768]; };
    static_assert(sizeof(WordChunk) <= 3584, "kernel-argument segment");
    __global__ void k_set_words(uint32_t *dst, const WordChunk chunk)
    {
      for (uint32_t i = threadIdx.x; i < chunk.n; i += blockDim.x) dst[i] = chunk.w[i];
    }
  }

  void launch_set_words(void *dDst, const void *hSrc, size_t bytes, hipStream_t s)
  {
    const size_t words = bytes / 4;
    for (size_t i0 = 0; i0 < words; i0 += 768)
    {
      WordChunk ch;
      ch.n = (uint32_t)(words - i0 < 768 ? words - i0 : 768);
      memset(ch.w, 0, sizeof(ch.w));
      memcpy(ch.w, (const uint32_t *)hSrc + i0, (size_t)ch.n * 4);
      hipLaunchKernelGGL(k_set_words, dim3(1), dim3(256), 0, s, (uint32_t *)dDst + i0, ch);
    }
  }

  namespace
  {
    // the image table of a batched encode travels to the device inside kernel arguments (copied at launch: no host buffer has to outlive the call, no blocking copy)
    struct TableChunk { ImageIO e[32]; uint32_t n; };
    static_assert(sizeof(TableChunk) <= 3584, "kernel-argument segment");
    __global__ void k_set_batch_table(ImageIO *dst, const TableChunk chunk)
    {
      const uint32_t *src = reinterpret_cast<const uint32_t *>(chunk.e);
      uint32_t *out = reinterpret_cast<uint32_t *>(dst);
      for (uint32_t i = threadIdx.x; i < chunk.n * (uint32_t)(sizeof(ImageIO) / 4); i += blockDim.x) out[i] = src[i];
    }
  }

  void launch_set_batch_table(ImageIO *dTable, const ImageIO *hTable, size_t count, hipStream_t s)
  {
    for (size_t i0 = 0; i0 < count; i0 += 32)
    {
      TableChunk ch;
      ch.n = (uint32_t)(count - i0 < 32 ? count - i0 : 32);
      for (uint32_t i = 0; i < ch.n; i++) ch.e[i] = hTable[i0 + i];
      for (uint32_t i = ch.n; i < 32; i++) ch.e[i] = ImageIO{};
      hipLaunchKernelGGL(k_set_batch_table, dim3(1), dim3(256), 0, s, dTable + i0, ch);
    }
  }

  void launch_fit_tpb(const EncodeParams &p, int channels, hipStream_t s)
  {
    const uint32_t units = ((p.blocksX + 63u) / 64u) * p.blocksY * p.batchCount;
    with_flags([&](auto rgba, auto FAST, auto DIRECT)
               { hipLaunchKernelGGL((k_fit_tpb<rgba ? 4 : 3, FAST, DIRECT>), dim3((units + tpb_waves<DIRECT>() - 1) / tpb_waves<DIRECT>()), dim3(64 * tpb_waves<DIRECT>()), 0, s, p); },
               channels == 4, p.floatFast != 0, p.vecIn != 0);
  }
}
