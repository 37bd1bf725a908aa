// limg_hip_kernels.hip -- gfx950 kernels of the limg encode hot path.
//
// Path (reference file:line, all relative to the upstream repository):
//   E step (fit_search_strip)   : block gather src/limg.cpp:1899-1905, channel sums :466-497, direction fit + extrema
//                                 src/limg_factorization.h:578-794 (4 ch) / :382-576 (3 ch), colour-error state
//                                 src/limg_internal.h:426-452, per-pixel factors src/limg_factorization.h:98-197, shift search
//                                 src/limg_bit_crush.h:331-392 + :502-666 (accurate mode :668-830) on top of the trial
//                                 src/limg_bit_crush_simd.h:311-810
//   F step (dither_store_strip) : dither src/limg.cpp:824-879 / :799-822 (noise bytes from the context's table), plane stores
//                                 :2004-2093, integer decode src/limg_decode.h:36-236
//   chain position              : the dither chain order of src/limg.cpp:1893,1951-1958 = exclusive prefix of the per-block
//                                 dither-call counts (decoupled look-back in the persistent kernel, k_strip_scan in the split path)
//
// Kernels: k_encode_persistent (one launch per image -- or per list of images of one shape, limg_hip_encode3d_batch_device: the tickets
// then run through the strips of image 0, image 1, ... --: every workgroup loops over work strips, E step of a new strip then the
// F step of the strip it fitted one iteration earlier), k_encode_list_rated (the same loop, limg_hip_persistent_loop.inc, for a list in compact stream mode whose
// images each carry their own error factor: the search's limits per work strip from a device table) and the three-launch split path k_fit_search / k_strip_scan /
// k_dither_store (images with partial edge blocks, whose chain has to be walked on the host; `_perf` mode; A/B testing).
// For images made of whole blocks the float stage (channel sums, direction fit, extrema, record) runs before them as its own
// kernel with one lane per block (k_fit_tpb, limg_hip_fit_tpb.hip; template parameter PREFIT here): the E step then starts from
// the records.  The float-stage code in this file is the lane == pixel form that images with partial edge blocks keep.
//
// Work decomposition: one 256-thread workgroup owns a "work strip" of 32 adjacent 8x8 image blocks (256 x 8 pixels): its
// eight 1 KiB pixel rows are read with 16-byte-per-lane loads into LDS, each of the 4 waves then owns 8 blocks and works
// with lane == pixel (wave64 == 64 pixels == one block) in the E step; per-block control flow (the shift search) is wave-uniform.
// The F step's per-pixel part works with lane == (block of the wave's 8, block row), 8 pixels per lane (phase_f_rows).
//
// Float-stage numerics are those of the reference's SSE4.1 path executed strictly (see DESIGN.md "numerics"):
//   * DPPS summation order (x0y0 + x1y1) + (x2y2 + x3y3), no FMA contraction (built with -ffp-contract=off);
//   * RSQRTPS through the captured 2048-entry table (limg_rsqrt_x86_table.h), read through the vector L1;
//   * the three direction accumulations run in *pixel order*: the per-pixel unit vectors of a batch of 4 blocks are parked in
//     LDS and 16 lanes (4 blocks x 4 channels) each walk one serial 64-term chain -- ~2 instructions per term for 16
//     chains at once instead of a 64-step dependent chain per block;
//   * correctly rounded division (hipcc default), once per batch and lane-parallel; round-to-nearest-even conversions.
//
// This file holds the E step -- its stages finish_block, publish_strip, park_or_store_factors (the ones before them, request_prefit_records / take_prefit_records,
// stage_strip_pixels, phase_e_view, pixel_factors: limg_hip_phase_e.h) and fit_search_strip, which calls them in order around the strip's block queue and keeps the lane == pixel float stage and
// the search's set-up inline --, the split path's scan, the F step
// (dither_store_strip), the kernels and their launchers.  The parts they are built from live in headers, so that all of it stays one
// translation unit under this file's compile flags:
//   limg_hip_phase_e.h     the E step's LDS layout and its stages from the record load to the per-pixel factors (also included by limg_hip_rate.hip)
//   limg_hip_search.h      the packed trial, the two search automata, the generic-path search
//   limg_hip_phase_f.h     the F step's parts: LDS areas, the factor-plane copy, preparation, plane stores, the rows / pixels phases, first dither calls
//   limg_hip_float_pixel.h the E step's view of its strip (EStrip), the per-block LDS state, and the lane == pixel float stage's direction sums (serial_sums2)
//   limg_hip_lookback.h    the decoupled look-back over the per-strip dither-call counts
// The dither chain partition (which chain a block row belongs to, which row heads it) is chain_of_row / chain_head_row in limg_hip_internal.h, shared with the host.
#include "limg_hip_phase_e.h"
#include "limg_hip_lookback.h"

namespace limg_hip
{
  namespace
  {
    constexpr int kPrioE = 2; // wave priority of the persistent kernel's E step (s_setprio)

    // =====================================================================================================================
    // kernel 1: fit + factors + shift search
    // =====================================================================================================================
    // (the LDS layout of an E task and the stages request_prefit_records .. pixel_factors: limg_hip_phase_e.h, shared with the stream's size probe)

    // E: block epilogue -- the block's dither calls and payload words into the wave's counter, its shift word to the park slot / the raster-order array, its
    // factor bytes to the staging area ([3 planes][8 rows][256 px] at the F step's strides)
    template <int CH, bool PERSIST, class P>
    __device__ __forceinline__ void finish_block(const P &p, const EStrip g, const uint32_t sb, const uint32_t bx, const BlkF *blkE, const uint32_t shift[3], const uint32_t fA,
                                                 const uint32_t fB, const uint32_t fC, const bool active, const uint32_t o, uint8_t *park, uint8_t *stage, uint32_t &waveCalls)
    {
      // dither calls this block will make (src/limg.cpp:1951-1958)
      // a shift of 1..7 dithers (one call), 0 and 8 do not; as scalar arithmetic -- ((s & 7) + 7) >> 3 -- because a boolean would go through a lane mask and a vector select
      const uint32_t calls = (((shift[0] & 7u) + 7u) >> 3) + (((shift[1] & 7u) + 7u) >> 3) + (((shift[2] & 7u) + 7u) >> 3);
      waveCalls += calls;
      if (p.stripWords)
      { // stream mode: the block's payload size in 8-byte words rides in bits 8.. of the same per-wave counter (calls of a strip stay below 256): a field of 8 - shift
        // bits per pixel is that many words; a factor at shift 8 has none unless its alpha normal is non-zero (raw-byte escape, limg_hip_stream.hip)
        uint32_t words = 0;
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
          const uint32_t sk = shift[k];
          if (sk < 8u) words += 8u - sk;
          else if (CH == 4 && sgpr((int)blkE->rec[8 * k + 3]) != sgpr((int)blkE->rec[8 * k + 7])) words += 8u;
        }
        waveCalls += words << 8;
      }

      const uint32_t word = shift[0] | (shift[1] << 8) | (shift[2] << 16) | (calls << 24);
      if (g.lane == 0)
      {
        if (!PERSIST) p.shifts[(size_t)g.byS * p.blocksX + bx] = word;
        else
        {
          if (p.compactOut)
          { // (the row's first index is worked out here, where it is stored to: hoisted out of the block loop its two words would sit in VGPR lanes across the search)
            uint32_t byS = g.byS;
            asm volatile("" : "+s"(byS));
            p.shifts[(size_t)byS * p.blocksX + bx] = word;
          }
          reinterpret_cast<uint32_t *>(park + kParkShift)[sb] = word;
        }
      }
      if (p.storePlanes && active) { stage[o] = (uint8_t)fA; stage[kFacPlane + o] = (uint8_t)fB; stage[2 * kFacPlane + o] = (uint8_t)fC; }
    }

    // E: strip epilogue, the strip's dither-call count (thread 0, behind the barrier that follows the block loop): to the look-back descriptor or to k_strip_scan
    template <bool PERSIST, class P>
    __device__ __forceinline__ void publish_strip(const P &p, const EStrip g, const uint32_t id, const uint32_t head0)
    {
      const uint32_t aggAll = g.calls[0] + g.calls[1] + g.calls[2] + g.calls[3];
      const uint32_t agg = aggAll & 0xFFu; // (bits 8..: the strip's payload words, stream mode)
      if (p.stripWords) p.stripWords[id] = aggAll >> 8;
      if (PERSIST)
      { // publish the count; if the predecessor's inclusive count is already there, publish ours as inclusive right away
        const uint32_t headId = head0 + chain_head_row(p.chainCount, p.chainRows, g.by) * p.stripsX;
#ifdef LIMG_HIP_TEST_HOOKS
        if (id == p.testSkipStrip) {} // (test build: a strip that never publishes)
        else
#endif
        if (id == headId) desc_store(p.desc + id, kDescInclusive, agg);
        else
        {
          const unsigned long long d = desc_load(p.desc + id - 1);
          if ((uint32_t)(d >> 32) == kDescInclusive) desc_store(p.desc + id, kDescInclusive, (uint32_t)d == kBasePoison ? kBasePoison : (uint32_t)d + agg);
          else desc_store(p.desc + id, kDescAggregate, agg);
        }
      }
      else p.stripCalls[id] = agg;
    }

    // E: strip epilogue, the strip's pre-dither factor bytes: parked (persistent kernel: private, L2-resident scratch; same workgroup reads them back) or stored to
    // the caller's factor planes (split path: rewritten in place by k_dither_store)
    template <bool PERSIST, class P, class IO>
    __device__ __forceinline__ void park_or_store_factors(const P &p, const IO &io, const EStrip g, uint8_t *park, uint8_t *stage)
    {
      if (PERSIST)
        for (int i = g.tid; i < 384; i += kThreads) reinterpret_cast<uint4 *>(park + kParkFac)[i] = *reinterpret_cast<const uint4 *>(stage + (i >> 4) * kFacRow + (i & 15) * 16); // 24 rows of 256 bytes
      else if (p.storePlanes) copy_factor_planes<true>(p, io, stage, g.x0, g.y0, g.stripW, g.ry, g.tid);
    }

    // the parameter block behind a pointer the compiler cannot follow (persistent kernels: p lies in the kernel-argument segment or a device table): what is read
    // through the result is fetched again, with scalar loads, instead of being kept from an earlier read
    template <class P>
    __device__ __forceinline__ const P &reread_params(const P &p)
    {
      const P *q = &p;
      asm volatile("" : "+s"(q));
      return *q;
    }

    // PREFIT: the float stage already ran in k_fit_tpb (limg_hip_fit_tpb.hip, one lane per block); this step loads the records and goes on with phase E.
    // id: the strip's number in ticket / look-back order (all images of a batch); local: its number inside its image (geometry); rowBase: the image's first
    // block row in the per-block scratch arrays; head0: the id of the image's first strip
    // ACC: the accurate search (fastBitCrushing == false) instead of the default one -- a kernel variant of its own, so that neither search's registers and code
    // weigh on the other
    // lim: where the search's limits (maxPixel32, blockLimitFull, maxBlock, crushBits) come from -- `p` itself, or the image's entry of a threshold table (k_encode_list_rated)
    // Two parts stay INLINE here, measured (profiles/e_step_stages_ab.md): as functions of their own (float_stage_pixel, search_block) the lane == pixel float stage and
    // the search's set-up left the persistent kernel's lane == pixel instances with 11-46 more spilled SGPRs and 1.1-1.8 KB more code, `--legacy-float-stage` 5.3 %
    // slower, and four k_fit_search instances with 2-4 more VGPRs; either one alone as a function does the same.
    template <int CH, bool PERSIST, bool FAST, bool PREFIT, bool ACC, bool NOSEL, class P, class LIM, class IO>
    __device__ __forceinline__ void fit_search_strip(const P &p, const LIM &lim, const IO &io, const uint32_t id, const uint32_t local, const uint32_t rowBase, const uint32_t head0, uint8_t *lds,
                                                     uint8_t *park, const int tid)
    {
      constexpr LdsLayout LL = lds_layout<PREFIT>();
      EStrip g;
      g.tid = tid; g.lane = tid & 63; g.wave = tid >> 6;
      g.strip = local % p.stripsX; g.by = local / p.stripsX; g.byS = rowBase + g.by;
      g.x0 = g.strip * (kStripBlocks * kBlock); g.y0 = g.by * kBlock;
      g.stripW = min(p.sizeX - g.x0, (uint32_t)(kStripBlocks * kBlock)); g.ry = min(p.sizeY - g.y0, (uint32_t)kBlock);
      g.pix = reinterpret_cast<uint32_t *>(lds + kLdsStrip); g.V = reinterpret_cast<float *>(lds + LL.v); g.blk = reinterpret_cast<BlkF *>(lds + LL.blk);
      g.calls = reinterpret_cast<uint32_t *>(lds + LL.calls); g.trialc = reinterpret_cast<int *>(lds + LL.trialc);
      const int lane = g.lane;

      uint32_t recVal[2] = { 0u, 0u };
      if (PREFIT) request_prefit_records(p, g, recVal);
      stage_strip_pixels(p, io, g);
      __syncthreads();
      if (PREFIT) take_prefit_records<PERSIST>(p, g, recVal, park);
      else
      { // the lane == pixel float stage (a4-a6), inline: see the note above this function
      // the 4 KiB RSQRTPS table is read straight from global memory (it lives in the CU's vector L1): keeping a copy in LDS would
      // cost the fifth workgroup per CU
      const unsigned short *s_rsq = d_rsqrt_x86_tab;
      const int lane = g.lane, wave = g.wave;
      const uint32_t strip = g.strip, by = g.by, byS = g.byS;
      float *V = g.V + wave * kBatch * kVDw;
      BlkF *blk = g.blk + wave * kBlocksPerWave;
      auto geom = [&](int b, uint32_t &rx, uint32_t &n) -> bool { return block_geom(p, g, wave * kBlocksPerWave + b, rx, n); }; // per-block geometry (wave-uniform)

      // The float stage runs in batches of kBatch blocks per wave: the parked contributions of one batch are what limits the
      // workgroups per CU (LDS), and 4 blocks x 4 waves keep it at 5 workgroups per CU.
      // Per-block values of the batch stay in registers across the phases (the loops over i are fully unrolled).
#pragma unroll 1
      for (int h = 0; h < kBlocksPerWave / kBatch; h++)
      {
      uint32_t px8[kBatch];
      V4 est8[kBatch];
      BlkF *const blkh = blk + h * kBatch;

      // ---- phase A: sums, average, first direction pass (a4, a5/a6 pass 1) ------------------------------------------
#pragma unroll
      for (int i = 0; i < kBatch; i++)
      {
        const int b = h * kBatch + i;
        uint32_t rx, n;
        px8[i] = 0;
        est8[i].a = float2_t{ 0.0f, 0.0f }; est8[i].b = float2_t{ 0.0f, 0.0f };
        if (!geom(b, rx, n))
        {
          if (lane == 0) { blk[b].flags = 0; blk[b].n = 0; blk[b].inv_count = 0.0f; }
          continue;
        }
        const uint32_t sb = wave * kBlocksPerWave + b;
        uint32_t lx, ly;
        const uint32_t px = block_pixel(g, sb, rx, n, lx, ly);
        px8[i] = px;
        const V4 pf = px_to_v4(px);
        uint32_t pxs = px;
        if (n < 4)
        { // Upstream's SIMD sum loop consumes at least 4 pixels (src/limg.cpp:478-487): a block of fewer than 4 also sums what the previous block of its
          // strip left at positions n..3 of the gather buffer (:1890, :1899-1905).  Only the bottom-right corner block can be that small; the previous
          // block in raster order is its left neighbour, or the last block of the row above for a one-block-wide image.  The first block of a strip
          // has no predecessor (uninitialised stack upstream): nothing is added then.
          const uint32_t bxx = strip * kStripBlocks + sb;
          const bool hasPrev = bxx > 0 || by > chain_head_row(p.chainCount, p.chainRows, by);
          if (hasPrev && (uint32_t)lane >= n && lane < 4)
          {
            const uint32_t pbx = bxx > 0 ? bxx - 1 : p.blocksX - 1, pby = bxx > 0 ? by : by - 1;
            const uint32_t prx = min(p.sizeX - pbx * kBlock, (uint32_t)kBlock);
            const uint32_t row = (uint32_t)lane / prx, col = (uint32_t)lane - row * prx; // gather index -> position inside the previous block
            pxs = io.in[(size_t)(pby * kBlock + row) * p.sizeX + pbx * kBlock + col];
          }
        }
        const uint32_t s02 = wave_sum(pxs & 0x00FF00FFu), s13 = wave_sum((pxs >> 8) & 0x00FF00FFu);
        float inv_count = 0.015625f;
        if (n != 64) inv_count = 1.0f / (float)n;
        V4 avg;
        avg.a = float2_t{ (float)(int)(s02 & 0xFFFF), (float)(int)(s02 >> 16) } * inv_count;
        avg.b = float2_t{ (float)(int)(s13 & 0xFFFF), CH == 4 ? (float)(int)(s13 >> 16) : 0.0f } * inv_count;
        V4 d = pf - avg;
        mask_alpha<CH>(d);
        st4(V + i * kVDw + lane * 4, unit4<CH, FAST>(s_rsq, d, (uint32_t)lane < n));
        if (lane == 0)
        {
          st4(blk[b].avg, avg);
          *reinterpret_cast<float4 *>(blk[b].dirB) = make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4 *>(blk[b].dirC) = make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4 *>(blk[b].est0) = make_float4(0.f, 0.f, 0.f, 0.f);
          *reinterpret_cast<float4 *>(blk[b].mm) = make_float4(0.f, 0.f, 0.f, 0.f);
          blk[b].mm[4] = 0.0f; blk[b].mm[5] = 0.0f;
          blk[b].inv_count = inv_count; blk[b].n = n; blk[b].flags = kValid;
        }
      }
      serial_sums2<CH, kDirA, FAST>(V, blkh, lane);

      // ---- phase B: factor A extrema, residual -> second direction (pass 2) --------------------------------------------
      {
        static_assert(kBatch == 4, "wave_reduce4_min_max");
        float mnv[kBatch], mxv[kBatch];
        bool did[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++)
        {
          const int b = h * kBatch + i;
          uint32_t rx, n;
          did[i] = false; mnv[i] = 0.0f; mxv[i] = 0.0f;
          if (!geom(b, rx, n)) continue;
          if ((uint32_t)sgpr((int)blk[b].flags) & kZeroA) continue;
          did[i] = true;
          const V4 dirA = ld4(blk[b].dirA), avg = ld4(blk[b].avg);
          const float invA = blk[b].invA;
          const V4 pf = px_to_v4(px8[i]);
          const bool active = (uint32_t)lane < n;
          const float fA = dp4<CH, FAST>(pf - avg, dirA) * invA;
          mnv[i] = active ? fA : 0.0f; mxv[i] = mnv[i]; // min / max start at 0 upstream (src/limg_factorization.h:633-634)
          est8[i] = avg + dirA * fA;
          V4 e = pf - est8[i];
          mask_alpha<CH>(e);
          st4(V + i * kVDw + lane * 4, unit4<CH, FAST>(s_rsq, e, active));
        }
        wave_reduce4_min_max(mnv, mxv);
#pragma unroll
        for (int i = 0; i < kBatch; i++)
          if (did[i] && lane == 0) { blk[h * kBatch + i].mm[0] = vmin(mnv[i], 0.0f); blk[h * kBatch + i].mm[1] = vmax(mxv[i], 0.0f); }
      }
      serial_sums2<CH, kDirB, FAST>(V, blkh, lane);

      // ---- phase C: factor B (and, 3 ch, C) extrema; 4 ch: residual -> third direction (pass 3) ---------------------
      float mnCv[kBatch], mxCv[kBatch];
      bool didC[kBatch];
#pragma unroll
      for (int i = 0; i < kBatch; i++) { didC[i] = false; mnCv[i] = FLT_MAX; mxCv[i] = -FLT_MAX; }
#pragma unroll
      for (int i = 0; i < kBatch; i++)
      {
        const int b = h * kBatch + i;
        uint32_t rx, n;
        if (!geom(b, rx, n)) continue;
        if ((uint32_t)sgpr((int)blk[b].flags) & kZeroB) continue; // 1/0 = inf => every fB is NaN upstream => B and C collapse to 0
        const V4 dirB = ld4(blk[b].dirB);
        const float invB = blk[b].invB;
        const V4 pf = px_to_v4(px8[i]);
        const bool active = (uint32_t)lane < n;
        const float fB = dp4<CH, FAST>(pf - est8[i], dirB) * invB;
        float mnB = active ? fB : FLT_MAX, mxB = active ? fB : -FLT_MAX;
        if (CH == 4)
        {
          didC[i] = true; mnCv[i] = mnB; mxCv[i] = mxB; // reduced for the whole batch after the loop
          est8[i] = est8[i] + dirB * fB;
          st4(V + i * kVDw + lane * 4, unit4<CH, FAST>(s_rsq, pf - est8[i], active));
          if (lane == 0) st4(blk[b].est0, est8[i]);
        }
        else
        {
          // dirC = dirA x dirB (src/limg_factorization.h:498-507); slots: a = (x0, x2), b = (x1, x3)
          const V4 dirA = ld4(blk[b].dirA);
          V4 dirC;
          dirC.a.x = dirA.b.x * dirB.a.y - dirA.a.y * dirB.b.x; // A1 B2 - A2 B1
          dirC.b.x = dirA.a.y * dirB.a.x - dirA.a.x * dirB.a.y; // A2 B0 - A0 B2
          dirC.a.y = dirA.a.x * dirB.b.x - dirA.b.x * dirB.a.x; // A0 B1 - A1 B0
          dirC.b.y = 0.0f;
          const bool zeroC = sgpr((dirC.a.x == 0.0f && dirC.b.x == 0.0f && dirC.a.y == 0.0f) ? 1 : 0) != 0;
          float mnC = 0.0f, mxC = 0.0f;
          if (!zeroC)
          {
            const float invC = FAST ? __builtin_amdgcn_rcpf(dp4<CH, FAST>(dirC, dirC)) : 1.0f / dp4<CH, FAST>(dirC, dirC);
            const V4 e = pf - (est8[i] + dirB * fB);
            const float fC = dp4<CH, FAST>(e, dirC) * invC;
            mnC = active ? fC : FLT_MAX; mxC = active ? fC : -FLT_MAX;
            wave_min_max(mnB, mxB);
            wave_min_max(mnC, mxC);
          }
          else
            wave_min_max(mnB, mxB);
          if (lane == 0)
          {
            blk[b].mm[2] = mnB; blk[b].mm[3] = mxB; blk[b].mm[4] = mnC; blk[b].mm[5] = mxC;
            st4(blk[b].dirC, dirC);
            if (zeroC) blk[b].flags |= kZeroC;
          }
        }
      }
      if (CH == 4)
      {
        wave_reduce4_min_max(mnCv, mxCv);
#pragma unroll
        for (int i = 0; i < kBatch; i++)
          if (didC[i] && lane == 0) { blk[h * kBatch + i].mm[2] = mnCv[i]; blk[h * kBatch + i].mm[3] = mxCv[i]; }
        // blocks that skipped phase C left stale pass-2 contributions in V; their dirC is never used (flags)
        serial_sums2<CH, kDirC, FAST>(V, blkh, lane);
        // ---- phase D: factor C extrema (pass 4).  Upstream never advances its estimate pointer in this loop
        //      (src/limg_factorization.h:748-758), so every pixel is measured against pixel 0's A+B estimate.
        float mnDv[kBatch], mxDv[kBatch];
        bool didD[kBatch];
#pragma unroll
        for (int i = 0; i < kBatch; i++)
        {
          const int b = h * kBatch + i;
          uint32_t rx, n;
          didD[i] = false; mnDv[i] = FLT_MAX; mxDv[i] = -FLT_MAX;
          if (!geom(b, rx, n)) continue;
          if ((uint32_t)sgpr((int)blk[b].flags) & kZeroC) continue;
          didD[i] = true;
          const V4 dirC = ld4(blk[b].dirC), est0 = ld4(blk[b].est0);
          const float invC = blk[b].invC;
          const V4 pf = px_to_v4(px8[i]);
          const bool active = (uint32_t)lane < n;
          const float fC = dp4<CH, FAST>(pf - est0, dirC) * invC;
          mnDv[i] = active ? fC : FLT_MAX; mxDv[i] = active ? fC : -FLT_MAX;
        }
        wave_reduce4_min_max(mnDv, mxDv);
#pragma unroll
        for (int i = 0; i < kBatch; i++)
          if (didD[i] && lane == 0) { blk[h * kBatch + i].mm[4] = mnDv[i]; blk[h * kBatch + i].mm[5] = mxDv[i]; }
      }
      } // batches
      wave_lds_fence();

      // ---- records (src/limg_factorization.h:764-790): 8 lanes per block, 3 values per lane --------------------------
      {
        const int b = lane >> 3, j = lane & 7;
        const uint32_t flags = blk[b].flags;
        uint32_t big = 0;
#pragma unroll
        for (int r = 0; r < 3; r++)
        {
          const int kc = j + 8 * r, k = kc >> 2, c = kc & 3; // k = 2 r + (j >> 2): A for r == 0, B for r == 1, C for r == 2
          const float *dir = r == 0 ? blk[b].dirA : (r == 1 ? blk[b].dirB : blk[b].dirC);
          const int sl = slot_of(c);
          float m = blk[b].mm[k], dv = dir[sl];
          const bool dead = (r == 2 && (flags & kZeroC)) || (r >= 1 && (flags & kZeroB)) || (flags & kZeroA);
          if (dead) { m = 0.0f; dv = 0.0f; }
          float val = m * dv;
          if (r == 0) val = blk[b].avg[sl] + val;
          int q = cvt_rne(val);
          if ((CH == 3 && c == 3) || !(flags & kValid)) q = 0;
          big |= (q > p.recordLimit || q < -p.recordLimit) ? 1u : 0u;
          blk[b].rec[kc] = (int16_t)q;
        }
        big |= (uint32_t)dpp<0xB1, 0xF>(0, (int)big);
        big |= (uint32_t)dpp<0x4E, 0xF>(0, (int)big);
        big |= (uint32_t)dpp<0x141, 0xF>(0, (int)big);
        if (j == 0 && big) blk[b].flags = flags | kBig;
      }
      wave_lds_fence();
      // record -> global (16 dwords per block: avg, then the 24 int16); persistent kernel: the int16 part is parked
      {
#pragma unroll
        for (int r = 0; r < 2; r++)
        {
          const int b = r * 4 + (lane >> 4), w = lane & 15;
          const uint32_t sb = wave * kBlocksPerWave + b, bx = strip * kStripBlocks + sb;
          const uint32_t val = w < 4 ? __float_as_uint(blk[b].avg[slot_of(w)]) : reinterpret_cast<const uint32_t *>(blk[b].rec)[w - 4];
          if (bx < p.blocksX && (!PERSIST || p.compactOut)) reinterpret_cast<uint32_t *>(p.records + (size_t)byS * p.blocksX + bx)[w] = val;
          if (PERSIST && w >= 4) reinterpret_cast<uint32_t *>(park + kParkRec)[sb * 12 + (w - 4)] = val;
        }
      }
    
      }
      if (!PERSIST && p.fitOnly) return; // pass 1 of the merged-block encoder: the records are all it needs (uniform for the workgroup)
      phase_e_view<CH, FAST, PREFIT>(g);
      uint32_t *s_queue = g.calls + 4;
      if (tid == 0) *s_queue = 0;
      __syncthreads(); // all waves are done with V: wave 0's V region becomes the factor-byte staging area

      uint8_t *stage = reinterpret_cast<uint8_t *>(g.V); // [3 planes][8 rows][256 px]
      if (PERSIST)
      { // from here on the park slot is known by ONE address, the one the block loop stores its shift words to: the strip's epilogue goes back from it, instead of
        // the slot's base and the offsets it was made of staying live across the search
        park += kParkShift;
        asm volatile("" : "+s"(park));
        park -= kParkShift;
      }
      uint32_t waveCalls = 0;
      // (No zeroing of the parked shift words of blocks past the right edge here: with the dynamic queue below another wave may already have parked a real
      //  word for a block of this wave's range by the time this wave gets to issue such a store -- a rare lost update, found in round 2.  The F step masks
      //  the words of blocks that do not exist instead.)

      // ---- phase E: per-pixel factors (a8) + shift search (a10-a12) ----------------------------------------------------
      // The strip's 32 blocks are handed out dynamically: the number of trials differs from block to block (2 .. 20), and with a fixed 8 blocks per wave
      // the fastest wave would idle at the next barrier.  Everything phase E touches of a block lives in LDS and is indexed by the block, not the wave.
      auto grab = [&]() -> uint32_t { uint32_t v = 0; if (lane == 0) v = atomicAdd(s_queue, 1u); return (uint32_t)sgpr((int)v); };
      uint32_t sbNext = grab();
#pragma unroll 1
      for (;;)
      {
        const uint32_t sb = sbNext;
        if (sb >= (uint32_t)kStripBlocks) break;
        uint32_t qv = 0;
        if (lane == 0) qv = atomicAdd(s_queue, 1u); // the next block's index arrives while this one is searched
        // (the persistent kernels run images of whole blocks only -- encode_plan: fused => !ragged --: a block that exists there has its 64 pixels, and the search's
        //  form for blocks with masked lanes is not instantiated)
        uint32_t rx = kBlock, n = kBlock * kBlock, lx, ly;
        if (PERSIST ? g.strip * kStripBlocks + sb >= p.blocksX : !block_geom(p, g, sb, rx, n)) { sbNext = (uint32_t)sgpr((int)qv); continue; }
        const BlkF *const blkE = g.blk + sb;
        const bool active = (uint32_t)lane < n;
        const uint32_t px = block_pixel(g, sb, rx, n, lx, ly);
        uint32_t fA, fB, fC, shift[3] = { 0, 0, 0 };
        pixel_factors<CH, FAST>(reinterpret_cast<const BlkE *>(blkE), px, fA, fB, fC);
        // the shift search of the block (a10-a12), inline (see the note above this function): limits, the packed trial's state, then one of the two automata or, for a
        // record out of the packed trial's range, the generic search
        if (p.forced[0] >= 0) { shift[0] = (uint32_t)p.forced[0]; shift[1] = (uint32_t)p.forced[1]; shift[2] = (uint32_t)p.forced[2]; }
        else if (lim.crushBits)
        {
          // be * 16 < maxBlock * n  <=>  be < ceil(maxBlock * n / 16); clamped to 32 bits (be itself never gets near 2^32).  Full blocks: from the host.
          uint32_t blockLimit = lim.blockLimitFull;
          if (n != 64)
          {
            const uint64_t lim64 = (lim.maxBlock * (uint64_t)n + 15ull) >> 4;
            blockLimit = (uint32_t)sgpr((int)(lim64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)lim64));
          }
          const bool big = ((uint32_t)sgpr((int)blkE->flags) & kBig) != 0;
          if (!big)
          {
            TrialState t;
            t.fA = fA; t.fB = fB; t.fC = fC;
            const uint32_t R = px & 0xFF, G = (px >> 8) & 0xFF;
            t.hiRG = (R + 0x8000u) | ((G + 0x8000u) << 16);
            t.loRG = (R + 0x8000u - 255u) | ((G + 0x8000u - 255u) << 16);
            t.pxB = (int)((px >> 16) & 0xFF);
            t.pxBlo = t.pxB - 255;
            if (PREFIT)
            { // uniform values, kept in VGPRs (they are operands of v_mad_i32_i24); prepared lane-parallel with the phase-E view above
              const int *tc = g.trialc + sb * kTrialConstDw;
#pragma unroll
              for (int c = 0; c < 3; c++)
              {
                t.nA[c] = tc[c]; t.nB[c] = tc[3 + c]; t.nC[c] = tc[6 + c];
                t.mA[c] = tc[9 + c]; t.mB[c] = tc[12 + c]; t.mC[c] = tc[15 + c];
              }
            }
            else
            { // lane == pixel float stage: no LDS left over for the table (other waves' parked contributions are still live when this wave gets here)
#pragma unroll
              for (int c = 0; c < 3; c++)
              {
                const int loA = blkE->rec[c], hiA = blkE->rec[4 + c], loB = blkE->rec[8 + c], hiB = blkE->rec[12 + c], loC = blkE->rec[16 + c], hiC = blkE->rec[20 + c];
                t.nA[c] = loA - hiA; t.nB[c] = loB - hiB; t.nC[c] = loC - hiC;
                t.mA[c] = term_const(0, c, loA); t.mB[c] = term_const(1, c, loB); t.mC[c] = term_const(2, c, loC);
              }
            }
            // per pixel: factor A's (negated) terms become  channel - term, so the three terms of a channel sum to  channel - estimate
            t.mA[0] += (int)(R << 8); t.mA[1] += (int)(G << 8); t.mA[2] += t.pxB << 8;
            // (the flag goes through an opaque scalar: hoisted out of the block loop as a boolean it comes back as a lane mask that is negated with two vector
            //  instructions per block)
            if (!ACC)
            {
              if (n == 64) search_fast_automaton<true, NOSEL>(t, true, lim.maxPixel32, blockLimit, shift);
              else search_fast_automaton<false, NOSEL>(t, active, lim.maxPixel32, blockLimit, shift);
            }
            else
            {
              if (n == 64) search_accurate_automaton<true, NOSEL>(t, true, lim.maxPixel32, blockLimit, p.accTable, shift);
              else search_accurate_automaton<false, NOSEL>(t, active, lim.maxPixel32, blockLimit, p.accTable, shift);
            }
          }
          else
          {
            // out-of-range record (never produced by a fit of byte pixels; kept so that no input can break exactness):
            // generic 32-bit trial, deliberately a real call so that none of it is speculated into the common path
            // (persistent kernels: the block limit is fetched here, where this rare path needs it, not held across every block's search)
            const uint64_t maxBlockN = (PERSIST ? reread_params(lim).maxBlock : lim.maxBlock) * (uint64_t)n;
            const uint32_t packed = (uint32_t)sgpr((int)search_generic(px, fA, fB, fC, blkE->rec, active, lim.maxPixel32, maxBlockN, !ACC)); // uniform: keeps the shift triple (and the bookkeeping below) on the scalar unit for the common path too
            shift[0] = packed & 0xFF; shift[1] = (packed >> 8) & 0xFF; shift[2] = (packed >> 16) & 0xFF;
          }
        }
    
        finish_block<CH, PERSIST>(p, g, sb, g.strip * kStripBlocks + sb, blkE, shift, fA, fB, fC, active, ly * kFacRow + sb * kBlock + lx, park, stage, waveCalls);
        sbNext = (uint32_t)sgpr((int)qv);
      }
      if (lane == 0) g.calls[g.wave] = waveCalls;
      __syncthreads();
      if (PERSIST)
      { // The strip's epilogue starts over from the parameter block, the thread id and the strip's block row: what the set-up above worked out of them (fields of
        // p, lane masks, addresses) would otherwise stay live across the block loop, where the search leaves no scalar register free, and be parked in VGPR lanes.
        const P &ps = reread_params(p);
        EStrip ge = g;
        asm volatile("" : "+v"(ge.tid));
        asm volatile("" : "+s"(ge.by));
        if (ge.tid == 0) publish_strip<true>(ps, ge, id, head0);
        park_or_store_factors<true>(ps, io, ge, park, stage);
        return;
      }
      if (tid == 0) publish_strip<PERSIST>(p, g, id, head0);
      park_or_store_factors<PERSIST>(p, io, g, park, stage);
    }

    // =====================================================================================================================
    // kernel 2: exclusive scan of the per-strip dither-call counts in raster order, restarting at every chain boundary
    // =====================================================================================================================
    __global__ __launch_bounds__(1024) void k_strip_scan(const EncodeParams p)
    {
      __shared__ uint32_t s_sum[1024];
      __shared__ uint32_t s_flag[1024];
      const uint32_t total = p.blocksY * p.stripsX;
      const uint32_t per = (total + 1023u) / 1024u;
      const uint32_t t = threadIdx.x;
      const uint32_t begin = min(t * per, total), end = min(begin + per, total);
      auto chain_of = [&](uint32_t e) -> uint32_t { return chain_of_row(p.chainCount, p.chainRows, e / p.stripsX); };
      auto is_head = [&](uint32_t e) -> bool { return e == 0 || chain_of(e) != chain_of(e - 1); };

      uint32_t sum = 0, flag = 0;
      for (uint32_t e = begin; e < end; e++)
      {
        if (is_head(e)) { sum = 0; flag = 1; }
        sum += p.stripCalls[e];
      }
      s_sum[t] = sum; s_flag[t] = flag;
      __syncthreads();
      // segmented inclusive scan (Hillis-Steele) over the 1024 partials
      for (uint32_t off = 1; off < 1024; off <<= 1)
      {
        uint32_t vs = s_sum[t], vf = s_flag[t];
        if (t >= off && !vf) { vs += s_sum[t - off]; vf = s_flag[t - off]; }
        __syncthreads();
        s_sum[t] = vs; s_flag[t] = vf;
        __syncthreads();
      }
      uint32_t run = (t == 0) ? 0u : s_sum[t - 1]; // calls in the current chain before this thread's chunk
      for (uint32_t e = begin; e < end; e++)
      {
        if (is_head(e)) run = 0;
        p.stripBase[e] = run;
        run += p.stripCalls[e];
      }
      // cross-GPU single chain (limg_hip_encode3d_chain_device): the dither calls of this whole image strip, for the exchange between the E and the F step
      if (p.chainCallsOut && end == total && begin < end) *p.chainCallsOut = run;
    }

    // =====================================================================================================================
    // kernel 3 (split path): phase F as its own launch
    // =====================================================================================================================
    // F task: dither + stores + decode of one work strip from the parked per-block results.
    // PERSIST == false: the strip's chain position comes from k_strip_scan (p.stripBase);
    // PERSIST == true : from the look-back over the descriptors, and the strip's inclusive count is published first thing.
    static_assert(kPhaseFBytes + kStripBlocks * 48 <= kLdsTotal - kLdsStrip - 16, "the F step's LDS overlays the E step's");

    template <int CH, bool PERSIST, class P, class IO>
    __device__ __forceinline__ void dither_store_strip(const P &p, const IO &io, const uint32_t id, const uint32_t local, const uint32_t rowBase, const uint32_t head0, uint8_t *fbase,
                                                       const uint8_t *park, const int tid)
    {
      int16_t *s_rec = reinterpret_cast<int16_t *>(fbase + kPhaseFBytes); // [32][24]
      const int lane = tid & 63, wave = tid >> 6;
      const uint32_t strip = local % p.stripsX, by = local / p.stripsX;
      const uint32_t byS = rowBase + by;
      const uint32_t x0 = strip * (kStripBlocks * kBlock), y0 = by * kBlock;
      const uint32_t stripW = min(p.sizeX - x0, (uint32_t)(kStripBlocks * kBlock));
      const uint32_t ry = min(p.sizeY - y0, (uint32_t)kBlock);
      const uint32_t nBlocks = min(p.blocksX - strip * kStripBlocks, (uint32_t)kStripBlocks);
      const StripLds L = carve_phase_f(fbase, s_rec, 24);

      if (PERSIST)
      {
        // (rolled on purpose: unrolled, the second loop became 19 dword loads and ~100 vector instructions of address arithmetic per wave; its 384 dwords go as 96 16-byte pieces)
        static_assert(kStripBlocks * 12 * 4 == 96 * 16, "record copy");
#pragma unroll 1
        for (int i = tid; i < 384; i += kThreads) *reinterpret_cast<uint4 *>(L.fac + (i >> 4) * kFacRow + (i & 15) * 16) = reinterpret_cast<const uint4 *>(park + kParkFac)[i];
        if (tid < 96) reinterpret_cast<uint4 *>(s_rec)[tid] = reinterpret_cast<const uint4 *>(park + kParkRec)[tid];
        if (tid < kStripBlocks) L.shift[tid] = (uint32_t)tid < nBlocks ? reinterpret_cast<const uint32_t *>(park + kParkShift)[tid] : 0u; // nothing is parked for blocks past the right edge
      }
      else
      {
        copy_factor_planes<false>(p, io, L.fac, x0, y0, stripW, ry, tid);
        // records (12 dwords of int16 per block) and shift words
        for (int i = tid; i < kStripBlocks * 12; i += kThreads)
        {
          const int sb = i / 12, w = i - sb * 12;
          uint32_t v = 0;
          if ((uint32_t)sb < nBlocks) v = reinterpret_cast<const uint32_t *>(p.records + (size_t)byS * p.blocksX + strip * kStripBlocks + sb)[4 + w];
          reinterpret_cast<uint32_t *>(s_rec + sb * 24)[w] = v;
        }
        if (tid < kStripBlocks) L.shift[tid] = (uint32_t)tid < nBlocks ? p.shifts[(size_t)byS * p.blocksX + strip * kStripBlocks + tid] : 0u;
      }
      __syncthreads();
      phase_f_prepare<CH>(L, lane, wave, p.recordLimit);
      wave_lds_fence();
      // strips of whole blocks (always in the persistent kernel; in the split path unless the image has partial edge blocks): the uniform planes' stores run inside
      // phase_f_rows, behind its noise loads; otherwise here
      const bool rowsPath = PERSIST || (p.sizeX % kBlock == 0 && ry == (uint32_t)kBlock);
      // the uniform planes (base-independent: 28 of the 35 output bytes per pixel): rows 0..3 here, beside wave 0's look-back; rows 4..7 behind the noise loads
      if (p.fullPlanes) phase_f_store_const(p, io, L, x0, y0, ry, lane, wave, rowsPath ? 1u : 3u);
      if (wave == 0)
      {
        uint32_t base;
        if (PERSIST)
        {
          const uint32_t headId = head0 + chain_head_row(p.chainCount, p.chainRows, by) * p.stripsX;
          const uint32_t w = lane < kStripBlocks ? L.shift[lane] : 0u;
          const uint32_t agg = wave_sum(w >> 24);
          const unsigned long long own = desc_load(p.desc + id);
          if ((uint32_t)(own >> 32) == kDescInclusive) base = (uint32_t)sgpr((int)((uint32_t)own == kBasePoison ? kBasePoison : (uint32_t)own - agg));
          else
          {
            base = lookback_base(p, id, headId, agg, lane);
            if (lane == 0 && publishes(p, id)) desc_store(p.desc + id, kDescInclusive, base == kBasePoison ? kBasePoison : base + agg);
          }
#ifdef LIMG_HIP_TEST_HOOKS
          if (id == p.testBaseErrStrip) base += 1u; // (test build: this strip alone dithers from the wrong place)
#endif
        }
        else
        {
          base = p.stripBase[id];
          if (p.chainBase) base += (uint32_t)*p.chainBase; // first dither call of this image strip inside a chain that started on another GPU
        }
        phase_f_first_calls(L, base, lane);
      }
      __syncthreads();
      if (PERSIST && L.first[0] == kBasePoison) return; // the look-back gave up (status word raised): nothing that depends on the chain position is stored (completing the
                                                        // block-uniform planes' rows 4..7 here costs the 4-channel kernel two spilled VGPRs: they stay half written, the call has failed anyway)
      if (rowsPath) phase_f_rows<CH>(p, io, L, strip, x0, y0, lane, wave, [&]() { if (p.fullPlanes) phase_f_store_const(p, io, L, x0, y0, ry, lane, wave, 2u); });
      else phase_f_pixels<CH>(p, io, L, strip, x0, y0, ry, lane, wave, tid);
    }

    // ---- kernels ---------------------------------------------------------------------------------------------------------
    // The trial's form (NOSEL: without the red-weight select, trial_pixel_error) follows from the launch's pixel limit by red_select_dead (limg_hip_encode_rules.h).
    // The limit is a kernel argument of these kernels, so each instance holds its step for both forms and takes one of them with ONE scalar branch per workgroup, at
    // the top of the kernel: nothing is decided per strip, block or trial, and inside either side the form is a template argument all the way down.  (Not a further
    // template argument of the kernels: the set of kernel instances that take EncodeParams is pinned, tests/test_product_library.py.)
    template <int CH, bool FAST, bool PREFIT, bool ACC>
    __global__ __launch_bounds__(kThreads) void k_fit_search(const EncodeParams p)
    {
      __shared__ __attribute__((aligned(16))) uint8_t s_lds[lds_layout<PREFIT>().total];
      if (red_select_dead(p.maxPixel32)) fit_search_strip<CH, false, FAST, PREFIT, ACC, true>(p, p, p.io, blockIdx.x, blockIdx.x, 0u, 0u, s_lds, nullptr, (int)threadIdx.x);
      else fit_search_strip<CH, false, FAST, PREFIT, ACC, false>(p, p, p.io, blockIdx.x, blockIdx.x, 0u, 0u, s_lds, nullptr, (int)threadIdx.x);
    }

    template <int CH>
    __global__ __launch_bounds__(kThreads) void k_dither_store(const EncodeParams p)
    {
      __shared__ __attribute__((aligned(16))) uint8_t s_lds[kPhaseFBytes + kStripBlocks * 48];
      if (p.chainBase && *p.chainBase == ~0ull) return; // cross-GPU chain aborted by a rank (k_chain_base): nothing is stored, the status word is already raised
      dither_store_strip<CH, false>(p, p.io, blockIdx.x, blockIdx.x, 0u, 0u, s_lds, nullptr, (int)threadIdx.x);
    }

    // Both steps are inlined into the loop.  Left alone, LLVM hoists every lane-dependent address computation of both steps
    // out of the loop (they only depend on threadIdx) and keeps them all live: 194 VGPRs.  Passing the thread id through an
    // empty asm at the top of each iteration makes it opaque per iteration, which keeps the two steps' live ranges apart.
    // Persistent single-launch encode: 6 workgroups per CU (5 with the float stage inside) loop over the work strips (ticket order).  Each iteration runs the
    // VALU-bound E step (fit + search) of a new strip and then the HBM-bound F step (dither, decode, all plane stores) of the
    // strip the SAME workgroup fitted one iteration earlier, whose parked results sit in a private, L2-resident 8 KiB slot.
    // The one-iteration lag means that by the time an F step asks for its strip's position in the dither chain, every
    // earlier strip has long published its call count, so the look-back does not wait; and since the workgroups of a CU
    // drift apart, E and F steps of different workgroups overlap on every CU.
    // Progress: a look-back only waits for strips with smaller tickets; those were drawn earlier by workgroups that are running, and an E step never waits
    // (see "decoupled look-back" above: no strip id is ever derived from blockIdx).
    // The loop itself: limg_hip_persistent_loop.inc, one text for this kernel -- once per form of the trial, see k_fit_search -- and for k_encode_list_rated below.
    template <int CH, bool FAST, bool PREFIT, bool ACC>
    __global__ __launch_bounds__(kThreads, PREFIT ? 6 : 5) void k_encode_persistent(const EncodeParams p)
    {
      __shared__ __attribute__((aligned(16))) uint8_t s_lds[lds_layout<PREFIT>().total];
      __shared__ uint32_t s_ticket;
      typedef const __attribute__((address_space(4))) EncodeParams KernArgs;
      // the caller's pointers of the image a strip belongs to: the kernel arguments themselves for a single image, an entry of the device table for a batch (same
      // address space, same scalar loads).  The table was written by a copy that precedes this launch on the stream and is not modified while the kernel runs.
      typedef const __attribute__((address_space(4))) ImageIO KernIO;
      auto io_of = [](KernArgs *a, uint32_t img) -> KernIO * { return a->batchCount > 1 ? (KernIO *)a->batch + img : &a->io; };
#define LIMG_LOOP_LIMITS(a, img) (*(a)) /* one error factor: the limits are kernel arguments */
// (a list of one shape: the image of a strip by a division, its strips and block rows image after image, the kernel arguments as every image's view)
#define LIMG_LOOP_STRIPS(a) ((a)->imageStrips * (a)->batchCount)
#define LIMG_LOOP_FIND_IMAGE(a, t, img) if ((a)->batchCount > 1) img = (t) / (a)->imageStrips;
#define LIMG_LOOP_HEAD0(a, img) ((img) * (a)->imageStrips)
#define LIMG_LOOP_ROWBASE(a, img) ((img) * (a)->blocksY)
#define LIMG_LOOP_VIEW(a, img) (a)
      if (red_select_dead(p.maxPixel32))
      {
        constexpr bool NOSEL = true;
#include "limg_hip_persistent_loop.inc"
      }
      else
      {
        constexpr bool NOSEL = false;
#include "limg_hip_persistent_loop.inc"
      }
#undef LIMG_LOOP_LIMITS
    }

    // A list whose images each carry their own error factor (limg_hip_encode_stream_batch_ef*): the same loop in compact stream mode behind k_fit_tpb, default search.
    // Once per strip the E step fetches its image's entry of the threshold table with scalar loads, as it fetches the image's pointers: the limits stay on the
    // scalar unit, no lane holds a threshold.  The F step needs none of them.  The table, like the ImageIO table, was written by a launch that precedes this one on
    // the stream and is not modified while the kernel runs.
    template <int CH, bool FAST>
    __global__ __launch_bounds__(kThreads, 6) void k_encode_list_rated(const RatedListParams p)
    {
      constexpr bool PREFIT = true, ACC = false, NOSEL = false; // (the limits differ from image to image, in device memory: the trial keeps its select)
      __shared__ __attribute__((aligned(16))) uint8_t s_lds[lds_layout<PREFIT>().total];
      __shared__ uint32_t s_ticket;
      typedef const __attribute__((address_space(4))) RatedListParams KernArgs;
      typedef const __attribute__((address_space(4))) ImageIO KernIO;
      typedef const __attribute__((address_space(4))) RatedImage KernLimits;
      auto io_of = [](KernArgs *a, uint32_t img) -> KernIO * { return (KernIO *)a->batch + img; }; // (a sub-batch of one image reads the table too)
#define LIMG_LOOP_LIMITS(a, img) (*((KernLimits *)(a)->rated + (img)))
#include "limg_hip_persistent_loop.inc"
    }
#undef LIMG_LOOP_STRIPS
#undef LIMG_LOOP_FIND_IMAGE
#undef LIMG_LOOP_HEAD0
#undef LIMG_LOOP_ROWBASE
#undef LIMG_LOOP_VIEW

    // A list whose images differ in SHAPE (limg_hip_encode_stream_list*; layout: limg_hip_list_plan.h): the same loop over the chunk's concatenated strips.  The image
    // of a strip comes from a wave-uniform binary search over the strip prefix; what the stages read as `p` is that image's VIEW, an entry of a device table with
    // RatedListParams' layout (its geometry, flags, chain partition, and records / invN / shifts offset to its first block: rowBase is 0), fetched with scalar
    // loads where a stage uses a field, exactly as the siblings fetch kernel arguments.  The F step of the previous strip reads the previous image's view by its
    // index.  Ticket, look-back (bounded, poisoning on a time-out) and park slots are those of the siblings; desc, stripWords, noise and timeout are the launch's
    // own in every view and indexed by the global strip id.  (find_strip_image: limg_hip_device.h, shared with the size probe of a mixed list.)
    template <int CH, bool FAST>
    __global__ __launch_bounds__(kThreads, 6) void k_encode_list_mixed(const MixedListParams p)
    {
      constexpr bool PREFIT = true, ACC = false, NOSEL = false;
      __shared__ __attribute__((aligned(16))) uint8_t s_lds[lds_layout<PREFIT>().total];
      __shared__ uint32_t s_ticket;
      typedef const __attribute__((address_space(4))) MixedListParams KernArgs;
      typedef const __attribute__((address_space(4))) RatedListParams KernView;
      typedef const __attribute__((address_space(4))) ImageIO KernIO;
      typedef const __attribute__((address_space(4))) RatedImage KernLimits;
      typedef const __attribute__((address_space(4))) uint32_t KernWord;
      auto io_of = [](KernArgs *a, uint32_t img) -> KernIO * { return (KernIO *)(uintptr_t)a->batch + img; };
#define LIMG_LOOP_STRIPS(a) ((a)->nStrips)
#define LIMG_LOOP_FIND_IMAGE(a, t, img) img = find_strip_image((a)->firstStrip, (a)->nImages, (t));
#define LIMG_LOOP_HEAD0(a, img) (((KernWord *)(uintptr_t)(a)->firstStrip)[img])
#define LIMG_LOOP_ROWBASE(a, img) 0u
#define LIMG_LOOP_VIEW(a, img) ((KernView *)(uintptr_t)(a)->views + (img))
#undef LIMG_LOOP_LIMITS
#define LIMG_LOOP_LIMITS(a, img) (*((KernLimits *)(uintptr_t)(a)->rated + (img)))
#include "limg_hip_persistent_loop.inc"
#undef LIMG_LOOP_LIMITS
#undef LIMG_LOOP_STRIPS
#undef LIMG_LOOP_FIND_IMAGE
#undef LIMG_LOOP_HEAD0
#undef LIMG_LOOP_ROWBASE
#undef LIMG_LOOP_VIEW
    }
  } // namespace

  // the kernel instance for (channels, float mode, float stage already done by k_fit_tpb, accurate search): launch(CH, FAST, PREFIT, ACC), each an
  // std::integral_constant
  template <class Launch>
  void with_encode_variant(const EncodeParams &p, int channels, Launch &&launch)
  {
    with_flags([&](auto acc, auto rgba, auto fast, auto prefit) { launch(std::integral_constant<int, rgba ? 4 : 3>(), fast, prefit, acc); }, !p.fast && p.crushBits,
               channels == 4, p.floatFast != 0, p.prefit != 0);
  }

  void launch_fit_search(const EncodeParams &p, int channels, hipStream_t s)
  {
    const dim3 grid(p.stripsX * p.blocksY), block(kThreads);
    with_encode_variant(p, channels, [&](auto CH, auto FAST, auto PREFIT, auto ACC) { hipLaunchKernelGGL((k_fit_search<CH, FAST, PREFIT, ACC>), grid, block, 0, s, p); });
  }

  void launch_encode_persistent(const EncodeParams &p, int channels, int workgroups, hipStream_t s)
  {
    const uint32_t strips = p.imageStrips * p.batchCount;
    const dim3 grid(strips < (uint32_t)workgroups ? strips : (uint32_t)workgroups), block(kThreads);
    with_encode_variant(p, channels, [&](auto CH, auto FAST, auto PREFIT, auto ACC) { hipLaunchKernelGGL((k_encode_persistent<CH, FAST, PREFIT, ACC>), grid, block, 0, s, p); });
  }

  namespace
  {
    // the threshold table of a list with one error factor per image: the factors travel inside kernel arguments (as k_set_batch_table's pointers: stream-ordered, and
    // the caller's array may die right away); thread i turns image i's into its entry by the rule every encode uses (thresholds, limg_hip_encode_rules.h)
    struct RatedChunk { uint32_t n; uint32_t errorFactor[64]; };
    __global__ void k_set_rated_table(RatedImage *dst, const RatedChunk chunk)
    {
      const uint32_t i = threadIdx.x;
      if (i >= chunk.n) return;
      const Thresholds t = thresholds(chunk.errorFactor[i]);
      RatedImage e;
      e.maxPixel32 = t.maxPixel32; e.blockLimitFull = t.blockLimitFull; e.maxBlock = t.maxBlock; e.crushBits = (int32_t)t.crushBits;
      e.errorFactor = chunk.errorFactor[i]; e.pad[0] = 0u; e.pad[1] = 0u;
      dst[i] = e;
    }
  }

  void launch_set_rated_table(RatedImage *dTable, const uint32_t *hErrorFactors, size_t count, hipStream_t s)
  {
    for (size_t i0 = 0; i0 < count; i0 += 64)
    {
      RatedChunk ch;
      ch.n = (uint32_t)(count - i0 < 64 ? count - i0 : 64);
      for (uint32_t i = 0; i < 64; i++) ch.errorFactor[i] = i < ch.n ? hErrorFactors[i0 + i] : 0u;
      hipLaunchKernelGGL(k_set_rated_table, dim3(1), dim3(64), 0, s, dTable + i0, ch);
    }
  }

  void launch_encode_list_rated(const RatedListParams &p, int channels, bool floatFast, int workgroups, hipStream_t s)
  {
    const uint32_t strips = p.imageStrips * p.batchCount;
    const dim3 grid(strips < (uint32_t)workgroups ? strips : (uint32_t)workgroups), block(kThreads);
    with_flags([&](auto rgba, auto fast) { hipLaunchKernelGGL((k_encode_list_rated<rgba ? 4 : 3, fast>), grid, block, 0, s, p); }, channels == 4, floatFast);
  }

  void launch_encode_list_mixed(const MixedListParams &p, int channels, bool floatFast, int workgroups, hipStream_t s)
  {
    const dim3 grid(p.nStrips < (uint32_t)workgroups ? p.nStrips : (uint32_t)workgroups), block(kThreads);
    with_flags([&](auto rgba, auto fast) { hipLaunchKernelGGL((k_encode_list_mixed<rgba ? 4 : 3, fast>), grid, block, 0, s, p); }, channels == 4, floatFast);
  }

  namespace
  {
    // exclusive prefix over the ranks before `rank` of the all-gathered per-rank dither-call totals.  A rank whose E step failed joins the all-gather with ~0: the
    // base is then poisoned too (k_dither_store stores nothing) and the context's sticky "aborted chain" word is raised for limg_hip_check_device_status.
    __global__ void k_chain_base(const unsigned long long *calls, int rank, int world, unsigned long long *base, uint32_t *aborted)
    {
      unsigned long long run = 0;
      bool poison = false;
      for (int r = 0; r < world; r++)
      {
        poison = poison || calls[r] == ~0ull;
        if (r < rank) run += calls[r];
      }
      *base = poison ? ~0ull : run;
      if (poison) *aborted = 1u;
    }
  }
  namespace
  {
    // The reference's bit statistics (src/limg.cpp:1971-1999, printed at :2232-2248): per factor the bits kept, summed over the pixels, and a histogram of the
    // pixels by shift -- a function of the per-block shift words and the blocks' pixel counts alone.  out[0..2] += (8 - shift) * n, out[3 + 9 f + shift] += n.
    __global__ __launch_bounds__(256) void k_shift_stats(const uint32_t *shifts, uint32_t blocksX, uint32_t blocksY, uint32_t rows /* blocksY x images */, uint32_t sizeX, uint32_t sizeY,
                                                         unsigned long long *out)
    {
      __shared__ uint32_t s_acc[30];
      if (threadIdx.x < 30) s_acc[threadIdx.x] = 0;
      __syncthreads();
      const uint64_t total = (uint64_t)blocksX * rows;
      // a workgroup covers at most 256 * 16 blocks of <= 64 pixels and <= 8 bits each: the 32-bit partial sums cannot overflow
      const uint64_t begin = (uint64_t)blockIdx.x * 4096u;
      for (uint64_t i = begin + threadIdx.x; i < min(begin + 4096u, total); i += 256u)
      {
        const uint32_t row = (uint32_t)(i / blocksX), bx = (uint32_t)(i - (uint64_t)row * blocksX), by = row % blocksY;
        const uint32_t rx = min(sizeX - bx * kBlock, (uint32_t)kBlock), ry = min(sizeY - by * kBlock, (uint32_t)kBlock), n = rx * ry;
        const uint32_t w = shifts[i];
#pragma unroll
        for (int f = 0; f < 3; f++)
        {
          const uint32_t sh = min((w >> (8 * f)) & 0xFFu, 8u);
          atomicAdd(&s_acc[f], (8u - sh) * n);
          atomicAdd(&s_acc[3 + 9 * f + sh], n);
        }
      }
      __syncthreads();
      if (threadIdx.x < 30 && s_acc[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)s_acc[threadIdx.x]);
    }
  }
  void launch_shift_stats(const uint32_t *dShifts, uint32_t blocksX, uint32_t blocksY, uint32_t rows, uint32_t sizeX, uint32_t sizeY, unsigned long long *dOut30, hipStream_t s)
  {
    const uint64_t total = (uint64_t)blocksX * rows;
    hipLaunchKernelGGL(k_shift_stats, dim3((uint32_t)((total + 4095u) / 4096u)), dim3(256), 0, s, dShifts, blocksX, blocksY, rows, sizeX, sizeY, dOut30);
  }

  void launch_chain_base(const unsigned long long *dCalls, int rank, int world, unsigned long long *dBase, uint32_t *dAborted, hipStream_t s)
  {
    hipLaunchKernelGGL(k_chain_base, dim3(1), dim3(1), 0, s, dCalls, rank, world, dBase, dAborted);
  }

  void launch_strip_scan(const EncodeParams &p, hipStream_t s) { hipLaunchKernelGGL(k_strip_scan, dim3(1), dim3(1024), 0, s, p); }

  void launch_dither_store(const EncodeParams &p, int channels, hipStream_t s)
  {
    const dim3 grid(p.stripsX * p.blocksY), block(kThreads);
    if (channels == 4) hipLaunchKernelGGL(k_dither_store<4>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_dither_store<3>, grid, block, 0, s, p);
  }
} // namespace limg_hip
