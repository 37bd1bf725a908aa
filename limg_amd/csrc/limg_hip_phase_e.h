// limg_hip_phase_e.h -- the E step's stages that start from the records of k_fit_tpb and end with a block's three factor bytes per pixel, and the LDS layout they
// work in: request_prefit_records / take_prefit_records, stage_strip_pixels, phase_e_view, pixel_factors.  fit_search_strip (limg_hip_kernels.hip) calls them around its
// block queue; the stream's size probe (k_rate_probe, limg_hip_rate.hip) runs the same stages and the same search and keeps only the field widths.  Every stage takes
// its parameters as a template type: what it reads of them is what the caller's struct has to have.
#ifndef LIMG_HIP_PHASE_E_H
#define LIMG_HIP_PHASE_E_H

#include "limg_hip_search.h"
#include "limg_hip_phase_f.h"
#include "limg_hip_float_pixel.h"

namespace limg_hip
{
  namespace
  {
    // LDS of an E task (fit + search of one work strip); the F task's areas overlay `V`.
    constexpr int kLdsStrip = 0, kLdsV = kLdsStrip + 8 * kRowDw * 4, kLdsVBytes = kWaves * kBatch * kVDw * 4;
    constexpr int kLdsBlk = kLdsV + kLdsVBytes, kLdsCalls = kLdsBlk + kStripBlocks * 192, kLdsTotal = kLdsCalls + 32; // 4 per-wave call counts + the phase-E block queue
    static_assert(kLdsTotal <= 32768 - 16, "5 workgroups per CU");
    // PREFIT (float stage done by k_fit_tpb): the parked-contribution area shrinks to the 7.5 KiB factor-byte staging area; E layout 24.3 KiB, F overlay 23.9 KiB
    // => 6 workgroups per CU
    struct LdsLayout { int v, blk, calls, trialc, total; };
    constexpr int kTrialConstDw = 20; // per block: nA[3] nB[3] nC[3] mA[3] mB[3] mC[3] (+2 pad): the integer view of the record the packed trial multiplies with
    template <bool PREFIT> __device__ __host__ constexpr LdsLayout lds_layout()
    {
      if (!PREFIT) return LdsLayout{ kLdsV, kLdsBlk, kLdsCalls, kLdsV, kLdsTotal }; // (no trial-constant table in this layout)
      const int v = kLdsStrip + 8 * kRowDw * 4, blk = v + kFacBytes, calls = blk + kStripBlocks * 192, tc = calls + 32, e = tc + kStripBlocks * kTrialConstDw * 4;
      const int f = kLdsStrip + kPhaseFBytes + kStripBlocks * 48 + 16; // the F step's overlay incl. its record copy
      return LdsLayout{ v, blk, calls, tc, e > f ? e : f };
    }
    static_assert(lds_layout<true>().total <= 163840 / 6, "6 workgroups per CU with the float stage in its own kernel");


    // PERSIST == false: split path, the strip's call count goes to p.stripCalls for k_strip_scan.
    // PERSIST == true : persistent kernel, the count is published as an "aggregate" look-back descriptor.
    // parked results of one strip (persistent kernel): pre-dither factor bytes, records (int16 part), shift words
    constexpr int kParkFac = 0, kParkRec = 6144, kParkShift = 6144 + 1536, kParkBytes = 8192;

    // ---- the E step's stages, in the order fit_search_strip calls them (tools/isa_budget.py attributes the kernel's instructions to them by function) ----------

    // E: record load + flags (PREFIT), first half.  The records of the wave's 8 blocks as k_fit_tpb left them (16 dwords per block: avg, then the 24 int16; 16 lanes
    // per block) are REQUESTED here, next to the strip's pixels, and used behind the barrier below: one memory round trip per strip instead of two.  Round 4, same-box A/B (tools/r04/run19.sh): persistent
    // kernel 1.079-1.085 -> 1.054-1.059 ms on 8192^2 photo-noise, config 4 15.01-15.13 -> 14.46-14.65 ms.  (The same idea for the F step -- the strip's own look-back
    // descriptor and the first window requested before the parked data -- costs 4 spilled registers and was measured 0.5-1 % slower: not kept.)
    template <class P>
    __device__ __forceinline__ void request_prefit_records(const P &p, const EStrip g, uint32_t recVal[2])
    {
#pragma unroll
      for (int r = 0; r < 2; r++)
      {
        const int b = r * 4 + (g.lane >> 4), w = g.lane & 15;
        const uint32_t bx = g.strip * kStripBlocks + g.wave * kBlocksPerWave + b;
        if (bx < p.blocksX) recVal[r] = w >= 4 ? reinterpret_cast<const uint32_t *>(p.records + (size_t)g.byS * p.blocksX + bx)[w] // (the averages in words 0..3 are not needed here)
                                               : reinterpret_cast<const uint32_t *>(p.invN)[((size_t)g.byS * p.blocksX + bx) * 4 + w];      // 1 / |n|^2 of A, B, C from k_fit_tpb
      }
    }

    // E: strip staging -- the strip's pixel rows into LDS (the rsqrt table is read from global memory where it is used)
    template <class P, class IO>
    __device__ __forceinline__ void stage_strip_pixels(const P &p, const IO &io, const EStrip g)
    {
      const int tid = g.tid;
      if (p.vecIn)
      {
#pragma unroll
        for (int pass = 0; pass < 2; pass++)
        {
          const uint32_t row = pass * 4 + (tid >> 6), col = (tid & 63) * 4; // 4 px per lane
          if (row < g.ry && col < g.stripW)
          {
            const uint4 v = *reinterpret_cast<const uint4 *>(io.in + (size_t)(g.y0 + row) * p.sizeX + g.x0 + col); // (as a non-temporal load: measured, no difference -- tools/r05/ab_nt_loads.sh)
            *reinterpret_cast<uint4 *>(&g.pix[row * kRowDw + col]) = v;
          }
        }
      }
      else
      {
        for (uint32_t i = tid; i < 8 * 256; i += kThreads)
        {
          const uint32_t row = i >> 8, col = i & 255;
          if (row < g.ry && col < g.stripW) g.pix[row * kRowDw + col] = io.in[(size_t)(g.y0 + row) * p.sizeX + g.x0 + col];
        }
      }
    }

    // E: record load + flags (PREFIT), second half -- the records requested above: into the phase-E view, the park slot, and the range flags
    template <bool PERSIST, class P>
    __device__ __forceinline__ void take_prefit_records(const P &p, const EStrip g, const uint32_t recVal[2], uint8_t *park)
    {
      BlkF *blk = g.blk + g.wave * kBlocksPerWave;
#pragma unroll
      for (int r = 0; r < 2; r++)
      {
        const int b = r * 4 + (g.lane >> 4), w = g.lane & 15;
        const uint32_t sb = g.wave * kBlocksPerWave + b, bx = g.strip * kStripBlocks + sb;
        const uint32_t val = recVal[r];
        if (w < 3) reinterpret_cast<BlkE *>(&blk[b])->invN[w] = __uint_as_float(val); // its place in the phase-E view (nothing else of the float-stage fields is live with PREFIT)
        if (w >= 4)
        {
          reinterpret_cast<uint32_t *>(blk[b].rec)[w - 4] = val;
          if (PERSIST) reinterpret_cast<uint32_t *>(park + kParkRec)[sb * 12 + (w - 4)] = val;
        }
        const int lo = (int)(int16_t)(val & 0xFFFFu), hi = (int)(int16_t)(val >> 16);
        uint32_t big = (w >= 4 && (lo > p.recordLimit || lo < -p.recordLimit || hi > p.recordLimit || hi < -p.recordLimit)) ? 1u : 0u;
        big |= (uint32_t)dpp<0xB1, 0xF>(0, (int)big);  // OR over the block's 16 lanes (one DPP row)
        big |= (uint32_t)dpp<0x4E, 0xF>(0, (int)big);
        big |= (uint32_t)dpp<0x141, 0xF>(0, (int)big);
        big |= (uint32_t)dpp<0x140, 0xF>(0, (int)big);
        if (w == 0) { blk[b].flags = (bx < p.blocksX ? kValid : 0u) | (big ? kBig : 0u); blk[b].n = bx < p.blocksX ? 64u : 0u; }
      }
      wave_lds_fence();
    }

    // E: phase-E view + trial constants (a7).  The view overlays the dead float-stage fields: float normals / offsets and 1 / |n|^2 in the serial limg_dot
    // order (src/limg_internal.h:426-452).  One lane per (block, factor, channel): 96 of 128 lane slots.
    template <int CH, bool FAST, bool PREFIT>
    __device__ __forceinline__ void phase_e_view(const EStrip g)
    {
      const int lane = g.lane;
      BlkF *blk = g.blk + g.wave * kBlocksPerWave;
      float nrm[2], off[2], invn[2];
#pragma unroll
      for (int r = 0; r < 2; r++)
      {
        const int idx = min(r * 64 + lane, 95);
        const int b = idx / 12, fc = idx - b * 12, f = fc >> 2, c = fc & 3;
        const int lo = blk[b].rec[f * 8 + c], hi = blk[b].rec[f * 8 + 4 + c];
        nrm[r] = (float)(hi - lo); off[r] = (float)lo;
        if (PREFIT) { invn[r] = 0.0f; continue; } // k_fit_tpb left 1 / |n|^2 with the record
        const float sq = nrm[r] * nrm[r];
        const float s0 = __int_as_float(dpp<0x00, 0xF>(0, __float_as_int(sq))), s1 = __int_as_float(dpp<0x55, 0xF>(0, __float_as_int(sq)));
        const float s2 = __int_as_float(dpp<0xAA, 0xF>(0, __float_as_int(sq))), s3 = __int_as_float(dpp<0xFF, 0xF>(0, __float_as_int(sq)));
        float s = ((0.0f + s0) + s1) + s2;
        if (CH == 4) s = s + s3;
        const bool nz = (s0 != 0.0f) || (s1 != 0.0f) || (s2 != 0.0f) || (CH == 4 && s3 != 0.0f);
        invn[r] = nz ? (FAST ? __builtin_amdgcn_rcpf(s) : 1.0f / s) : 0.0f;
      }
      wave_lds_fence(); // every lane has read what it needs of the float-stage fields before the overlay is written
#pragma unroll
      for (int r = 0; r < 2; r++)
      {
        const int idx = r * 64 + lane;
        if (idx < 96)
        {
          const int b = idx / 12, fc = idx - b * 12, f = fc >> 2, c = fc & 3;
          BlkE *e = reinterpret_cast<BlkE *>(&blk[b]);
          e->nrm[f][slot_of(c)] = nrm[r]; e->off[f][slot_of(c)] = off[r]; // slot order x0 x2 x1 x3, see V4
          if (!PREFIT && c == 0) e->invN[f] = invn[r];
          if (PREFIT && c < 3)
          { // the packed trial's integer operands (negated, see "a9, packed form"), once per block here instead of per lane in phase E
            int *tc = g.trialc + (g.wave * kBlocksPerWave + b) * kTrialConstDw;
            tc[f * 3 + c] = -(int)nrm[r];
            tc[9 + f * 3 + c] = term_const(f, c, (int)off[r]);
          }
        }
      }
    }

    // E: per-pixel factors, a8 (src/limg_factorization.h:149-197): fa = ((px - Amin) . nA) * invA, est = Amin + nA * fa, fb from px - est - Boff, ...
    template <int CH, bool FAST>
    __device__ __forceinline__ void pixel_factors(const BlkE *be, const uint32_t px, uint32_t &fA, uint32_t &fB, uint32_t &fC)
    {
      const V4 pv = px_to_v4(px);
      const V4 nA = ld4(be->nrm[0]), mnA = ld4(be->off[0]);
      const float fa = dp4<CH, FAST>(pv - mnA, nA) * be->invN[0];
      fA = cvt_u8_rne_sat(255.0f * fa);
      const V4 nB = ld4(be->nrm[1]), ofB = ld4(be->off[1]);
      V4 est = mnA + nA * fa;
      const float fb = dp4<CH, FAST>((pv - est) - ofB, nB) * be->invN[1];
      fB = cvt_u8_rne_sat(255.0f * fb);
      const V4 nC = ld4(be->nrm[2]), ofC = ld4(be->off[2]);
      est = est + nB * fb;
      const float fc = dp4<CH, FAST>((pv - est) - ofC, nC) * be->invN[2];
      fC = cvt_u8_rne_sat(255.0f * fc);
    }
  } // namespace
} // namespace limg_hip

#endif
