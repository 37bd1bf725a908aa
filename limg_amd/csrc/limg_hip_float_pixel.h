// limg_hip_float_pixel.h -- the E step's lane == pixel float stage (a4-a6), which images with partial edge blocks keep: the per-block LDS state (BlkF, and the
// phase-E view BlkE that overlays it), what every stage of the E step knows of its strip (EStrip, block_geom, block_pixel) and the pixel-order direction sums
// (serial_sums2).  Phases A-D themselves are inline in fit_search_strip: as a function of their own they cost the instances that run them 5 % (see there).
// Included through limg_hip_phase_e.h by limg_hip_kernels.hip and limg_hip_rate.hip, each one translation unit (the same per-source compile flags cover this code).
#ifndef LIMG_HIP_FLOAT_PIXEL_H
#define LIMG_HIP_FLOAT_PIXEL_H

#include "limg_hip_device.h"

namespace limg_hip
{
  namespace
  {
    constexpr int kRowDw = 264; // LDS pixel-row stride in dwords: 256 px + 8 pad => bank = (8*row + x) mod 32, conflict-free per 32-lane half
    constexpr int kVDw = 260;   // per-block stride of the parked contributions: 64 px * 4 ch + 4 pad => the (block, channel) walkers hit 32 distinct banks

    // Per-block state in LDS.  The first 120 bytes are the float-stage state; once the record has been produced they are
    // dead and the same bytes carry what phase E needs (`BlkE` view).
    struct BlkF
    {
      float avg[4], dirA[4], dirB[4], dirC[4], est0[4]; // 80
      float mm[6];                                      // 104: minA maxA minB maxB minC maxC
      float inv_count, invA, invB, invC;                // 120
      uint32_t flags, n;                                // 128
      int16_t rec[24];                                  // 176
      float pad[4];                                     // 192
    };
    struct BlkE
    {
      float nrm[3][4]; // 48: float normals (max - min) of A, B, C            (slot order x0 x2 x1 x3)
      float off[3][4]; // 96: float dirA_min, dirB_offset, dirC_offset         (slot order)
      float invN[3];   // 108
    };
    static_assert(sizeof(BlkE) <= 120, "BlkE must fit the dead float-stage fields");
    static_assert(sizeof(BlkF) == 192, "BlkF layout");

    // What every stage of the E step (fit_search_strip, limg_hip_kernels.hip) knows of its work strip: geometry (wave-uniform), the thread, the LDS areas.
    // The stages take it BY VALUE: a stage is optimised on its own before it is inlined, and behind a reference every LDS store in it might alias these fields
    // (measured on the compiler's metadata: by reference the split path's lane == pixel instances take 2 more VGPRs).
    struct EStrip
    {
      uint32_t strip, by, byS; // the strip's place in its block row, its block row in the image, and in the per-block scratch arrays (records, shift words)
      uint32_t x0, y0, stripW, ry; // pixels: origin, width and rows inside the image
      int tid, lane, wave;
      uint32_t *pix;   // [8 rows][kRowDw] the strip's pixels
      float *V;        // the parked contributions of the float stage (all waves); later the factor-byte staging area
      BlkF *blk;       // [kStripBlocks]
      uint32_t *calls; // 4 per-wave call counts + the phase-E block queue
      int *trialc;     // PREFIT: [kStripBlocks][kTrialConstDw]
    };

    // geometry of block sb of the strip (wave-uniform): its width and pixel count; false: past the image's right edge
    template <class P>
    __device__ __forceinline__ bool block_geom(const P &p, const EStrip g, const uint32_t sb, uint32_t &rx, uint32_t &n)
    {
      const uint32_t bx = g.strip * kStripBlocks + sb;
      if (bx >= p.blocksX) { rx = 0; n = 0; return false; }
      rx = min(p.sizeX - bx * kBlock, (uint32_t)kBlock);
      n = rx * g.ry;
      return true;
    }

    // lane == pixel: the lane's pixel of block sb (0 for lanes past the block's n pixels) and its position inside the block
    __device__ __forceinline__ uint32_t block_pixel(const EStrip g, const uint32_t sb, const uint32_t rx, const uint32_t n, uint32_t &lx, uint32_t &ly)
    {
      const int lane = g.lane;
      if (rx == 8) { lx = lane & 7; ly = lane >> 3; }
      else { const uint32_t l = (uint32_t)lane < n ? (uint32_t)lane : 0u; ly = l / rx; lx = l - ly * rx; }
      const uint32_t px = g.pix[ly * kRowDw + sb * kBlock + lx];
      return (uint32_t)lane < n ? px : 0u;
    }

    enum : int { kDirA = 0, kDirB = 1, kDirC = 2 };
    constexpr int kBatch = 4; // blocks per wave whose pass contributions are parked at a time
    constexpr uint32_t kBig = 16u; // some |record value| > kRecordLimit => generic 32-bit trial

    // Pixel-order accumulation (as `serial_sums`) followed, lane-parallel over the wave's 8 blocks, by everything the next
    // phase needs of the new direction: 1 / (dir . dir) with the DPPS order (correctly rounded division, once per 8 blocks)
    // and the all-zero flag.
    template <int CH, int WHICH, bool FAST>
    __device__ __forceinline__ void serial_sums2(const float *V, BlkF *blk, int lane)
    {
      wave_lds_fence();
      if (lane < 4 * kBatch)
      {
        const int b = lane >> 2, c = lane & 3;
        const float *src = V + b * kVDw + c;
        float s = 0.0f;
#pragma unroll 16
        for (int i = 0; i < 64; i++) s = s + src[i * 4];
        const float dir = s * blk[b].inv_count;
        float *dst = WHICH == kDirA ? blk[b].dirA : (WHICH == kDirB ? blk[b].dirB : blk[b].dirC);
        dst[c] = dir;
        // (p0 + p1) + (p2 + p3) inside each quad of lanes (slot order x0 x2 x1 x3: channels 0,1 sit in slots 0,2); float add is
        // commutative, so the two xor butterflies give exactly that
        float p = (CH == 3 && c == 3) ? 0.0f : dir * dir;
        p = p + __int_as_float(dpp<0x4E, 0xF>(0, __float_as_int(p))); // slot ^ 2
        p = p + __int_as_float(dpp<0xB1, 0xF>(0, __float_as_int(p))); // slot ^ 1
        uint32_t z = (dir == 0.0f) ? 1u : 0u;
        z &= (uint32_t)dpp<0xB1, 0xF>(0, (int)z);
        z &= (uint32_t)dpp<0x4E, 0xF>(0, (int)z);
        const float inv = FAST ? __builtin_amdgcn_rcpf(p) : 1.0f / p;
        if (c == 0)
        {
          if (WHICH == kDirA) { blk[b].invA = inv; if (z) blk[b].flags |= kZeroA | kZeroB | kZeroC; }
          else if (WHICH == kDirB) { blk[b].invB = inv; if (z) blk[b].flags |= kZeroB | kZeroC; }
          else { blk[b].invC = inv; if (z) blk[b].flags |= kZeroC; }
        }
      }
      wave_lds_fence();
    }
  } // namespace
} // namespace limg_hip

#endif
