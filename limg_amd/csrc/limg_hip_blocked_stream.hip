// limg_hip_blocked_stream.hip -- version 2 of the "LMG3" stream: the merged-block encoder's rectangles (format: include/limg_hip.h).  The packer; every decode of this
// version, the whole image included, is limg_hip_stream_window.hip.
//
// Pack, after a compact-mode merged-block encode (blocked_encode_device with no planes), from what that leaves in the context: per rectangle its descriptor, record and
// shift word, its pre-dither factor bytes and noise bytes, both region-major (pixel i = yy * wpx + xx of the rectangle at byte i: the order the stream wants).
//   k_bstream_sizes<false>  per tile of 256 rectangles: payload words and 64-pixel runs
//   k_stream_tile_scan<2>   one workgroup: exclusive prefix over the tiles, the header (limg_hip_stream_format.h, shared with version 1)
//   k_bstream_sizes<true>   per rectangle: its first payload word and first run, its 64-byte table entry
//   k_bstream_pack          lane = one RUN: 64 consecutive pixels of one rectangle, its three fields one after the other.  Rectangles are wildly uneven (a single
//                           block up to thousands), runs are not: a lane finds its rectangle by bisection over the runs' prefix, reads 64 factor bytes (and 64 noise
//                           bytes where the field is dithered) with four 16-byte loads, dithers and crushes them (dither_crush4, as k_blocked_store does), squeezes every 8
//                           values into b bytes with the mask-and-shift steps of k_stream_pack_strips and stores b 8-byte words.  Runs that are short (the tail of a
//                           rectangle on an image with partial blocks) or not 16-byte aligned gather their bytes one by one -- same bytes out.
#include "limg_hip_stream_format.h"

namespace limg_hip
{
  namespace
  {
    constexpr int kRectTile = 256;
    // ---- pack ------------------------------------------------------------------------------------------------------------------------
    struct RectSize { uint32_t bits, words, runs, sw; };
    __device__ __forceinline__ RectSize rect_size(const BlockedStreamParams &p, uint32_t r)
    {
      const RegionDesc R = p.regions[r];
      const uint4 *rp = reinterpret_cast<const uint4 *>(p.out + r) + 1; // skip avg[4]: {dirA_min, dirA_max}, {dirB_offset, dirB_mag}, {dirC_offset, dirC_mag}
      int mn3[3], mx3[3];
      alpha_lanes(rp[0], rp[1], rp[2], mn3, mx3);
      RectSize o;
      o.sw = p.out[r].shiftWord & 0xFFFFFFu;
      o.bits = field_bits(o.sw, mn3, mx3, (int)p.channels);
      uint32_t wpx;
      const uint32_t n = rect_pixels(p.sizeX, p.sizeY, p.blocksX, p.blocksY, R.ox, R.oy, R.rx, R.ry, wpx);
      o.words = rect_words(n, o.bits);
      o.runs = (n + 63u) >> 6;
      return o;
    }

    // ENTRIES = false: the tile's totals.  ENTRIES = true (after the scan): every rectangle's first payload word and first run, and its table entry.
    template <bool ENTRIES>
    __global__ __launch_bounds__(kRectTile) void k_bstream_sizes(const BlockedStreamParams p)
    {
      __shared__ uint32_t sWords[4], sRuns[4];
      const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
      const uint32_t r = blockIdx.x * kRectTile + tid;
      RectSize z = { 0, 0, 0, 0 };
      if (r < p.nRegions) z = rect_size(p, r);
      const uint32_t iw = wave_scan_inclusive(z.words, lane), ir = wave_scan_inclusive(z.runs, lane);
      if (lane == 63) { sWords[wave] = iw; sRuns[wave] = ir; }
      __syncthreads();
      if (!ENTRIES)
      {
        if (tid == 0) { p.tiles[2 * blockIdx.x] = sWords[0] + sWords[1] + sWords[2] + sWords[3]; p.tiles[2 * blockIdx.x + 1] = sRuns[0] + sRuns[1] + sRuns[2] + sRuns[3]; }
        return;
      }
      uint32_t word = p.tiles[2 * blockIdx.x] + iw - z.words, run = p.tiles[2 * blockIdx.x + 1] + ir - z.runs;
      for (int w = 0; w < wave; w++) { word += sWords[w]; run += sRuns[w]; }
      if (r >= p.nRegions) return;
      p.units[r] = run;
      if (r + 1 == p.nRegions) p.units[r + 1] = run + z.runs;
      const RegionDesc R = p.regions[r];
      const uint4 *rp = reinterpret_cast<const uint4 *>(p.out + r) + 1;
      uint4 *e = reinterpret_cast<uint4 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)r * kRectEntry);
      e[0] = rp[0]; e[1] = rp[1]; e[2] = rp[2];
      e[3] = make_uint4(z.sw | (z.bits & 0xFF000000u), word, R.ox | (R.oy << 16), R.rx | (R.ry << 16));
    }

    // 64 bytes of a region-major array into 16 dwords: four 16-byte loads where the run is whole and aligned, else byte by byte (absent pixels read as 0)
    __device__ __forceinline__ void load_run(const uint8_t *src, uint32_t count, uint32_t v[16])
    {
      if (count == 64u && (reinterpret_cast<uintptr_t>(src) & 15u) == 0)
      {
#pragma unroll
        for (int q = 0; q < 4; q++)
        {
          const uint4 t = reinterpret_cast<const uint4 *>(src)[q];
          v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
        return;
      }
#pragma unroll
      for (int q = 0; q < 16; q++)
      {
        uint32_t w = 0;
#pragma unroll
        for (int t = 0; t < 4; t++)
          if ((uint32_t)(4 * q + t) < count) w |= (uint32_t)src[4 * q + t] << (8 * t);
        v[q] = w;
      }
    }

    // 64 values of B bits, one per byte of v -> B words at dst (only the first `words` of them: a short run ends early)
    template <int B>
    __device__ __forceinline__ void squeeze_run(const uint32_t v[16], unsigned long long *dst, uint32_t words)
    {
      constexpr uint32_t m1 = (1u << B) - 1u, mPair = (m1 * 0x00010001u) << B;
      unsigned long long w[B];
#pragma unroll
      for (int i = 0; i < B; i++) w[i] = 0;
#pragma unroll
      for (int r = 0; r < 8; r++)
      { // 8 values -> 8 B bits = B bytes, at byte r B of the run's words (k_stream_pack_strips' squeeze_row, on values that sit in the LOW bits of their bytes)
        uint32_t z[2];
#pragma unroll
        for (int h = 0; h < 2; h++)
        {
          const uint32_t x = v[2 * r + h];
          const uint32_t y = ((x >> (8 - B)) & mPair) | (x & 0x00FF00FFu & (m1 * 0x00010001u)); // v0 | v1 << B in the low half, v2 | v3 << B in the high half
          z[h] = (y & 0xFFFFu) | ((y >> 16) << (2 * B));
        }
        const unsigned long long row = (unsigned long long)z[0] | ((unsigned long long)z[1] << (4 * B));
        constexpr int kBits = 8 * B;
        const int pos = r * kBits, idx = pos >> 6, sh = pos & 63;
        w[idx] |= row << sh;
        if (sh + kBits > 64) w[idx + 1] |= row >> (64 - sh);
      }
#pragma unroll
      for (int i = 0; i < B; i++)
        if ((uint32_t)i < words) dst[i] = w[i];
    }

    __global__ __launch_bounds__(256) void k_bstream_pack(const BlockedStreamParams p)
    {
      const uint32_t nRuns = p.units[p.nRegions];
      unsigned long long *const payload = reinterpret_cast<unsigned long long *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)p.nRegions * kRectEntry);
      for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < nRuns; u += gridDim.x * 256u)
      {
        // the rectangle of run u: the last r with units[r] <= u
        uint32_t lo = 0, hi = p.nRegions - 1u;
        while (lo < hi)
        {
          const uint32_t mid = (lo + hi + 1u) >> 1;
          if (p.units[mid] <= u) lo = mid; else hi = mid - 1u;
        }
        const uint32_t r = lo, run = u - p.units[r];
        const RegionDesc R = p.regions[r];
        const uint4 e3 = reinterpret_cast<const uint4 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)r * kRectEntry)[3]; // (k_bstream_sizes<true> wrote it)
        const uint32_t sw = e3.x, bits = entry_bits(sw);
        uint32_t wpx;
        const uint32_t n = rect_pixels(p.sizeX, p.sizeY, p.blocksX, p.blocksY, R.ox, R.oy, R.rx, R.ry, wpx);
        const uint32_t i0 = run * 64u, count = min(64u, n - i0);
        const uint8_t *nz = p.noise + p.noiseBase[r]; // the rectangle's dither calls back to back in A, B, C order, n bytes each
        unsigned long long *field = payload + e3.y;
#pragma unroll 1
        for (int k = 0; k < 3; k++)
        {
          const uint32_t s = (sw >> (8 * k)) & 0xFFu, b = (bits >> (8 * k)) & 0xFFu;
          const bool dithered = s != 0u && s < 8u;
          const uint8_t *noise = nz;
          if (dithered) nz += n;
          if (b == 0u) continue;
          uint32_t v[16];
          load_run(p.scratchFac + (size_t)k * p.scratchCap + R.scratch + i0, count, v);
          if (dithered)
          {
            uint32_t z[16];
            load_run(noise + i0, count, z);
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = dither_crush4(v[q], z[q], s); // (pixels beyond the rectangle's end read as factor 0, noise 0: their bits stay 0)
          }
          unsigned long long *dst = field + (size_t)run * b;
          const uint32_t words = field_words(count, b);
          switch (b)
          {
          case 1: squeeze_run<1>(v, dst, words); break;
          case 2: squeeze_run<2>(v, dst, words); break;
          case 3: squeeze_run<3>(v, dst, words); break;
          case 4: squeeze_run<4>(v, dst, words); break;
          case 5: squeeze_run<5>(v, dst, words); break;
          case 6: squeeze_run<6>(v, dst, words); break;
          case 7: squeeze_run<7>(v, dst, words); break;
          default: squeeze_run<8>(v, dst, words); break;
          }
          field += field_words(n, b);
        }
      }
    }
  }

  void launch_blocked_stream_pack(const BlockedStreamParams &p, int cus, hipStream_t s)
  {
    if (p.nRegions == 0) return;
    hipLaunchKernelGGL(k_bstream_sizes<false>, dim3(p.nTiles), dim3(kRectTile), 0, s, p);
    const StreamHeaderInfo info = { LIMG_HIP_STREAM_VERSION_BLOCKED, p.sizeX, p.sizeY, p.channels, p.errorFactor, p.blocksX, p.blocksY, p.flags | LIMG_HIP_STREAM_FLAG_MERGED,
                                    p.nRegions, (uint32_t)kRectEntry, p.nRegions };
    hipLaunchKernelGGL(k_stream_tile_scan<2>, dim3(1), dim3(1024), 0, s, p.tiles, p.nTiles, p.stream, info); // columns: payload words, runs (runs <= blocks)
    hipLaunchKernelGGL(k_bstream_sizes<true>, dim3(p.nTiles), dim3(kRectTile), 0, s, p);
    // one lane per run of 64 pixels; an image has at most blocks + rectangles runs.  Eight workgroups of four waves per CU, striding
    const uint64_t runsMax = (uint64_t)p.blocksX * p.blocksY + p.nRegions, need = (runsMax + 255u) / 256u, slots = (uint64_t)cus * 8u;
    hipLaunchKernelGGL(k_bstream_pack, dim3((uint32_t)(need < slots ? need : slots)), dim3(256), 0, s, p);
  }
}
