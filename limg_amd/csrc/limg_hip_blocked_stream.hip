// limg_hip_blocked_stream.hip -- version 2 of the "LMG3" stream: the merged-block encoder's rectangles (format: include/limg_hip.h).
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
// Decode:
//   k_bstream_map           validates the table and scatters it into a block -> rectangle map: 64 rectangles per wave step, a lane claims the blocks of a small
//                           rectangle itself (atomicCAS on ~0), the wave claims a large one together; the claimed blocks are counted
//   k_bstream_decode        refuses unless every block was claimed and nothing was flagged; then lane = (block j = lane & 7, block row r = lane >> 3) over units of 8
//                           consecutive blocks: the lane's 8 pixels are the bit run at ((y - 8 oy) * wpx + (x - 8 ox)) * b of each field of the block's rectangle; the
//                           integer decode is a16_constants / a16_pixel, as in k_blocked_store; a wave's stores are 8 row pieces of 256 contiguous bytes.
// Nothing here reads through an offset the map kernel has not checked against the stream's size.
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

    // ---- decode ----------------------------------------------------------------------------------------------------------------------
    __device__ __forceinline__ void refuse(const BlockedDecodeParams &p, uint32_t bit)
    {
      atomicOr(p.state + 1, 1u);
      atomicOr(p.status, bit);
    }

    __global__ __launch_bounds__(256) void k_bstream_map(const BlockedDecodeParams p)
    {
      const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
      const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(p.stream);
      const unsigned long long payloadWords = h->payloadWords;
      const uint32_t nRects = h->reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES];
      if (!(nRects >= 1u && nRects <= p.nBlocks && stream_header_ok(h, LIMG_HIP_STREAM_VERSION_BLOCKED, kRectEntry, nRects, p)))
      {
        if (tid == 0 && blockIdx.x == 0) refuse(p, 1u);
        return;
      }
      uint32_t claimed = 0;
      for (uint32_t base = (blockIdx.x * 4u + (uint32_t)wave) * 64u; base < nRects; base += gridDim.x * 256u)
      {
        if (ld_volatile(p.state + 1) != 0u) break; // refused already (all lanes read the same word: wave-uniform)
        const uint32_t r = base + (uint32_t)lane;
        uint32_t ox = 0, oy = 0, rx = 0, ry = 0;
        bool good = false;
        if (r < nRects)
        {
          const uint4 e3 = reinterpret_cast<const uint4 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)r * kRectEntry)[3];
          ox = e3.z & 0xFFFFu; oy = e3.z >> 16; rx = e3.w & 0xFFFFu; ry = e3.w >> 16;
          const uint32_t sw = e3.x;
          good = rx >= 1u && ry >= 1u && ox + rx <= p.blocksX && oy + ry <= p.blocksY && (sw & 0xFFu) <= 8u && ((sw >> 8) & 0xFFu) <= 8u && ((sw >> 16) & 0xFFu) <= 8u;
          if (good)
          {
            uint32_t wpx;
            const uint32_t n = rect_pixels(p.sizeX, p.sizeY, p.blocksX, p.blocksY, ox, oy, rx, ry, wpx);
            good = (unsigned long long)e3.y + rect_words(n, entry_bits(sw)) <= payloadWords; // (a field is at most n / 8 + 1 words, three of them far below 2^32)
          }
          if (!good) refuse(p, 2u);
        }
        const uint32_t nb = good ? rx * ry : 0u;
        bool clash = false;
        if (nb >= 1u && nb <= 4u)
        { // a small rectangle: its lane claims it
          for (uint32_t i = 0; i < nb; i++)
          {
            const uint32_t dy = i / rx, dx = i - dy * rx;
            if (atomicCAS(p.map + (size_t)(oy + dy) * p.blocksX + ox + dx, kNoRect, r) != kNoRect) { clash = true; break; }
            claimed++;
          }
        }
        // the large ones, one after the other, by the whole wave; a block that is taken already ends the rectangle (and the stream): the work is bounded by the blocks
        unsigned long long big = __builtin_amdgcn_ballot_w64(nb > 4u);
        while (big != 0ull && __builtin_amdgcn_ballot_w64(clash) == 0ull)
        {
          const int src = __builtin_ctzll(big);
          big &= big - 1ull;
          const uint32_t box = (uint32_t)__shfl((int)ox, src, 64), boy = (uint32_t)__shfl((int)oy, src, 64), brx = (uint32_t)__shfl((int)rx, src, 64),
                         bnb = (uint32_t)__shfl((int)nb, src, 64);
          for (uint32_t i0 = 0; i0 < bnb && __builtin_amdgcn_ballot_w64(clash) == 0ull; i0 += 64u)
          {
            const uint32_t i = i0 + (uint32_t)lane;
            if (i < bnb)
            {
              const uint32_t dy = i / brx, dx = i - dy * brx;
              if (atomicCAS(p.map + (size_t)(boy + dy) * p.blocksX + box + dx, kNoRect, base + (uint32_t)src) != kNoRect) clash = true;
              else claimed++;
            }
          }
        }
        if (clash) refuse(p, 2u);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) claimed += (uint32_t)__shfl_xor((int)claimed, off, 64);
      if (lane == 0 && claimed) atomicAdd(p.state, claimed);
    }

    __global__ __launch_bounds__(256) void k_bstream_decode(const BlockedDecodeParams p)
    {
      const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
      // the verdict of k_bstream_map: nothing flagged and every block claimed exactly once (claims never overlap, so the count says it)
      if (ld_volatile(p.state + 1) != 0u || ld_volatile(p.state) != p.nBlocks)
      {
        if (tid == 0 && blockIdx.x == 0) atomicOr(p.status, 2u);
        return;
      }
      const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(p.stream);
      const uint32_t nRects = h->reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES], channels = h->channels;
      const unsigned long long tableEnd = sizeof(limg_hip_stream_header) + (unsigned long long)nRects * kRectEntry, total = tableEnd + h->payloadWords * 8ull;
      const uint32_t unitsX = (p.blocksX + 7u) / 8u, nUnits = unitsX * p.blocksY;
      const uint32_t j = (uint32_t)lane & 7u, row = (uint32_t)lane >> 3;
      const bool rowAligned = (p.sizeX & 3u) == 0;
      for (uint32_t unit = blockIdx.x * 4u + (uint32_t)wave; unit < nUnits; unit += gridDim.x * 4u)
      {
        const uint32_t by = unit / unitsX, bx = (unit - by * unitsX) * 8u + j;
        const uint32_t y = by * 8u + row, x0 = bx * 8u;
        if (bx >= p.blocksX || y >= p.sizeY) continue;
        const uint32_t rect = p.map[(size_t)by * p.blocksX + bx];
        if (rect >= nRects) continue; // (cannot happen after the check above; a lane never indexes the table with anything else)
        const uint4 *ep = reinterpret_cast<const uint4 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)rect * kRectEntry);
        const uint4 e0 = ep[0], e1 = ep[1], e2 = ep[2], e3 = ep[3];
        const uint32_t ev[12] = { e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x, e2.y, e2.z, e2.w };
        const uint32_t sw = e3.x, ox = e3.z & 0xFFFFu, oy = e3.z >> 16, rx = e3.w & 0xFFFFu, ry = e3.w >> 16;
        uint32_t wpx;
        const uint32_t n = rect_pixels(p.sizeX, p.sizeY, p.blocksX, p.blocksY, ox, oy, rx, ry, wpx);
        const uint32_t cnt = min(8u, p.sizeX - x0);
        const unsigned long long i0 = (unsigned long long)(y - oy * 8u) * wpx + (x0 - ox * 8u);
        const uint32_t bits = entry_bits(sw);
        // the lane's 8 values of each field: the bit run at i0 * b
        unsigned long long packed[3];
        uint32_t bb[3], shift[3];
        unsigned long long fieldByte = tableEnd + (unsigned long long)e3.y * 8ull;
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
          const uint32_t b = (bits >> (8 * k)) & 0xFFu;
          bb[k] = b; shift[k] = (sw >> (8 * k)) & 0xFFu;
          packed[k] = 0;
          if (b)
          {
            const unsigned long long bit = i0 * b, byte = fieldByte + (bit >> 3), at = byte & ~3ull;
            const uint32_t sh = (uint32_t)(byte & 3ull) * 8u + (uint32_t)(bit & 7ull); // < 32
            // three aligned dwords hold the run's 64 bits wherever it starts; the last may lie beyond the stream's end (never beyond the field's: it is not used then)
            const uint32_t *wp = reinterpret_cast<const uint32_t *>(p.stream + at);
            const uint32_t d0 = at + 4ull <= total ? wp[0] : 0u, d1 = at + 8ull <= total ? wp[1] : 0u, d2 = at + 12ull <= total ? wp[2] : 0u;
            const unsigned long long lo = ((unsigned long long)d1 << 32) | d0;
            packed[k] = sh ? ((lo >> sh) | ((unsigned long long)d2 << (64u - sh))) : lo;
            fieldByte += (unsigned long long)field_words(n, b) * 8ull;
          }
        }
        const A16 k = a16_constants([&](int v, int c) { return (int)(int16_t)(ev[2 * v + (c >> 1)] >> (16 * (c & 1))); }, shift, (int)channels);
        uint32_t px[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
          px[i] = a16_pixel(k, (uint32_t)(packed[0] >> (i * bb[0])) & ((1u << bb[0]) - 1u), (uint32_t)(packed[1] >> (i * bb[1])) & ((1u << bb[1]) - 1u),
                            (uint32_t)(packed[2] >> (i * bb[2])) & ((1u << bb[2]) - 1u));
        uint32_t *dst = p.out + (size_t)y * p.sizeX + x0;
        if (cnt == 8u && rowAligned)
        { // a wave's stores: 8 row pieces of 8 x 32 contiguous bytes
          reinterpret_cast<uint4 *>(dst)[0] = make_uint4(px[0], px[1], px[2], px[3]);
          reinterpret_cast<uint4 *>(dst)[1] = make_uint4(px[4], px[5], px[6], px[7]);
        }
        else
        {
#pragma unroll
          for (int i = 0; i < 8; i++)
            if ((uint32_t)i < cnt) dst[i] = px[i];
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

  void launch_blocked_stream_decode(const BlockedDecodeParams &p, int cus, hipStream_t s)
  {
    const uint32_t slots = (uint32_t)cus * 8u;
    const uint32_t needMap = (p.nBlocks + 255u) / 256u; // at most nBlocks rectangles, 64 per wave
    hipLaunchKernelGGL(k_bstream_map, dim3(needMap < slots ? needMap : slots), dim3(256), 0, s, p);
    const uint32_t units = ((p.blocksX + 7u) / 8u) * p.blocksY, need = (units + 3u) / 4u;
    hipLaunchKernelGGL(k_bstream_decode, dim3(need < slots ? need : slots), dim3(256), 0, s, p);
  }
}
