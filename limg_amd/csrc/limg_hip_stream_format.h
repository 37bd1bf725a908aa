// limg_hip_stream_format.h -- the rules of the "LMG3" stream (include/limg_hip.h) that both versions share, on the device: field widths, the header (writer and check),
// the one-workgroup scan over the packers' tile totals -- and, as named functions of the version 2 kernels (k_bstream_pack, k_bstream_window_decode), the dither + crush that
// produces the stored values and the reference's decoder arithmetic (a16) in 32-bit terms, and version 2's rectangle geometry (pixels, field sizes).  Included by
// limg_hip_stream.hip (version 1: 8x8 blocks), limg_hip_blocked_stream.hip (version 2: its packer) and limg_hip_stream_window.hip (window decode of both; all of version 2's decode).  k_blocked_store (limg_hip_blocked.hip) has the same dither and a16 written out in place (reason there); the
// packed-form decoders (decode_row_packed, phase_f_rows) are a different algorithm for a16's result and live with their kernels.
#ifndef LIMG_HIP_STREAM_FORMAT_H
#define LIMG_HIP_STREAM_FORMAT_H

#include "limg_hip_wave.h"

namespace limg_hip
{
  namespace
  {
    // ---- field widths ----------------------------------------------------------------------------------------------------------------
    // the alpha lanes (lane 3) of a record's vector pairs: mn3 of {dirA_min, dirB_offset, dirC_offset}, mx3 of {dirA_max, dirB_mag, dirC_mag}.
    // r0, r1, r2: {dirA_min, dirA_max}, {dirB_offset, dirB_mag}, {dirC_offset, dirC_mag} as 16 bytes each, the way records and entries hold them
    __device__ __forceinline__ void alpha_lanes(const uint4 &r0, const uint4 &r1, const uint4 &r2, int mn3[3], int mx3[3])
    {
      mn3[0] = (int)(int16_t)(r0.y >> 16); mn3[1] = (int)(int16_t)(r1.y >> 16); mn3[2] = (int)(int16_t)(r2.y >> 16);
      mx3[0] = (int)(int16_t)(r0.w >> 16); mx3[1] = (int)(int16_t)(r1.w >> 16); mx3[2] = (int)(int16_t)(r2.w >> 16);
    }

    // bits per pixel of the three factor fields + raw-escape mask (bA | bB << 8 | bC << 16 | rawMask << 24) from the shift triple and the alpha lanes: a factor
    // whose shift is 8 is kept as raw bytes where its alpha normal is non-zero (include/limg_hip.h)
    __device__ __forceinline__ uint32_t field_bits(uint32_t shiftWord, const int mn3[3], const int mx3[3], int channels)
    {
      uint32_t r = 0;
#pragma unroll
      for (int k = 0; k < 3; k++)
      {
        const uint32_t s = (shiftWord >> (8 * k)) & 0xFF;
        uint32_t b = s >= 8 ? 0u : 8u - s;
        if (s >= 8 && channels == 4 && mn3[k] != mx3[k]) { b = 8; r |= 1u << (24 + k); }
        r |= b << (8 * k);
      }
      return r;
    }

    // the bits per pixel from an entry's shift word, whose bits 24..26 say which factors are escaped
    // (k_stream_decode spells the same loop out in place)
    __device__ __forceinline__ uint32_t entry_bits(uint32_t sw)
    {
      uint32_t r = 0;
#pragma unroll
      for (int k = 0; k < 3; k++)
      {
        const uint32_t s = (sw >> (8 * k)) & 0xFFu;
        r |= (s >= 8u ? (((sw >> (24 + k)) & 1u) ? 8u : 0u) : 8u - s) << (8 * k);
      }
      return r;
    }

    // ---- version 2: a rectangle's pixels and field sizes (both decoders of limg_hip_blocked_stream.hip and limg_hip_stream_window.hip, and the packer) ------------
    constexpr int kRectEntry = 64;
    constexpr uint32_t kNoRect = 0xFFFFFFFFu;

    // pixels of a rectangle: 8 rx x 8 ry clipped to the image (src/limg.cpp:1722-1740)
    __device__ __forceinline__ uint32_t rect_pixels(uint32_t sizeX, uint32_t sizeY, uint32_t blocksX, uint32_t blocksY, uint32_t ox, uint32_t oy, uint32_t rx, uint32_t ry, uint32_t &wpx)
    {
      uint32_t hpx = ry * kBlock;
      wpx = rx * kBlock;
      if (ox + rx == blocksX && (sizeX % kBlock)) wpx = wpx - kBlock + sizeX % kBlock;
      if (oy + ry == blocksY && (sizeY % kBlock)) hpx = hpx - kBlock + sizeY % kBlock;
      return wpx * hpx;
    }

    __device__ __forceinline__ uint32_t field_words(uint32_t n, uint32_t b) { return (uint32_t)(((unsigned long long)n * b + 63ull) >> 6); }
    __device__ __forceinline__ uint32_t rect_words(uint32_t n, uint32_t bits) { return field_words(n, bits & 0xFFu) + field_words(n, (bits >> 8) & 0xFFu) + field_words(n, (bits >> 16) & 0xFFu); }

    // a word another launch or another workgroup of this one may have written (the decoders' verdict words)
    __device__ __forceinline__ uint32_t ld_volatile(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

    // ---- header --------------------------------------------------------------------------------------------------------------------------
    // what a packer knows before its scan has run: everything but the payload's size
    struct StreamHeaderInfo
    {
      uint32_t version, sizeX, sizeY, channels, errorFactor, blocksX, blocksY, flags;
      uint32_t nEntries, entryBytes; // the table: blocks x 56 (version 1), rectangles x 64 (version 2)
      uint32_t reserved0;            // version 2: the rectangle count
    };

    __device__ __forceinline__ void write_stream_header(uint8_t *stream, const StreamHeaderInfo &i, unsigned long long payloadWords)
    {
      limg_hip_stream_header h;
      h.magic = LIMG_HIP_STREAM_MAGIC; h.version = i.version;
      h.sizeX = i.sizeX; h.sizeY = i.sizeY; h.channels = i.channels; h.errorFactor = i.errorFactor;
      h.blocksX = i.blocksX; h.blocksY = i.blocksY;
      h.payloadWords = payloadWords;
      h.totalBytes = sizeof(limg_hip_stream_header) + (unsigned long long)i.nEntries * i.entryBytes + payloadWords * 8ull;
      h.flags = i.flags; h.reserved[0] = i.reserved0; h.reserved[1] = h.reserved[2] = 0;
      *reinterpret_cast<limg_hip_stream_header *>(stream) = h;
    }

    // The header a decoder is about to trust, against the call's own geometry and the size of the buffer it was handed.  P: DecodeParams / WindowDecodeParams / WindowGroup.
    template <class P>
    __device__ __forceinline__ bool stream_header_ok(const limg_hip_stream_header *h, uint32_t version, uint32_t entryBytes, uint32_t nEntries, const P &p)
    {
      return h->magic == LIMG_HIP_STREAM_MAGIC && h->version == version && h->sizeX == p.sizeX && h->sizeY == p.sizeY &&
             h->blocksX == p.blocksX && h->blocksY == p.blocksY && (h->channels == 3 || h->channels == 4) &&
             h->payloadWords <= (unsigned long long)p.nBlocks * 24ull && // 3 fields x 8 words at most per block: bounds the product below
             sizeof(limg_hip_stream_header) + (unsigned long long)nEntries * entryBytes + h->payloadWords * 8ull <= p.streamBytes;
    }

    // ---- the packers' scan ---------------------------------------------------------------------------------------------------------------
    // One workgroup: exclusive prefix, in place, of `nTiles` tile totals of COLS interleaved columns, then the header.  Column 0 is the payload words.
    // (an entry's payloadWord is 32 bits: the host refuses images whose worst-case payload would not fit -- limg_hip_stream_bound; the other columns are smaller)
    template <int COLS>
    __global__ __launch_bounds__(1024) void k_stream_tile_scan(uint32_t *tiles, uint32_t nTiles, uint8_t *stream, const StreamHeaderInfo info)
    {
      __shared__ unsigned long long sWave[COLS][16];
      __shared__ unsigned long long sCarry[COLS];
      const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
      if (tid < COLS) sCarry[tid] = 0;
      __syncthreads();
      for (uint32_t base = 0; base < nTiles; base += 1024)
      {
        const uint32_t i = base + tid;
        unsigned long long v[COLS], incl[COLS], pre[COLS];
#pragma unroll
        for (int c = 0; c < COLS; c++) incl[c] = v[c] = i < nTiles ? tiles[COLS * i + c] : 0u;
        // (wave_scan_inclusive of every column, one shuffle step of all of them at a time: the columns' chains are independent and overlap)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
        {
          unsigned long long up[COLS];
#pragma unroll
          for (int c = 0; c < COLS; c++) up[c] = __shfl_up(incl[c], off, 64);
          if (lane >= off)
#pragma unroll
            for (int c = 0; c < COLS; c++) incl[c] += up[c];
        }
        if (lane == 63)
#pragma unroll
          for (int c = 0; c < COLS; c++) sWave[c][wave] = incl[c];
        __syncthreads();
#pragma unroll
        for (int c = 0; c < COLS; c++) pre[c] = sCarry[c];
        for (int w = 0; w < wave; w++)
#pragma unroll
          for (int c = 0; c < COLS; c++) pre[c] += sWave[c][w];
        if (i < nTiles)
#pragma unroll
          for (int c = 0; c < COLS; c++) tiles[COLS * i + c] = (uint32_t)(pre[c] + incl[c] - v[c]);
        __syncthreads();
        if (tid == 1023)
#pragma unroll
          for (int c = 0; c < COLS; c++) sCarry[c] = pre[c] + incl[c];
        __syncthreads();
      }
      if (tid == 0) write_stream_header(stream, info, sCarry[0]);
    }

    // ---- stored values: dither + crush -----------------------------------------------------------------------------------------------
    // src/limg.cpp:824-879 for one factor byte at shift s (1..7): (noise & ditherSize) - ditherOffset, add, clamp, shift
    __device__ __forceinline__ uint32_t dither_crush(uint32_t f, uint32_t noise, uint32_t s)
    {
      int t = (int)f + ((int)(noise & ((1u << s) - 1u)) - (int)(1u << (s - 1)));
      t = t < 0 ? 0 : (t > 255 ? 255 : t);
      return (uint32_t)t >> s;
    }
    // ... for four of them, a byte each (a byte that holds factor 0 and noise 0 stays 0: 0 - offset clamps to 0)
    __device__ __forceinline__ uint32_t dither_crush4(uint32_t f4, uint32_t noise4, uint32_t s)
    {
      uint32_t out = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) out |= dither_crush((f4 >> (8 * q)) & 0xFFu, noise4 >> (8 * q), s) << (8 * q);
      return out;
    }

    // ---- a16: the reference's decoder in 32-bit terms (src/limg_decode.h:139-196 / :40-101) ---------------------------------------------------
    struct A16
    {
      int nn[3][4], mc[3][4]; // per factor and channel: normal, additive constant
      int mul[3];             // per factor: the re-expansion multiplier of its shift
    };
    // vec(k, c): lane c of the record's vector k (dirA_min, dirA_max, dirB_offset, dirB_mag, dirC_offset, dirC_mag).
    // (k_stream_decode prepares its own: its constants carry the packed form's biases and its multiplier is folded into the normals; sharing this one would take a
    //  flag that only that caller sets)
    template <class VEC>
    __device__ __forceinline__ A16 a16_constants(VEC &&vec, const uint32_t shift[3], int channels)
    {
      A16 k;
#pragma unroll
      for (int f = 0; f < 3; f++)
      {
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
          int nv = vec(2 * f + 1, c) - vec(2 * f, c), m = vec(2 * f, c);
          if (c < 3) { if (shift[f] > 7) { nv = 0; if (f > 0) m = 0; } }
          else if (channels == 3) { nv = 0; m = 0xFFFF; }
          k.nn[f][c] = nv;
          k.mc[f][c] = (int)(((uint32_t)m << 8) + 128u);
        }
        k.mul[f] = (int)shift_mul(shift[f]);
      }
      return k;
    }
    // one pixel from its three stored factor values
    __device__ __forceinline__ uint32_t a16_pixel(const A16 &k, uint32_t vA, uint32_t vB, uint32_t vC)
    {
      const int dA = (int)vA * k.mul[0], dB = (int)vB * k.mul[1], dC = (int)vC * k.mul[2];
      uint32_t decoded = 0;
#pragma unroll
      for (int c = 0; c < 4; c++)
      {
        int est = (mad_i24(dA, k.nn[0][c], k.mc[0][c]) >> 8) + (mad_i24(dB, k.nn[1][c], k.mc[1][c]) >> 8) + (mad_i24(dC, k.nn[2][c], k.mc[2][c]) >> 8);
        est = est < 0 ? 0 : (est > 255 ? 255 : est);
        decoded |= (uint32_t)est << (8 * c);
      }
      return decoded;
    }
  }
}

#endif
