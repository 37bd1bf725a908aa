// limg_hip_stream_splice.hip -- stream splice: a version 1 "LMG3" stream assembled from rectangles of 8x8 blocks of version 1 streams (crop, join, tile assembly)
// without decoding a pixel.  A block is self-contained -- its 56-byte entry holds record, shift word and payloadWord, its payload is bA + bB + bC whole words -- so
// the output's block is the source's block with payloadWord rebased, and the result decodes to the source's pixels bit for bit.
//
// The host (limg_hip_splice_plan.h) has checked the geometry and cut the pieces into RUNS, one block row of one piece each, in the output's raster order.  Inside
// a run entries and payload are contiguous in the source (payloadWord is the raster-order exclusive prefix of the blocks' words) and in the output.  Three launches,
// whatever the pieces are:
//   k_splice_measure   a wave per run, 64 blocks at a time: the entries' shift words give the blocks' words, a wave scan checks that every payloadWord is the
//                      run's start + the words before it (the sources are untrusted: all of it in 64 bits) and that the run ends inside the payload; the run's
//                      words go to totals[run].  The source's header is checked by every run that reads it.  A refusal raises the context's status word and the
//                      call's own fail word.
//   k_stream_tile_scan the packers' scan (limg_hip_stream_format.h; launch_stream_scan of limg_hip_stream.hip, where its one instance lives) over the runs' totals:
//                      where each run's payload starts in the output, and the header.
//   k_splice_copy      a wave per item of up to 64 blocks of a run: the entries as 8-byte words with payloadWord moved by (output start - source start), the
//                      payload as one range of 8-byte words, lane after lane.  A call that failed copies nothing and takes its header back.
// Context memory: the run table and a word per run.  Plain vector loads and stores only.
#include "limg_hip_stream_format.h"
#include "limg_hip_splice_plan.h"

namespace limg_hip
{
  namespace
  {
    constexpr int kEntry = 56;
    static_assert(kSpliceItemBlocks == 64u, "k_splice_copy: an item is what one wave copies, lane == block where it reads an entry");

    __device__ __forceinline__ uint32_t words_of(uint32_t bits) { return (bits & 0xFF) + ((bits >> 8) & 0xFF) + ((bits >> 16) & 0xFF); }
    // a pointer read from a table in memory is device memory: global loads and stores, not the generic ones the compiler would emit for it
    template <class T>
    __device__ __forceinline__ T *as_global(T *q) { return (T *)(__attribute__((address_space(1))) T *)q; }

    __global__ __launch_bounds__(256) void k_splice_measure(const SpliceParams p)
    {
      const int lane = lane_id(), wave = threadIdx.x >> 6;
      for (uint32_t run = blockIdx.x * 4u + (uint32_t)wave; run < p.nRuns; run += gridDim.x * 4u) // (wave-uniform)
      {
        const SpliceRun r = p.runs[run];
        SpliceSource s = p.sources[r.piece];
        s.stream = as_global(s.stream);
        // (the host has checked: streamBytes holds a header, and the run lies inside the block grid of s.sizeX x s.sizeY; the table's extent: stream_header_ok)
        const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(s.stream);
        uint32_t bad = stream_header_ok(h, LIMG_HIP_STREAM_VERSION, kEntry, s.nBlocks, s) && h->channels == p.channels ? 0u : 1u;
        unsigned long long total = 0;
        if (!bad)
        {
          const unsigned long long payloadWords = h->payloadWords;
          const uint2 *tail = reinterpret_cast<const uint2 *>(s.stream + sizeof(limg_hip_stream_header) + (size_t)r.srcEntry * kEntry) + 6; // an entry's {shift, payloadWord}
          unsigned long long start = 0;
          for (uint32_t k0 = 0; k0 < r.count; k0 += 64u)
          {
            const uint32_t k = k0 + (uint32_t)lane;
            const bool valid = k < r.count;
            const uint2 e = valid ? tail[(size_t)k * (kEntry / 8)] : make_uint2(0u, 0u);
            const uint32_t words = valid ? words_of(entry_bits(e.x)) : 0u;
            const uint32_t incl = wave_scan_inclusive(words, lane);
            if (k0 == 0) start = (uint32_t)__shfl((int)e.y, 0, 64);
            // canonical: this block's payload begins where the run's begins plus the words of the blocks before it
            const unsigned long long expect = start + total + (incl - words);
            if (__builtin_amdgcn_ballot_w64(valid && (unsigned long long)e.y != expect) != 0) { bad = 2u; break; } // (wave-uniform)
            total += (uint32_t)__shfl((int)incl, 63, 64);
          }
          if (!bad && start + total > payloadWords) bad = 2u;
        }
        if (lane == 0)
        {
          p.totals[run] = bad ? 0u : (uint32_t)total; // (at most 24 words a block: the host has bounded the block count)
          if (bad) { atomicOr(p.status, bad); atomicOr(p.fail, bad); }
        }
      }
    }

    // base[i] <= x < base[i + 1] (no slot is empty); x is wave-uniform
    __device__ __forceinline__ uint32_t find_slot(const uint32_t *__restrict__ base, uint32_t n, uint32_t x)
    {
      uint32_t lo = 0, hi = n;
      while (hi - lo > 1u)
      {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid] <= x) lo = mid; else hi = mid;
      }
      return lo;
    }

    __global__ __launch_bounds__(256) void k_splice_copy(const SpliceParams p)
    {
      const int lane = lane_id(), wave = threadIdx.x >> 6;
      if (*p.fail != 0u)
      { // a source was refused: nothing is copied, and the header the scan wrote goes (totalBytes 0: no stream)
        if (blockIdx.x == 0 && threadIdx.x < sizeof(limg_hip_stream_header) / 4) reinterpret_cast<uint32_t *>(p.out)[threadIdx.x] = 0u;
        return;
      }
      uint2 *outPayload = reinterpret_cast<uint2 *>(p.out + sizeof(limg_hip_stream_header) + (size_t)p.nBlocks * kEntry);
      for (uint32_t item = blockIdx.x * 4u + (uint32_t)wave; item < p.nItems; item += gridDim.x * 4u) // (wave-uniform)
      {
        const uint32_t run = find_slot(p.itemBase, p.nRuns, item);
        const SpliceRun r = p.runs[run];
        SpliceSource s = p.sources[r.piece];
        s.stream = as_global(s.stream);
        const uint32_t k0 = (item - p.itemBase[run]) * kSpliceItemBlocks, n = min(kSpliceItemBlocks, r.count - k0);
        const uint2 *srcE = reinterpret_cast<const uint2 *>(s.stream + sizeof(limg_hip_stream_header) + (size_t)r.srcEntry * kEntry);
        uint2 *dstE = reinterpret_cast<uint2 *>(p.out + sizeof(limg_hip_stream_header) + (size_t)r.dstEntry * kEntry);
        // (everything below was checked by k_splice_measure: the run's payloadWords are its start + a prefix, and start + words <= the source's payloadWords)
        const uint32_t srcStart = srcE[6].y, dstStart = p.totals[run], runWords = p.totals[run + 1u] - dstStart, delta = dstStart - srcStart;
        const uint32_t w0 = srcE[(size_t)k0 * 7u + 6u].y, w1 = k0 + n < r.count ? srcE[(size_t)(k0 + n) * 7u + 6u].y : srcStart + runWords;

        { // the entries: n x 7 words of 8 bytes, the seventh of each holding payloadWord in its high half
          const uint2 *se = srcE + (size_t)k0 * 7u;
          uint2 *de = dstE + (size_t)k0 * 7u;
          const uint32_t nw = n * 7u;
          uint2 v[7];
#pragma unroll
          for (uint32_t i = 0; i < 7u; i++)
          {
            const uint32_t w = (uint32_t)lane + 64u * i;
            v[i] = w < nw ? se[w] : make_uint2(0u, 0u);
          }
#pragma unroll
          for (uint32_t i = 0; i < 7u; i++)
          {
            const uint32_t w = (uint32_t)lane + 64u * i;
            if (w % 7u == 6u) v[i].y += delta;
            if (w < nw) de[w] = v[i];
          }
        }
        { // the payload: words [w0, w1) of the source to the same words moved by delta
          const uint2 *sp = reinterpret_cast<const uint2 *>(s.stream + sizeof(limg_hip_stream_header) + (size_t)s.nBlocks * kEntry) + w0;
          uint2 *dp = outPayload + (uint32_t)(w0 + delta);
          const uint32_t nw = w1 - w0;
          for (uint32_t base = 0; base < nw; base += 256u)
          {
            uint2 v[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++)
            {
              const uint32_t w = base + (uint32_t)lane + 64u * i;
              v[i] = w < nw ? sp[w] : make_uint2(0u, 0u);
            }
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++)
            {
              const uint32_t w = base + (uint32_t)lane + 64u * i;
              if (w < nw) dp[w] = v[i];
            }
          }
        }
      }
    }
  }

  void launch_stream_splice(const SpliceParams &p, int cus, hipStream_t s)
  {
    const uint32_t cap = (uint32_t)cus * 16u;
    k_splice_measure<<<std::min((p.nRuns + 3u) / 4u, cap), 256, 0, s>>>(p);
    launch_stream_scan(p.totals, p.nRuns + 1u, p.out, p.sizeX, p.sizeY, p.channels, p.errorFactor, p.flags, s); // (the entry behind the last run: the payload's size)
    k_splice_copy<<<std::min((p.nItems + 3u) / 4u, cap), 256, 0, s>>>(p);
  }
}
