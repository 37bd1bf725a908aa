// limg_hip_rate.hip -- the LMG3 stream's size probe: how long the version 1 stream of an image would be at an error factor, without encoding it.
//
// A stream is 64 + 56 blocks + 8 W bytes, W = the blocks' payload words; a block's words follow from its shift triple and its record's alpha lanes alone (field_bits,
// limg_hip_stream_format.h).  The records do not depend on the error factor and the shift triple depends on it only through the two thresholds, so one k_fit_tpb
// (the `fitOnly` route of encode_device) serves any number of probes, and a probe is the E step's front half -- strip staging, record load, phase-E view, per-pixel
// factors, the shift search (limg_hip_phase_e.h, limg_hip_search.h) -- with W summed instead of anything stored: no noise table, no look-back, no F step, no planes.
//
// k_rate_probe: one workgroup per work strip (32 blocks), wave = block, lane = pixel, as the E step.  Images of whole 8x8 blocks, the default search, records from
// k_fit_tpb.  The thresholds come from a small device-resident state, not from the kernel arguments, and a one-thread k_rate_step between two probes turns the
// counted words into the next thresholds: a list of error factors (limg_hip_stream_sizes*) or the search of limg_hip_rate_step.h (limg_hip_encode_stream_budget*).  So
// all launches of a call are enqueued at once, with no host round trip between them; probes behind the end of a search return at once.
// Progress: no workgroup waits for another one -- no look-back, no spin, no ticket; a workgroup's only global write is one 64-bit atomic add.
//
// The *_batch kernels are the same three for a LIST of same-shape images (limg_hip_encode_stream_budget_batch*): one RateDevice and one counter per image, one probe
// workgroup per (image, work strip) over records that run image after image, every image on a search of its own.  The probe's body is written once
// (rate_probe_strip) and takes what differs -- the image's pixels, state, counter and its block rows in the records -- as arguments.
//
// The *_list forms are the same for a chunk of images that differ in SHAPE (limg_hip_encode_stream_budget_list*, limg_hip_stream_sizes_list*; the chunk's layout:
// limg_hip_list_plan.h, its records: k_fit_tpb_list).  k_rate_probe_list: one workgroup per work strip of the chunk; the strip's image by the binary search over the
// strip prefix that k_encode_list_mixed uses, that image's geometry, access flag and slice starts from its ListImage entry (scalar loads, once per workgroup) as the
// view rate_probe_strip reads in place of the kernel arguments.  The begin and step kernels of a list take the ListImage table too: an image's fixed bytes are its own.
#include "limg_hip_phase_e.h"

namespace limg_hip
{
  namespace
  {
    // thresholds and flags of an error factor: the rule encode_params (limg_hip_encode.hip) applies on the host (limg_hip_encode_rules.h)
    __device__ __forceinline__ void set_thresholds(RateDevice *d, uint32_t errorFactor)
    {
      const Thresholds t = thresholds(errorFactor);
      d->maxPixel32 = t.maxPixel32; d->blockLimitFull = t.blockLimitFull; d->maxBlock = t.maxBlock; d->crushBits = t.crushBits;
    }

    // in front of a call's first probe: the search's state (or the list's position), the first thresholds, an empty counter
    __global__ void k_rate_begin(RateDevice *d, unsigned long long *counter, const RateState first, const uint32_t firstErrorFactor)
    {
      d->search = first;
      d->listNext = 0u;
      set_thresholds(d, firstErrorFactor);
      *counter = 0ull;
    }

    // between two probes, one image.  bytes from words: a stream is its fixed bytes (header + table) + 8 x the payload words just counted.  list == nullptr: the
    // search takes that size (rate_step) and names the next error factor, 2 h; otherwise the size goes to listBytes[i] and the list's next entry is set up.
    __device__ __forceinline__ void rate_step_image(RateDevice *d, unsigned long long *counter, const unsigned long long fixedBytes, const uint32_t *list,
                                                    unsigned long long *listBytes, const uint32_t listCount)
    {
      const unsigned long long bytes = fixedBytes + 8ull * *counter;
      *counter = 0ull;
      if (list)
      {
        const uint32_t i = d->listNext;
        if (i >= listCount) return;
        listBytes[i] = bytes;
        d->listNext = i + 1u;
        if (i + 1u < listCount) set_thresholds(d, list[i + 1u]);
        return;
      }
      if (d->search.done) return;
      rate_step(d->search, bytes);
      if (!d->search.done) set_thresholds(d, 2u * d->search.next);
    }

    __global__ void k_rate_step(RateDevice *d, unsigned long long *counter, const unsigned long long fixedBytes, const uint32_t *list, unsigned long long *listBytes,
                                const uint32_t listCount)
    {
      rate_step_image(d, counter, fixedBytes, list, listBytes, listCount);
    }

    // One work strip's probe: strip `strip` of block row `by` of the image whose pixels are io.in; byS: that row in p.records / p.invN.  P: RateProbeParams or
    // RateProbeBatchParams; everything but `lane`-derived values is wave-uniform.
    template <int CH, bool FAST, class P, class IO>
    __device__ __forceinline__ void rate_probe_strip(const P &p, const IO &io, const RateDevice *const st, unsigned long long *const counter, uint8_t *const lds,
                                                     const uint32_t strip, const uint32_t by, const uint32_t byS)
    {
      constexpr LdsLayout LL = lds_layout<true>();
      if (st->search.done) return; // (uniform: the step kernel in front of this launch wrote it)
      const uint32_t maxPixel32 = (uint32_t)sgpr((int)st->maxPixel32), blockLimit = (uint32_t)sgpr((int)st->blockLimitFull), crushBits = (uint32_t)sgpr((int)st->crushBits);
      const int tid = (int)threadIdx.x;
      EStrip g;
      g.tid = tid; g.lane = tid & 63; g.wave = tid >> 6;
      g.strip = strip; g.by = by; g.byS = byS;
      g.x0 = g.strip * (kStripBlocks * kBlock); g.y0 = g.by * kBlock;
      g.stripW = min(p.sizeX - g.x0, (uint32_t)(kStripBlocks * kBlock)); g.ry = (uint32_t)kBlock; // whole blocks
      g.pix = reinterpret_cast<uint32_t *>(lds + kLdsStrip); g.V = reinterpret_cast<float *>(lds + LL.v); g.blk = reinterpret_cast<BlkF *>(lds + LL.blk);
      g.calls = reinterpret_cast<uint32_t *>(lds + LL.calls); g.trialc = reinterpret_cast<int *>(lds + LL.trialc);
      const int lane = g.lane;

      uint32_t recVal[2] = { 0u, 0u };
      request_prefit_records(p, g, recVal);
      stage_strip_pixels(p, io, g);
      __syncthreads();
      take_prefit_records<false>(p, g, recVal, nullptr);
      phase_e_view<CH, FAST, true>(g);
      uint32_t *s_queue = g.calls + 4;
      if (tid == 0) *s_queue = 0;
      __syncthreads();

      // the strip's blocks from a queue, as phase E hands them out: the number of trials differs from block to block
      uint32_t waveWords = 0; // scalar
      auto grab = [&]() -> uint32_t { uint32_t v = 0; if (lane == 0) v = atomicAdd(s_queue, 1u); return (uint32_t)sgpr((int)v); };
      uint32_t sbNext = grab();
#pragma unroll 1
      for (;;)
      {
        const uint32_t sb = sbNext;
        if (sb >= (uint32_t)kStripBlocks) break;
        uint32_t qv = 0;
        if (lane == 0) qv = atomicAdd(s_queue, 1u);
        uint32_t rx, n, lx, ly;
        if (!block_geom(p, g, sb, rx, n)) { sbNext = (uint32_t)sgpr((int)qv); continue; }
        const BlkF *const blkE = g.blk + sb;
        uint32_t shift[3] = { 0, 0, 0 };
        if (p.forced[0] >= 0) { shift[0] = (uint32_t)p.forced[0]; shift[1] = (uint32_t)p.forced[1]; shift[2] = (uint32_t)p.forced[2]; }
        else if (crushBits)
        {
          const uint32_t px = block_pixel(g, sb, rx, n, lx, ly);
          uint32_t fA, fB, fC;
          pixel_factors<CH, FAST>(reinterpret_cast<const BlkE *>(blkE), px, fA, fB, fC);
          if (!((uint32_t)sgpr((int)blkE->flags) & kBig))
          { // the packed trial's state, as fit_search_strip sets it up for a whole block with the trial constants of phase_e_view
            TrialState t;
            t.fA = fA; t.fB = fB; t.fC = fC;
            const uint32_t R = px & 0xFF, G = (px >> 8) & 0xFF;
            t.hiRG = (R + 0x8000u) | ((G + 0x8000u) << 16);
            t.loRG = (R + 0x8000u - 255u) | ((G + 0x8000u - 255u) << 16);
            t.pxB = (int)((px >> 16) & 0xFF);
            t.pxBlo = t.pxB - 255;
            const int *tc = g.trialc + sb * kTrialConstDw;
#pragma unroll
            for (int c = 0; c < 3; c++)
            {
              t.nA[c] = tc[c]; t.nB[c] = tc[3 + c]; t.nC[c] = tc[6 + c];
              t.mA[c] = tc[9 + c]; t.mB[c] = tc[12 + c]; t.mC[c] = tc[15 + c];
            }
            t.mA[0] += (int)(R << 8); t.mA[1] += (int)(G << 8); t.mA[2] += t.pxB << 8;
            search_fast_automaton<true, false>(t, true, maxPixel32, blockLimit, shift); // (the limits come from device memory: the trial keeps its red-weight select)
          }
          else
          { // a record out of the packed trial's range: the generic 32-bit search, as phase E
            const uint32_t packed = (uint32_t)sgpr((int)search_generic(px, fA, fB, fC, blkE->rec, true, maxPixel32, st->maxBlock * 64ull, true));
            shift[0] = packed & 0xFF; shift[1] = (packed >> 8) & 0xFF; shift[2] = (packed >> 16) & 0xFF;
          }
        }
        // the block's payload words (finish_block's count; field_bits, limg_hip_stream_format.h): a field of 8 - shift bits per pixel is that many 8-byte words; a
        // factor at shift 8 has none unless its alpha normal is non-zero (raw-byte escape)
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
          const uint32_t sk = shift[k];
          if (sk < 8u) waveWords += 8u - sk;
          else if (CH == 4 && sgpr((int)blkE->rec[8 * k + 3]) != sgpr((int)blkE->rec[8 * k + 7])) waveWords += 8u;
        }
        sbNext = (uint32_t)sgpr((int)qv);
      }
      if (lane == 0) g.calls[g.wave] = waveWords;
      __syncthreads();
      if (tid == 0) atomicAdd(counter, (unsigned long long)(g.calls[0] + g.calls[1] + g.calls[2] + g.calls[3])); // <= 32 blocks x 24 words
    }

    template <int CH, bool FAST>
    __global__ __launch_bounds__(kThreads, 6) void k_rate_probe(const RateProbeParams p)
    {
      __shared__ __attribute__((aligned(16))) uint8_t lds[lds_layout<true>().total];
      rate_probe_strip<CH, FAST>(p, p.io, p.state, p.counter, lds, blockIdx.x % p.stripsX, blockIdx.x / p.stripsX, blockIdx.x / p.stripsX);
    }

    // ---- a list of images: one search per image ----
    // thread i: image i's search over [hLo, hHi] for its budget, the thresholds of its first probe (2 hHi), an empty counter.  list: the call measures a list of
    // error factors instead (limg_hip_stream_sizes_list*): no search, the thresholds of the list's first entry.
    __global__ void k_rate_begin_batch(RateDevice *d, unsigned long long *counters, const RateBudgetChunk budgets, const uint32_t hLo, const uint32_t hHi, const uint32_t *list)
    {
      const uint32_t i = threadIdx.x;
      if (i >= budgets.n) return;
      d[i].search = rate_begin(hLo, hHi, budgets.maxBytes[i]);
      d[i].listNext = 0u;
      set_thresholds(d + i, list ? list[0] : 2u * hHi);
      counters[i] = 0ull;
    }

    // thread i: the step of image i.  images == nullptr: a list of one shape, fixedBytes is every image's; else a chunk of mixed shapes, whose image i has the fixed
    // bytes of its own block count (header + table: limg_hip_stream_header, limg_hip_stream_block).  list: the list form, image i's sizes at listBytes[i * listCount + k].
    __global__ void k_rate_step_batch(RateDevice *d, unsigned long long *counters, const uint32_t nImages, const unsigned long long fixedBytes, const ListImage *images,
                                      const uint32_t *list, unsigned long long *listBytes, const uint32_t listCount)
    {
      const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
      if (i >= nImages) return;
      const unsigned long long fixed = images ? sizeof(limg_hip_stream_header) + (unsigned long long)images[i].nBlocks * sizeof(limg_hip_stream_block) : fixedBytes;
      rate_step_image(d + i, counters + i, fixed, list, list ? listBytes + (size_t)i * listCount : nullptr, listCount);
    }

    // One workgroup per (image, work strip); the image index is wave-uniform, and the image's pixels come from its entry of the device table through the constant
    // address space (scalar loads, as the persistent kernel's io_of).  A workgroup of an image whose search is over returns at its first load.
    template <int CH, bool FAST>
    __global__ __launch_bounds__(kThreads, 6) void k_rate_probe_batch(const RateProbeBatchParams p)
    {
      __shared__ __attribute__((aligned(16))) uint8_t lds[lds_layout<true>().total];
      const uint32_t img = blockIdx.x / p.imageStrips, local = blockIdx.x - img * p.imageStrips; // (the grid is nImages * imageStrips workgroups)
      typedef const __attribute__((address_space(4))) ImageIO KernIO;
      KernIO *const io = (KernIO *)p.batch + img;
      const uint32_t by = local / p.stripsX;
      rate_probe_strip<CH, FAST>(p, *io, p.states + img, p.counters + img, lds, local - by * p.stripsX, by, img * p.blocksY + by);
    }

    // ---- a chunk of images of mixed shapes ----
    // what rate_probe_strip reads as `p`, built from one image's ListImage entry: records and invN start at the image's first block, so its rows count from 0
    struct RateProbeView
    {
      uint32_t sizeX, sizeY, blocksX, blocksY, stripsX;
      int32_t vecIn;
      int32_t recordLimit;
      int32_t forced[3];
      const limg_hip_block_record *records;
      const float *invN;
    };

    // One workgroup per work strip of the chunk (the grid is the chunk's strip total).  Everything of the view is wave-uniform and comes through the constant address
    // space: the tables were written by launches that precede this one on the stream.  A workgroup of an image whose search is over returns at its first load.
    template <int CH, bool FAST>
    __global__ __launch_bounds__(kThreads, 6) void k_rate_probe_list(const RateProbeListParams p)
    {
      __shared__ __attribute__((aligned(16))) uint8_t lds[lds_layout<true>().total];
      typedef const __attribute__((address_space(4))) ListImage KernImage;
      typedef const __attribute__((address_space(4))) ImageIO KernIO;
      if (blockIdx.x >= p.nStrips) return;
      const uint32_t img = find_strip_image(p.firstStrip, p.nImages, blockIdx.x);
      if (p.states[img].search.done) return;
      KernImage *const im = (KernImage *)(uintptr_t)p.images + img;
      KernIO *const io = (KernIO *)(uintptr_t)p.batch + img;
      RateProbeView v;
      v.sizeX = im->sizeX; v.sizeY = im->sizeY; v.blocksX = im->blocksX; v.blocksY = im->blocksY; v.stripsX = im->stripsX;
      v.vecIn = (im->vec & kListVecIn) ? 1 : 0; // of THIS image
      v.recordLimit = p.recordLimit;
      v.forced[0] = p.forced[0]; v.forced[1] = p.forced[1]; v.forced[2] = p.forced[2];
      v.records = p.records + im->firstBlock; v.invN = p.invN + 4 * im->firstBlock;
      const uint32_t local = blockIdx.x - im->firstStrip, by = local / v.stripsX;
      rate_probe_strip<CH, FAST>(v, *io, p.states + img, p.counters + img, lds, local - by * v.stripsX, by, by);
    }
  } // namespace

  void launch_rate_begin(RateDevice *dState, unsigned long long *dCounter, const RateState &first, uint32_t firstErrorFactor, hipStream_t s)
  {
    hipLaunchKernelGGL(k_rate_begin, dim3(1), dim3(1), 0, s, dState, dCounter, first, firstErrorFactor);
  }

  void launch_rate_step(RateDevice *dState, unsigned long long *dCounter, uint64_t fixedBytes, const uint32_t *dList, unsigned long long *dListBytes, uint32_t listCount,
                        hipStream_t s)
  {
    hipLaunchKernelGGL(k_rate_step, dim3(1), dim3(1), 0, s, dState, dCounter, (unsigned long long)fixedBytes, dList, dListBytes, listCount);
  }

  void launch_rate_probe(const RateProbeParams &p, int channels, bool floatFast, hipStream_t s)
  {
    const dim3 grid(p.stripsX * p.blocksY), block(kThreads);
    with_flags([&](auto rgba, auto fast) { hipLaunchKernelGGL((k_rate_probe<rgba ? 4 : 3, fast>), grid, block, 0, s, p); }, channels == 4, floatFast);
  }

  void launch_rate_begin_batch(RateDevice *dStates, unsigned long long *dCounters, const uint64_t *hMaxBytes, size_t count, uint32_t hLo, uint32_t hHi, hipStream_t s,
                               const uint32_t *dList)
  {
    for (size_t i0 = 0; i0 < count; i0 += 64)
    { // the budgets through kernel arguments: stream-ordered, and the host array may die right away
      RateBudgetChunk ch;
      ch.n = (uint32_t)(count - i0 < 64 ? count - i0 : 64);
      for (uint32_t i = 0; i < 64; i++) ch.maxBytes[i] = hMaxBytes && i < ch.n ? (unsigned long long)hMaxBytes[i0 + i] : 0ull;
      hipLaunchKernelGGL(k_rate_begin_batch, dim3(1), dim3(64), 0, s, dStates + i0, dCounters + i0, ch, hLo, hHi, dList);
    }
  }

  void launch_rate_step_batch(RateDevice *dStates, unsigned long long *dCounters, uint32_t nImages, uint64_t fixedBytes, hipStream_t s, const ListImage *dImages,
                              const uint32_t *dList, unsigned long long *dListBytes, uint32_t listCount)
  {
    hipLaunchKernelGGL(k_rate_step_batch, dim3((nImages + 63u) / 64u), dim3(64), 0, s, dStates, dCounters, nImages, (unsigned long long)fixedBytes, dImages, dList, dListBytes,
                       listCount);
  }

  void launch_rate_probe_batch(const RateProbeBatchParams &p, int channels, bool floatFast, hipStream_t s)
  {
    const dim3 grid(p.nImages * p.imageStrips), block(kThreads);
    with_flags([&](auto rgba, auto fast) { hipLaunchKernelGGL((k_rate_probe_batch<rgba ? 4 : 3, fast>), grid, block, 0, s, p); }, channels == 4, floatFast);
  }

  void launch_rate_probe_list(const RateProbeListParams &p, int channels, bool floatFast, hipStream_t s)
  {
    const dim3 grid(p.nStrips), block(kThreads);
    with_flags([&](auto rgba, auto fast) { hipLaunchKernelGGL((k_rate_probe_list<rgba ? 4 : 3, fast>), grid, block, 0, s, p); }, channels == 4, floatFast);
  }
} // namespace limg_hip
