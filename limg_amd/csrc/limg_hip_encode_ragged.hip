// limg_hip_encode_ragged.hip -- the 8x8 encode of images with partial edge blocks: the split path's kernels around a dither chain the host walks.
// Partial edge blocks make the chain walk depend on each block's pixel count (a call over N pixels is N / 8 AES rounds + N % 8 PCG steps: G_N), so it is
// evaluated in raster order on the host from the per-block call counts.  What crosses PCIe: the shift words down, then -- through pinned staging -- the
// strips' first call indices and, per dither call, the chain value it starts from and its pixel count (9 bytes; k_noise_expand turns them into the call's
// 64 noise bytes on the device; rounds 1-3 uploaded the 64 bytes).
#include "limg_hip_context.h"

using namespace limg_hip;

namespace
{
  // pinned staging of the ragged paths' host step (c->host.stage): shift words | previous descriptor | strip bases | per call: chain value, pixel count (worst case:
  // 3 calls per block)
  struct RaggedStage
  {
    size_t maxCalls, offPrev, offBase, offStates, offPixels, bytes;
    uint32_t *shifts = nullptr;
    unsigned long long *prev = nullptr;
    uint32_t *base = nullptr;
    unsigned long long *states = nullptr;
    uint8_t *pixels = nullptr;
    RaggedStage(size_t blocks, size_t strips) : maxCalls(blocks * 3)
    {
      offPrev = (blocks * 4 + 15) & ~(size_t)15; offBase = offPrev + 16; offStates = (offBase + strips * 4 + 15) & ~(size_t)15; offPixels = offStates + maxCalls * 8;
      bytes = offPixels + maxCalls + 16;
    }
    RaggedStage(size_t blocks, size_t strips, void *p) : RaggedStage(blocks, strips)
    {
      shifts = (uint32_t *)p;
      prev = (unsigned long long *)((uint8_t *)p + offPrev);
      base = (uint32_t *)((uint8_t *)p + offBase);
      states = (unsigned long long *)((uint8_t *)p + offStates);
      pixels = (uint8_t *)p + offPixels;
    }
  };

  // the previous ragged encode's H2D copies out of the staging buffer were asynchronous -- possibly on another stream: they must have read it before it is rewritten
  // or reallocated
  limg_hip_result ensure_stage(EncodeJob &e)
  {
    limg_hip_context *const c = e.c;
    if (c->host.stageBusy) { HIP_TRY(hipEventSynchronize(c->host.stageEvent)); c->host.stageBusy = false; }
    return c->host.stage.ensure(RaggedStage(e.blocks, e.strips).bytes);
  }

  // the staging buffer is the context's: the event marks the point where this encode's copies have read it (waited for by the next encode that uses it, on
  // whatever stream; the context goes only once the device is idle)
  limg_hip_result release_stage(EncodeJob &e)
  {
    limg_hip_context *const c = e.c;
    const limg_hip_result r = c->host.stageEvent.ensure(hipEventDisableTiming);
    if (r != limg_hip_success) return r;
    HIP_TRY(hipEventRecord(c->host.stageEvent, e.stream));
    c->host.stageBusy = true;
    return limg_hip_success;
  }

  // device side: per dither call 64 noise bytes + the 9 bytes they are expanded from (c->noise.dyn, c->noise.states); the F step reads the noise from there
  limg_hip_result size_noise_calls(EncodeJob &e, size_t calls)
  {
    limg_hip_context *const c = e.c;
    limg_hip_result r;
    if ((r = c->noise.dyn.ensure((calls + 1) * 64)) != limg_hip_success) return r;
    if ((r = c->noise.states.ensure(calls * 9 + 16)) != limg_hip_success) return r;
    e.p.noise = (const uint8_t *)c->noise.dyn.p;
    e.p.noiseLast = (uint32_t)calls; // (entry `calls` exists: the clamp of a call index cannot land outside the buffer)
    return limg_hip_success;
  }

  // dither calls [call0, call0 + n) of the walk: their chain values and pixel counts up, k_noise_expand makes their noise bytes
  limg_hip_result upload_calls(EncodeJob &e, const RaggedStage &h, size_t calls, size_t call0, size_t n)
  {
    limg_hip_context *const c = e.c;
    if (!n) return limg_hip_success;
    unsigned long long *dStates = (unsigned long long *)c->noise.states.p;
    uint8_t *dPixels = (uint8_t *)c->noise.states.p + calls * 8;
    HIP_TRY(hipMemcpyAsync(dStates + call0, h.states + call0, n * 8, hipMemcpyHostToDevice, e.stream));
    HIP_TRY(hipMemcpyAsync(dPixels + call0, h.pixels + call0, n, hipMemcpyHostToDevice, e.stream));
    launch_noise_expand((uint8_t *)c->noise.dyn.p + call0 * 64, dStates + call0, dPixels + call0, n, c->opt.dither_pcg != 0, e.stream);
    return limg_hip_success;
  }

  // band b of a banded encode as a sub-image: pointers advanced, block rows counted from its top
  EncodeParams band_params(const EncodeJob &e, uint32_t bandRows, uint32_t b)
  {
    const EncodeParams &p = e.p;
    EncodeParams q = p;
    const uint32_t r0 = b * bandRows, r1 = r0 + bandRows < p.blocksY ? r0 + bandRows : p.blocksY;
    const size_t y0 = (size_t)r0 * kBlock, skip = y0 * e.sizeX;
    q.io.in = p.io.in + skip;
    advance_planes(q.io.info, skip);
    q.sizeY = (uint32_t)(((size_t)r1 * kBlock < e.sizeY ? (size_t)r1 * kBlock : e.sizeY) - y0);
    q.blocksY = r1 - r0;
    q.imageStrips = q.stripsX * q.blocksY;
    q.records += (size_t)r0 * p.blocksX; q.shifts += (size_t)r0 * p.blocksX; q.invN += (size_t)r0 * p.blocksX * 4;
    q.stripCalls += (size_t)r0 * p.stripsX; q.stripBase += (size_t)r0 * p.stripsX;
    return q;
  }

  // ---- one chain, walked band by band under the E step; every band's F step under the walk of the next (when: encode_plan) ----
  // Timeline: {E step of all bands, the walk with the other bands' F steps under it, the last band's F step}
  limg_hip_result encode_ragged_banded(EncodeJob &e)
  {
    const uint32_t nBands = e.plan.bands, bandRows = e.plan.bandRows;
    limg_hip_context *const c = e.c;
    const EncodeParams &p = e.p;
    const hipStream_t stream = e.stream;
    limg_hip_result r;
    e.tl.mark();
    if ((r = ensure_stage(e)) != limg_hip_success) return r;
    if ((r = c->host.raggedEvents.ensure(nBands, hipEventDisableTiming)) != limg_hip_success) return r;
    const RaggedStage h(e.blocks, e.strips, c->host.stage.p);
    for (uint32_t b = 0; b < nBands; b++)
    {
      const EncodeParams q = band_params(e, bandRows, b);
      launch_fit_search(q, e.channels, stream);
      const size_t off = (size_t)b * bandRows * p.blocksX;
      HIP_TRY(hipMemcpyAsync(h.shifts + off, p.shifts + off, (size_t)q.blocksY * p.blocksX * 4, hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipEventRecord(c->host.raggedEvents[b], stream));
    }
    e.tl.mark();
    // sized for the worst case up front (3 calls per block): a band's calls go up while later bands are still being walked
    if ((r = size_noise_calls(e, h.maxCalls)) != limg_hip_success) return r;
    const bool pcg = c->opt.dither_pcg != 0;
    uint64_t hv = kDitherSeed;
    size_t call = 0;
    for (uint32_t b = 0; b < nBands; b++)
    {
      EncodeParams q = band_params(e, bandRows, b);
      const uint32_t r0 = b * bandRows, r1 = r0 + q.blocksY;
      HIP_TRY(hipEventSynchronize(c->host.raggedEvents[b])); // this band's shift words are down
      const size_t call0 = call;
      chain_walk_rows(hv, call, r0, r1, p.blocksX, p.stripsX, e.sizeX, e.sizeY, 1, 0, h.shifts, h.base, h.states, h.pixels, h.maxCalls, pcg);
      if ((r = upload_calls(e, h, h.maxCalls, call0, call - call0)) != limg_hip_success) return r;
      HIP_TRY(hipMemcpyAsync(p.stripBase + (size_t)r0 * p.stripsX, h.base + (size_t)r0 * p.stripsX, (size_t)q.blocksY * p.stripsX * 4, hipMemcpyHostToDevice, stream));
      q.noise = p.noise; q.noiseLast = p.noiseLast;
      if (b + 1 == nBands) e.tl.mark();
      launch_dither_store(q, e.channels, stream);
    }
    return release_stage(e);
  }
}

namespace limg_hip
{
  limg_hip_result encode_ragged(EncodeJob &e)
  {
    limg_hip_context *const c = e.c;
    const EncodeParams &p = e.p;
    const Partition &pt = e.pt;
    const hipStream_t stream = e.stream;
    if (e.plan.bands > 1) return encode_ragged_banded(e);

    e.tl.mark(); // the split path's timeline: {k_fit_search, the walk, k_dither_store}
    launch_fit_search(p, e.channels, stream);
    e.tl.mark();
    if (!e.dInfo) return limg_hip_success; // `_perf` behaviour: nothing to dither into, nothing to store
    limg_hip_result r;
    if ((r = ensure_stage(e)) != limg_hip_success) return r;
    const RaggedStage h(e.blocks, e.strips, c->host.stage.p);
    const size_t blocks = e.blocks, maxCalls = h.maxCalls;
    const bool pcg = c->opt.dither_pcg != 0;
    HIP_TRY(hipMemcpyAsync(h.shifts, p.shifts, blocks * 4, hipMemcpyDeviceToHost, stream));
    if (e.x.dPrevDesc) HIP_TRY(hipMemcpyAsync(h.prev, e.x.dPrevDesc, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    // sized for the calls the shift words count: a 32766 x 32768 image would otherwise hold 3.6 GB of the GPU for nothing
    size_t calls = 0;
    {
      size_t sumCalls = 0;
      for (size_t i = 0; i < blocks; i++) sumCalls += h.shifts[i] >> 24;
      calls = sumCalls < maxCalls ? sumCalls : maxCalls;
      if ((r = size_noise_calls(e, calls)) != limg_hip_success) return r;
    }
    uint64_t h0 = kDitherSeed;
    if (e.x.dPrevDesc)
    { // the block rows above this sub-image ran through the persistent kernel: every strip's descriptor ends as the inclusive call count of its chain
      if ((uint32_t)(*h.prev >> 32) != 2u || (uint32_t)*h.prev == 0xFFFFFFFFu || !chain_value_at((uint32_t)*h.prev, &h0))
      {
        fprintf(stderr, "limg_hip: the chain position of the last block row is unavailable (descriptor %016llx)\n", *h.prev);
        return limg_hip_error_Generic;
      }
    }
    size_t totalCalls = 0;
    // chains that restart at the seed are independent (the reference walks them on its pool's threads, src/limg.cpp:2114-2134): count every chain's calls, then
    // walk them side by side on up to limg_hip_options.ragged_walk_threads host threads (0: as many as there are chains, at most 16)
    unsigned threads = 1;
    if (pt.chainCount > 1 && pt.chainRows != 0 && !e.x.dPrevDesc && (blocks >= 4096 || c->opt.ragged_walk_threads > 1))
    {
      threads = c->opt.ragged_walk_threads > 0 ? (unsigned)c->opt.ragged_walk_threads : 16u;
      const unsigned hw = std::thread::hardware_concurrency();
      if (hw && threads > hw) threads = hw;
      if (threads > pt.chainCount) threads = pt.chainCount;
    }
    if (threads > 1)
    {
      size_t *first = new (std::nothrow) size_t[pt.chainCount + 1];
      uint32_t *row0 = new (std::nothrow) uint32_t[pt.chainCount + 1];
      if (!first || !row0) { delete[] first; delete[] row0; return limg_hip_error_MemoryAllocationFailure; }
      first[0] = 0;
      for (uint32_t k = 0; k < pt.chainCount; k++)
      {
        row0[k] = k * pt.chainRows;
        const uint32_t r1 = k + 1 < pt.chainCount ? (k + 1) * pt.chainRows : p.blocksY;
        size_t n = 0;
        for (size_t i = (size_t)row0[k] * p.blocksX; i < (size_t)r1 * p.blocksX; i++) n += h.shifts[i] >> 24;
        first[k + 1] = first[k] + n;
      }
      row0[pt.chainCount] = p.blocksY;
      run_on_threads(threads, [&](unsigned t) {
        for (uint32_t k = t; k < pt.chainCount; k += threads)
        {
          uint64_t hv = kDitherSeed;
          size_t call = first[k];
          chain_walk_rows(hv, call, row0[k], row0[k + 1], p.blocksX, p.stripsX, e.sizeX, e.sizeY, pt.chainCount, pt.chainRows, h.shifts, h.base, h.states, h.pixels, maxCalls, pcg);
        }
      });
      const size_t allCalls = first[pt.chainCount];
      delete[] first; delete[] row0;
      totalCalls = allCalls < maxCalls ? allCalls : maxCalls;
    }
    else totalCalls = chain_walk_blocks(h0, p.blocksX, p.blocksY, p.stripsX, e.sizeX, e.sizeY, pt.chainCount, pt.chainRows, h.shifts, h.base, h.states, h.pixels, maxCalls, pcg);
    if ((r = upload_calls(e, h, calls, 0, totalCalls)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpyAsync(p.stripBase, h.base, e.strips * 4, hipMemcpyHostToDevice, stream));
    if ((r = release_stage(e)) != limg_hip_success) return r;
    e.tl.mark();
    launch_dither_store(p, e.channels, stream);
    return limg_hip_success;
  }
}
