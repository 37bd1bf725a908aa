// limg_hip_blocked_api.hip -- the merged-block encoder's entries of the C ABI (reference: limg_blocked_encode3d_test, src/limg.cpp:1774-1885, :2329-2453): pass 1
// through the 8x8 encode, the similarity kernels, and the two-thread pipeline of the host merge (limg_hip_blocked_host.cpp) with the fit / search / store kernels
// (limg_hip_blocked.hip); the host-only merge helpers.
#include "limg_hip_context.h"

#include <chrono>
#include <condition_variable>
#include <functional>

using namespace limg_hip;

namespace
{
  using clk = std::chrono::steady_clock;
  double ms(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
  bool add_elapsed(double &ms, hipEvent_t a, hipEvent_t b) { float t = 0; if (hipEventElapsedTime(&t, a, b) != hipSuccess) return false; ms += t; return true; }

  constexpr size_t kInFlight = 32; // batches of the worker (below) whose fit + search kernel has been enqueued and whose chain has not been walked yet
  constexpr uint32_t kBands = 16;  // the similarity bits are produced and copied in this many bands of block rows

  // f(m) for the member pointer m of each of the 13 planes the encoder writes: every member of limg_hip_blocked_encode3d_info but pBlockError, in member order
  template <class F> void for_each_written_plane(F &&f)
  {
    using I = limg_hip_blocked_encode3d_info;
    auto each = [&](auto... m) { (f(m), ...); };
    each(&I::pDecoded, &I::pFactorsA, &I::pFactorsB, &I::pFactorsC, &I::pBitsPerPixel, &I::pShiftABCX, &I::pColAMin, &I::pColAMax, &I::pColBMin, &I::pColBMax, &I::pColCMin,
         &I::pColCMax, &I::pBlockIndex);
  }
  bool has_written_planes(const limg_hip_blocked_encode3d_info &info) { bool all = true; for_each_written_plane([&](auto m) { all = all && info.*m; }); return all; }

  size_t copy_regions(const std::vector<HostRegion> &regs, limg_hip_region *pRegions, size_t capacity)
  {
    for (size_t i = 0; pRegions && i < regs.size() && i < capacity; i++) pRegions[i] = { regs[i].ox, regs[i].oy, regs[i].rx, regs[i].ry };
    return regs.size();
  }

  // One merged-block encode as set_up and ensure_resources lay it out.  Fixed before the pipeline starts; while it runs, the merge writes a rectangle's desc and
  // npx entries before it publishes the rectangle, and the worker reads them after.
  struct BlockedJob
  {
    limg_hip_context *c;
    hipStream_t s; // the caller's
    size_t sizeX, sizeY, blocks, maxCalls;
    uint32_t blocksX, blocksY, bandRows, nBands;
    int channels; bool pcg; // pcg: limg_hip_options.dither_pcg
    bool compact;           // no plane is stored: the stream packer (limg_hip_stream_api.hip) takes the rectangles from the context's buffers
    BlockedParams bp;
    hipEvent_t *frontTimers; // begin of pass 1, its end = begin of the similarity kernels, their end
    // the context's pinned staging, and per dither call its chain value, noise offset and pixel count on the host (call*) and on the device (dCall*)
    limg_hip_block_record *hRec; unsigned long long *hBits; uint8_t *hFlags;
    RegionDesc *desc; RegionOut *hOut; unsigned long long *noiseBase;
    unsigned long long *callState, *callOff, *dCallState, *dCallOff;
    uint32_t *callPx, *dCallPx;
    uint32_t *npx; // per rectangle its pixel count
  };

  // Set-up: the shape, and every field of BlockedParams that does not point into the context's buffers.
  limg_hip_result set_up(BlockedJob &j, limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_blocked_encode3d_info &info,
                         uint32_t errorFactor, int fastBitCrushing, void *stream, bool compact)
  {
    j.compact = compact;
    j.c = c; j.s = (hipStream_t)stream; j.sizeX = sizeX; j.sizeY = sizeY; j.channels = hasAlpha ? 4 : 3; j.pcg = c->opt.dither_pcg != 0;
    j.blocksX = (uint32_t)((sizeX + kBlock - 1) / kBlock); j.blocksY = (uint32_t)((sizeY + kBlock - 1) / kBlock);
    j.blocks = (size_t)j.blocksX * j.blocksY; j.maxCalls = 3 * j.blocks;
    j.bandRows = (j.blocksY + kBands - 1) / kBands; j.nBands = (j.blocksY + j.bandRows - 1) / j.bandRows;
    const uint64_t capMax = ((uint64_t)sizeX * sizeY + 3ull * j.blocks + 3ull) & ~3ull; // every rectangle's scratch slice is rounded up to a multiple of 4
    if (capMax > 0xFFFFFFF0ull) return limg_hip_error_InvalidParameter;
    BlockedParams &bp = j.bp;
    memset(&bp, 0, sizeof(bp));
    bp.in = pIn; bp.sizeX = (uint32_t)sizeX; bp.sizeY = (uint32_t)sizeY; bp.blocksX = j.blocksX; bp.blocksY = j.blocksY; bp.channels = (uint32_t)j.channels;
    const Thresholds t = thresholds(errorFactor); // src/limg.cpp:2343-2368, same values as the 8x8 path
    bp.maxPixel32 = t.maxPixel32; bp.maxBlock = t.maxBlock;
    bp.crushBits = (int32_t)t.crushBits; bp.fast = fastBitCrushing != 0;
    forced_shifts(c->opt.forced_shift, bp.forced);
    bp.info = info;
    bp.scratchCap = (uint32_t)capMax;
    // k_blocked_store's 4-pixels-per-lane form: whole blocks (every rectangle row is a multiple of 8 pixels, every scratch / noise offset a multiple of 4) and planes
    // whose rows start 16-byte (32-bit planes) / 4-byte (byte planes) aligned
    uintptr_t w = 0, b8 = 0;
    for_each_written_plane([&](auto m) { (sizeof(*(info.*m)) == 4 ? w : b8) |= (uintptr_t)(info.*m); });
    bp.vecStore = (sizeX % kBlock == 0 && sizeY % kBlock == 0 && (w & 15u) == 0 && (b8 & 3u) == 0 && TOPT(c, blocked_no_vec_store) == 0) ? 1 : 0;
    return limg_hip_success;
  }

  // Resources: every buffer, stream and event of the call, before anything is enqueued -- a failure leaves no work in flight.  Buffers are sized for the worst
  // case, so that nothing is reallocated while the pipeline runs.
  limg_hip_result ensure_resources(BlockedJob &j)
  {
    limg_hip_context *c = j.c;
    const size_t blocks = j.blocks, maxCalls = j.maxCalls, px = j.sizeX * j.sizeY, capMax = j.bp.scratchCap;
    const bool bound = TOPT(c, blocked_no_bound) == 0;
    limg_hip_result r = c->blocked.workTimers.ensure(4 * kInFlight + 3, hipEventDefault);
    auto need = [&r](auto &buf, size_t bytes) { if (r == limg_hip_success) r = buf.ensure(bytes); };
    need(c->blocked.match, blocks * kMatchWords * 8); need(c->blocked.flags, blocks); need(c->blocked.hFlags, blocks + 16); // (+ 16: the merge's scan reads 16 flags at a time)
    if (bound) need(c->blocked.bound, blocks * 16);
    need(c->blocked.hRec, blocks * sizeof(limg_hip_block_record)); need(c->blocked.hBits, blocks * kMatchWords * 8);
    if (r == limg_hip_success) r = c->blocked.bandEvents.ensure(2 * kBands + 1, hipEventDisableTiming);
    need(c->blocked.hDesc, blocks * sizeof(RegionDesc)); need(c->blocked.hOut, blocks * sizeof(RegionOut)); need(c->blocked.hNoiseBase, blocks * 8 + 8);
    need(c->blocked.hNoise, maxCalls * 20 + 64); need(c->blocked.calls, maxCalls * 20 + 64); // per dither call 8 + 8 + 4 bytes
    need(c->blocked.regions, blocks * sizeof(RegionDesc)); need(c->blocked.out, blocks * sizeof(RegionOut)); need(c->blocked.noiseBase, blocks * 8 + 8); need(c->blocked.order, blocks * 4);
    need(c->blocked.noise, 3 * px + 64); need(c->blocked.px, capMax * 4); need(c->blocked.fac, capMax * 3);
    hipStream_t made;
    for (Stream *st : { &c->blocked.copyStream, &c->blocked.searchStream, &c->blocked.storeStream }) // (in this order: HIP maps streams to hardware queues in creation order)
      if (r == limg_hip_success) r = st->get(made);
    if (r == limg_hip_success) r = c->blocked.workEvents.ensure(kInFlight, hipEventDisableTiming);
    if (r != limg_hip_success) return r;
    try { c->blocked.regionPx.resize(blocks); }
    catch (const std::bad_alloc &) { return limg_hip_error_MemoryAllocationFailure; }
    j.npx = c->blocked.regionPx.data();
    j.frontTimers = c->blocked.workTimers.data() + 4 * kInFlight;
    j.hRec = (limg_hip_block_record *)c->blocked.hRec.p; j.hBits = (unsigned long long *)c->blocked.hBits.p; j.hFlags = (uint8_t *)c->blocked.hFlags.p;
    j.desc = (RegionDesc *)c->blocked.hDesc.p; j.hOut = (RegionOut *)c->blocked.hOut.p; j.noiseBase = (unsigned long long *)c->blocked.hNoiseBase.p;
    j.callState = (unsigned long long *)c->blocked.hNoise.p; j.callOff = j.callState + maxCalls; j.callPx = (uint32_t *)(j.callOff + maxCalls);
    j.dCallState = (unsigned long long *)c->blocked.calls.p; j.dCallOff = j.dCallState + maxCalls; j.dCallPx = (uint32_t *)(j.dCallOff + maxCalls);
    j.bp.matchBits = (unsigned long long *)c->blocked.match.p; j.bp.matchFlags = (uint8_t *)c->blocked.flags.p;
    if (bound) j.bp.matchBound = (float *)c->blocked.bound.p;
    j.bp.scratchPx = (uint32_t *)c->blocked.px.p; j.bp.scratchFac = (uint8_t *)c->blocked.fac.p; j.bp.noise = (const uint8_t *)c->blocked.noise.p;
    return limg_hip_success;
  }

  // Similarity bands: the bits are produced and copied band by band (block rows) so that the merge, which consumes seeds in raster order, can start after the
  // first band: kernel launches on `s`, copies on a second stream chained by events.  Returns once the first band is on the host.
  limg_hip_result similarity_bands(BlockedJob &j)
  {
    limg_hip_context *c = j.c;
    BlockedParams &bp = j.bp;
    const hipStream_t s = j.s, cs = c->blocked.copyStream;
    // The records go to the host as well, but the merge reads them only for pairs outside the similarity window (a few dozen per image): their copy (64 MB for 8192^2,
    // 1.3 ms of PCIe) is queued BEHIND the first two bands' bits, and the merge waits for it when it first needs a record -- not before it starts.
    HIP_TRY(hipEventRecord(j.frontTimers[1], s));
    c->blocked.lastBlocks = j.blocks;
    launch_blocked_bounds(bp, s);
    for (uint32_t b = 0; b < j.nBands; b++)
    {
      const uint32_t row0 = b * j.bandRows, rows = min(j.bandRows, j.blocksY - row0);
      bp.seedBase = row0 * j.blocksX; bp.seedCount = rows * j.blocksX;
      launch_blocked_match(bp, s);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(c->blocked.bandEvents[2 * b], s));
      HIP_TRY(hipStreamWaitEvent(cs, c->blocked.bandEvents[2 * b], 0));
      HIP_TRY(hipMemcpyAsync(j.hBits + (size_t)bp.seedBase * kMatchWords, bp.matchBits + (size_t)bp.seedBase * kMatchWords, (size_t)bp.seedCount * kMatchWords * 8,
                             hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipMemcpyAsync(j.hFlags + bp.seedBase, bp.matchFlags + bp.seedBase, bp.seedCount, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipEventRecord(c->blocked.bandEvents[2 * b + 1], cs));
      if (b == 1 || (b == 0 && j.nBands == 1))
      {
        HIP_TRY(hipMemcpyAsync(j.hRec, c->enc.records.p, j.blocks * sizeof(limg_hip_block_record), hipMemcpyDeviceToHost, cs)); // (`cs` has waited for a band's kernel: pass 1 is long done)
        HIP_TRY(hipEventRecord(c->blocked.bandEvents[2 * kBands], cs)); // "records are on the host"
      }
    }
    HIP_TRY(hipEventRecord(j.frontTimers[2], s)); // (`s` holds nothing but the similarity kernels between the two timers: the copies run on `cs`)
    HIP_TRY(hipEventSynchronize(c->blocked.bandEvents[1])); // the first band's bits: the merge can start
    return limg_hip_success;
  }

  // The rest of the call is a two-thread pipeline.  The calling thread runs the greedy raster merge (serial by construction; it only looks the similarity bits up)
  // and publishes finished rectangles every few thousand; a worker thread takes them batch by batch, in creation order: fit + search kernel, copy of the shift
  // words, dither chain walk for the batch (the chain is serial too, but independent of the merge), noise upload, store kernel.
  struct Pipe { std::mutex m; std::condition_variable cv; size_t ready = 0; bool finished = false; }; // rectangles [0, ready) are published

  // Producer: the merge; its progress callback lays the finished rectangles out (pixel counts, scratch slices) and hands them over.
  struct Merge
  {
    BlockedJob &j;
    Pipe &pipe;
    uint32_t bandsReady = 0;
    bool recordsHere = false, bandError = false, failed = false;
    size_t laid = 0; uint64_t cap = 0; // rectangles laid out, their scratch
    clk::time_point end;
    void need_records() { if (!recordsHere && hipEventSynchronize(j.c->blocked.bandEvents[2 * kBands]) != hipSuccess) bandError = true; recordsHere = true; }
    void need_seed_row(uint32_t row)
    {
      for (; bandsReady < j.nBands && row >= bandsReady * j.bandRows; bandsReady++)
        if (hipEventSynchronize(j.c->blocked.bandEvents[2 * bandsReady + 1]) != hipSuccess) bandError = true;
    }
    void publish(size_t count)
    {
      for (size_t i = laid; i < count; i++)
      {
        const HostRegion &h = j.c->blocked.lastRegions[i];
        size_t xpx = (size_t)h.rx * kBlock, ypx = (size_t)h.ry * kBlock;
        if (h.ox + h.rx == j.blocksX && (j.sizeX % kBlock)) xpx = xpx - kBlock + j.sizeX % kBlock;
        if (h.oy + h.ry == j.blocksY && (j.sizeY % kBlock)) ypx = ypx - kBlock + j.sizeY % kBlock;
        j.npx[i] = (uint32_t)(xpx * ypx);
        j.desc[i] = { h.ox, h.oy, h.rx, h.ry, h.keep, (uint32_t)cap, { 0, 0 } };
        cap += ((uint64_t)j.npx[i] + 3) & ~3ull;
      }
      laid = count;
      { std::lock_guard<std::mutex> lk(pipe.m); pipe.ready = count; }
      pipe.cv.notify_one();
    }
    void run() noexcept
    {
      try
      {
        const std::function<void()> records = [this] { need_records(); };
        const std::function<void(uint32_t)> seedRow = [this](uint32_t row) { need_seed_row(row); };
        const std::function<void(size_t)> progress = [this](size_t count) { publish(count); };
        blocked_merge(j.hRec, j.hBits, j.blocksX, j.blocksY, j.channels, j.c->blocked.lastRegions, &progress, &seedRow, j.hFlags, &records);
      }
      catch (...) { failed = true; } // out of host memory: the worker must still be released
      need_seed_row(j.blocksY - 1); // every band's copy is complete before the staging buffers can be reused
      need_records();
      end = clk::now();
      { std::lock_guard<std::mutex> lk(pipe.m); pipe.finished = true; }
      pipe.cv.notify_one();
    }
  };

  // Worker: the GPU runs AHEAD of this thread: whatever the merge has published goes to the device at once (rectangle table up, fit + search kernel, records and
  // shift words back, one event per batch, up to kInFlight batches), and the chain -- this thread's real work, serial by construction -- is walked batch by batch
  // in creation order as the results arrive.  (Rounds 2-3 kept one batch in flight: every batch's GPU round trip was waited for, 11-20 ms per image.)
  // One batch = everything the merge has published when the worker looks; one stream for the fit + search kernels.  Measured on one box (profiles/archive/r04_blocked_pipeline.md):
  // batches capped at 8 K ... 64 K rectangles, two or four streams round-robin, a high-priority stream -- all within +-2 ms of this, most of them worse: the GPU
  // (similarity kernels 13 ms + fit / search kernels 13 ms per 8192^2 image) is as busy as the two host threads, so reordering its queue buys nothing.
  struct Worker
  {
    struct Batch { size_t r0, r1, ev; }; // rectangles [r0, r1); ev: its slot of workEvents / workTimers
    const BlockedJob &j;
    Pipe &pipe;
    limg_hip_context *const c = j.c;
    Batch queue[kInFlight]; // FIFO: batches [head, tail), batch k in queue[k % kInFlight]
    size_t head = 0, tail = 0, issued = 0; // issued: rectangles taken from the merge
    bool fin = false;                      // ... all of them
    uint64_t chain = kDitherSeed, noiseOff = 0; size_t callCount = 0; // the dither chain walked so far
    double kernelMs[2] = { 0, 0 };   // HIP events, summed over the batches: fit + search, noise expansion + store
    double busy[3] = { 0, 0, 0 };    // fit + search (incl. copies), chain walk, store launch
    bool storeTimed[kInFlight] = {}; // slot i's store timers hold a finished-or-enqueued interval that has not been added up yet
    limg_hip_result result = limg_hip_success;
    static constexpr size_t kOrderFrom = 512; // batches from this many rectangles on get the device-side "large rectangles first" order (k_blocked_order)
    // enqueue_published is called at the top of every round AND between the pieces of a batch's chain walk: a batch's walk takes milliseconds, and what the merge
    // publishes meanwhile should be on the GPU (kernel latency: the life of its largest rectangle, 0.6-2 ms) before this thread comes looking for it -- not be
    // enqueued when the walk is over.  A kernel's duration is the life of its largest rectangle whatever the batch's size and the batches of a stream run one after
    // the other, so a look from inside a walk (minNew > 0) takes a batch only when it is worth a launch; a look with nothing else to do takes whatever there is.
    // (same-box A/B of these three and of the merge's first report, tools/r04/run38.sh: photo-noise 27.5-27.7 ms against 28.8-32.0 with "any size, looks every
    //  8192 rectangles, first report at 4096", gradient 20.3-20.4 against 19.9-21.1)
    static constexpr size_t kWorthWithOneInFlight = 16384, kWorthFromInsideAWalk = 8192, kWalkPiece = 2048;
    BlockedParams params_of(const Batch &b) const
    {
      BlockedParams q = j.bp;
      q.regions = (const RegionDesc *)c->blocked.regions.p + b.r0; q.nRegions = (uint32_t)(b.r1 - b.r0); q.regionBase = (uint32_t)b.r0;
      q.out = (RegionOut *)c->blocked.out.p + b.r0; q.noiseBase = (const unsigned long long *)c->blocked.noiseBase.p + b.r0;
      q.order = (b.r1 - b.r0 >= kOrderFrom && TOPT(c, blocked_no_order) == 0) ? (uint32_t *)c->blocked.order.p + b.r0 : nullptr; // (a small batch is one round of workgroups anyway)
      return q;
    }
    // Everything the merge has published since the last look goes to the GPU as one batch.  mayWait: nothing is left to walk, so wait for the merge.
    void enqueue_published(bool mayWait, size_t minNew)
    {
      if (fin || tail - head >= kInFlight) return;
      size_t r0 = 0, r1 = 0;
      {
        std::unique_lock<std::mutex> lk(pipe.m);
        if (mayWait) pipe.cv.wait(lk, [&] { return pipe.ready > issued || pipe.finished; });
        if (pipe.ready == issued) fin = pipe.finished;
        else if (pipe.ready - issued >= minNew || pipe.finished) { r0 = issued; r1 = issued = pipe.ready; }
      }
      if (r1 == r0) return;
      const Batch nb = { r0, r1, tail % kInFlight };
      if (storeTimed[nb.ev]) // the slot comes round again: its previous batch's store kernels were enqueued kInFlight batches ago
        if (hipEventSynchronize(c->blocked.workTimers[4 * nb.ev + 3]) == hipSuccess) add_elapsed(kernelMs[1], c->blocked.workTimers[4 * nb.ev + 2], c->blocked.workTimers[4 * nb.ev + 3]);
      storeTimed[nb.ev] = false;
      if (result == limg_hip_success)
      {
        const size_t n = r1 - r0;
        const BlockedParams q = params_of(nb);
        const hipStream_t bs = c->blocked.searchStream;
        bool ok = hipMemcpyAsync((RegionDesc *)c->blocked.regions.p + r0, j.desc + r0, n * sizeof(RegionDesc), hipMemcpyHostToDevice, bs) == hipSuccess;
        ok = ok && hipEventRecord(c->blocked.workTimers[4 * nb.ev], bs) == hipSuccess;
        if (ok) { launch_blocked_order(q, bs); launch_blocked_fit_search(q, bs); ok = hipGetLastError() == hipSuccess; }
        ok = ok && hipEventRecord(c->blocked.workTimers[4 * nb.ev + 1], bs) == hipSuccess;
        ok = ok && hipMemcpyAsync(j.hOut + r0, (RegionOut *)c->blocked.out.p + r0, n * sizeof(RegionOut), hipMemcpyDeviceToHost, bs) == hipSuccess;
        ok = ok && hipEventRecord(c->blocked.workEvents[nb.ev], bs) == hipSuccess;
        if (!ok) result = limg_hip_error_Generic;
      }
      queue[tail++ % kInFlight] = nb;
    }
    // The oldest batch in flight, once its shift words are back: walk its stretch of the dither chain and enqueue its noise expansion and store.  (`pending` is a
    // copy: the walk may queue a new batch in its slot.)
    void walk_and_store(const Batch pending, clk::time_point w0)
    {
      if (result != limg_hip_success) return;
      bool ok = hipEventSynchronize(c->blocked.workEvents[pending.ev]) == hipSuccess;
      if (ok) add_elapsed(kernelMs[0], c->blocked.workTimers[4 * pending.ev], c->blocked.workTimers[4 * pending.ev + 1]);
      const clk::time_point w1 = clk::now();
      // the dither chain (src/limg_internal.h:711, src/limg.cpp:1541-1551): one chain through all rectangles in creation order; a call over N
      // pixels advances it by floor(N / 8) AES rounds + N % 8 PCG steps, so it is walked here -- for the chain VALUES only: every call's start value, pixel
      // count and place in the noise buffer go up (20 bytes per call) and k_noise_expand_calls produces the byte every pixel adds on the device.  (Rounds
      // 1-3 wrote the bytes here and uploaded them: 200 MB per 8192^2 image through this thread's store buffers and over PCIe.)
      const size_t call0 = callCount;
      // (kWalkPiece rectangles between two looks at what the merge has published: 0.1-0.6 ms of chain)
      for (size_t w = pending.r0; ok && w < pending.r1; w += kWalkPiece)
      {
        const size_t n = pending.r1 - w < kWalkPiece ? pending.r1 - w : kWalkPiece;
        chain = chain_walk_batch(chain, n, reinterpret_cast<const uint8_t *>(&j.hOut[w].shiftWord), sizeof(RegionOut), j.npx + w, j.noiseBase + w, j.callState, j.callOff,
                                 j.callPx, noiseOff, callCount, j.maxCalls, j.pcg);
        if (w + n < pending.r1) enqueue_published(false, kWorthFromInsideAWalk);
      }
      const clk::time_point w2 = clk::now();
      const size_t nc = callCount - call0;
      const hipStream_t ss = c->blocked.storeStream; // noise expansion + store kernels of a batch: beside the next batch's fit + search kernel, not behind it
      ok = ok && hipStreamWaitEvent(ss, c->blocked.workEvents[pending.ev], 0) == hipSuccess; // this batch's records and shift words are in bOut
      ok = ok && hipEventRecord(c->blocked.workTimers[4 * pending.ev + 2], ss) == hipSuccess;
      if (ok && nc)
      {
        ok = hipMemcpyAsync(j.dCallState + call0, j.callState + call0, nc * 8, hipMemcpyHostToDevice, ss) == hipSuccess &&
             hipMemcpyAsync(j.dCallOff + call0, j.callOff + call0, nc * 8, hipMemcpyHostToDevice, ss) == hipSuccess &&
             hipMemcpyAsync(j.dCallPx + call0, j.callPx + call0, nc * 4, hipMemcpyHostToDevice, ss) == hipSuccess;
        if (ok) { launch_noise_expand_calls((uint8_t *)c->blocked.noise.p, j.dCallState + call0, j.dCallOff + call0, j.dCallPx + call0, nc, j.pcg, ss); ok = hipGetLastError() == hipSuccess; }
      }
      ok = ok && hipMemcpyAsync((unsigned long long *)c->blocked.noiseBase.p + pending.r0, j.noiseBase + pending.r0, (pending.r1 - pending.r0) * 8, hipMemcpyHostToDevice, ss) == hipSuccess;
      if (ok && !j.compact) { launch_blocked_store(params_of(pending), ss); ok = hipGetLastError() == hipSuccess; }
      if (ok && hipEventRecord(c->blocked.workTimers[4 * pending.ev + 3], ss) == hipSuccess) storeTimed[pending.ev] = true;
      const clk::time_point w3 = clk::now();
      busy[0] += ms(w0, w1); busy[1] += ms(w1, w2); busy[2] += ms(w2, w3);
      if (!ok) result = limg_hip_error_Generic;
    }
    void run() noexcept
    {
      if (hipSetDevice(c->device) != hipSuccess) result = limg_hip_error_Generic;
      for (;;)
      {
        const clk::time_point w0 = clk::now();
        enqueue_published(head == tail, head == tail ? 0 : kWorthWithOneInFlight); // (with a batch in flight to wait for and walk, small change accumulates meanwhile)
        if (head < tail) walk_and_store(queue[head++ % kInFlight], w0);
        if (fin && head == tail) break;
      }
      if (hipStreamSynchronize(c->blocked.searchStream) != hipSuccess && result == limg_hip_success) result = limg_hip_error_Generic;
      if (hipStreamSynchronize(c->blocked.storeStream) != hipSuccess && result == limg_hip_success) result = limg_hip_error_Generic;
      for (size_t i = 0; i < kInFlight; i++)
        if (storeTimed[i]) add_elapsed(kernelMs[1], c->blocked.workTimers[4 * i + 2], c->blocked.workTimers[4 * i + 3]);
    }
  };

  // Statistics: src/limg.cpp:1561-1590 per rectangle: (8 - shift) bits for each of its pixels, and the pixels by shift
  void collect_stats(const BlockedJob &j)
  {
    limg_hip_context *c = j.c;
    memset(c->stats.host, 0, sizeof(c->stats.host));
    for (size_t i = 0; i < c->blocked.lastRegions.size(); i++)
      for (int f = 0; f < 3; f++)
      {
        uint32_t sh = (j.hOut[i].shiftWord >> (8 * f)) & 0xFFu;
        if (sh > 8) sh = 8;
        c->stats.host[f] += (uint64_t)(8 - sh) * j.npx[i];
        c->stats.host[3 + 9 * f + sh] += j.npx[i];
      }
    c->stats.state = 2; c->stats.pixels = (uint64_t)j.sizeX * j.sizeY;
  }
}

extern "C"
{
  int limg_hip_host_blocked_matches(int channels, const limg_hip_block_record *pSeed, const limg_hip_block_record *pCandidate)
  {
    if (!pSeed || !pCandidate || (channels != 3 && channels != 4)) return -1;
    return blocked_matches_host(channels, *pSeed, *pCandidate) ? 1 : 0;
  }

  limg_hip_result limg_hip_host_blocked_merge(const limg_hip_block_record *pFits, const uint64_t *pMatchBits, size_t blocksX, size_t blocksY, int channels, limg_hip_region *pRegions,
                                              size_t capacity, size_t *pCount)
  {
    if (!pFits || !pCount) return limg_hip_error_ArgumentNull;
    if (blocksX == 0 || blocksY == 0 || blocksX > 0x0FFFFFFFull || blocksY > 0x0FFFFFFFull || (channels != 3 && channels != 4)) return limg_hip_error_InvalidParameter;
    std::vector<HostRegion> regs;
    std::vector<uint8_t> flags;
    if (pMatchBits)
    { // the per-seed viability flags the GPU kernel derives from the same bits (k_blocked_match)
      flags.resize(blocksX * blocksY + 16); // (+ 16: the merge's scan reads 16 flags at a time)
      for (size_t i = 0; i < blocksX * blocksY; i++)
      {
        const uint64_t *w = pMatchBits + i * kMatchWords;
        auto bit = [&](int dx, int dy) -> unsigned { const int cell = (dy + kMatchLo) * kMatchSide + dx + kMatchLo; return (unsigned)(w[cell >> 6] >> (cell & 63)) & 1u; };
        const unsigned all8 = bit(1, 0) & bit(2, 0) & bit(0, 1) & bit(1, 1) & bit(2, 1) & bit(0, 2) & bit(1, 2) & bit(2, 2);
        flags[i] = (uint8_t)(all8 | ((bit(1, 0) | bit(0, 1)) << 1));
      }
    }
    blocked_merge(pFits, (const unsigned long long *)pMatchBits, (uint32_t)blocksX, (uint32_t)blocksY, channels, regs, nullptr, nullptr, pMatchBits ? flags.data() : nullptr);
    *pCount = copy_regions(regs, pRegions, capacity);
    return limg_hip_success;
  }

  size_t limg_hip_host_blocked_match_words(void) { return kMatchWords; }

  limg_hip_result limg_hip_host_blocked_match_bits(const limg_hip_block_record *pFits, size_t blocksX, size_t blocksY, int channels, uint64_t *pMatchBits)
  {
    if (!pFits || !pMatchBits) return limg_hip_error_ArgumentNull;
    if (channels != 3 && channels != 4) return limg_hip_error_InvalidParameter;
    for (size_t sy = 0; sy < blocksY; sy++)
      for (size_t sx = 0; sx < blocksX; sx++)
      {
        uint64_t *w = pMatchBits + (sy * blocksX + sx) * kMatchWords;
        for (int i = 0; i < kMatchWords; i++) w[i] = 0;
        for (int cell = 0; cell < kMatchCells; cell++)
        {
          const long dy = cell / kMatchSide - kMatchLo, dx = cell % kMatchSide - kMatchLo;
          const long cx = (long)sx + dx, cy = (long)sy + dy;
          if ((dx | dy) == 0 || cx < 0 || cy < 0 || cx >= (long)blocksX || cy >= (long)blocksY) continue;
          if (blocked_matches_host(channels, pFits[sy * blocksX + sx], pFits[(size_t)cy * blocksX + cx])) w[cell >> 6] |= 1ull << (cell & 63);
        }
      }
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_encode3d_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_blocked_encode3d_info *pInfo,
                                                   uint32_t errorFactor, int fastBitCrushing, void *stream)
  {
    if (!c || !pIn || !pInfo || !has_written_planes(*pInfo)) return limg_hip_error_ArgumentNull;
    return blocked_encode_device(c, pIn, sizeX, sizeY, hasAlpha, pInfo, errorFactor, fastBitCrushing, (hipStream_t)stream);
  }
}

namespace limg_hip
{
  limg_hip_result blocked_encode_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_blocked_encode3d_info *pInfo,
                                        uint32_t errorFactor, int fastBitCrushing, hipStream_t stream)
  {
    const limg_hip_blocked_encode3d_info noPlanes = {};
    if (!EncodeShape(sizeX, sizeY).valid || sizeX * sizeY > 0x60000000ull) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    const clk::time_point t0 = clk::now();
    BlockedJob j; limg_hip_result r;
    if ((r = set_up(j, c, pIn, sizeX, sizeY, hasAlpha, pInfo ? *pInfo : noPlanes, errorFactor, fastBitCrushing, stream, pInfo == nullptr)) != limg_hip_success) return r;
    if ((r = ensure_resources(j)) != limg_hip_success) return r;
    c->blocked.scratchCap = j.bp.scratchCap; c->stream.packTimed = false; c->blocked.last.valid = false;
    // pass 1 (src/limg.cpp:1088-1119): every block's own fit = the 8x8 path's E step, records only
    EncodeExtra x1; x1.fitOnly = true;
    HIP_TRY(hipEventRecord(j.frontTimers[0], j.s));
    if ((r = encode_device(c, pIn, sizeX, sizeY, hasAlpha, nullptr, nullptr, errorFactor, 0, fastBitCrushing, j.s, x1)) != limg_hip_success) return r;
    j.bp.pass1 = (const limg_hip_block_record *)c->enc.records.p;
    if ((r = similarity_bands(j)) != limg_hip_success) { (void)hipStreamSynchronize(c->blocked.copyStream); return r; } // (no copy into the pinned staging may outlive the call)
    const clk::time_point t1 = clk::now();
    Pipe pipe;
    Merge merge{ j, pipe };
    Worker worker{ j, pipe };
    // the merge on this thread, the worker on one of its own -- or after the merge, on this thread, if the host refuses the thread: the merge never waits for it
    run_on_threads(2, [&](unsigned t) { if (t == 0) merge.run(); else worker.run(); });
    const clk::time_point t5 = clk::now();
    double a = 0, b = 0; // (both intervals ended before the merge's last band arrived)
    const bool ok = add_elapsed(a, j.frontTimers[0], j.frontTimers[1]) && add_elapsed(b, j.frontTimers[1], j.frontTimers[2]);
    c->blocked.kernelMs[0] = ok ? a : 0; c->blocked.kernelMs[1] = ok ? b : 0; c->blocked.kernelMs[2] = worker.kernelMs[0]; c->blocked.kernelMs[3] = worker.kernelMs[1];
    c->blocked.ms[0] = ms(t0, t1); c->blocked.ms[1] = ms(t1, merge.end); c->blocked.ms[2] = worker.busy[0]; c->blocked.ms[3] = worker.busy[1]; c->blocked.ms[4] = worker.busy[2];
    c->blocked.ms[5] = ms(t0, t5);
    if (merge.failed) return limg_hip_error_MemoryAllocationFailure;
    if (merge.bandError) return limg_hip_error_Generic;
    if (worker.result == limg_hip_success && c->opt.collect_stats) collect_stats(j);
    c->blocked.last.sizeX = sizeX; c->blocked.last.sizeY = sizeY; c->blocked.last.channels = j.channels; c->blocked.last.errorFactor = errorFactor;
    c->blocked.last.flags = (fastBitCrushing ? 1u : 0u) | (j.pcg ? 2u : 0u);
    c->blocked.last.valid = worker.result == limg_hip_success;
    return worker.result;
  }
}

extern "C"
{

  limg_hip_result limg_hip_blocked_regions(limg_hip_context *c, limg_hip_region *pRegions, size_t capacity, size_t *pCount)
  {
    if (!c || !pCount) return limg_hip_error_ArgumentNull;
    *pCount = copy_regions(c->blocked.lastRegions, pRegions, capacity);
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_timing(limg_hip_context *c, double *pMs6)
  {
    if (!c || !pMs6) return limg_hip_error_ArgumentNull;
    memcpy(pMs6, c->blocked.ms, sizeof(c->blocked.ms));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_match_bits(limg_hip_context *c, uint64_t *pBits, size_t capacityWords, size_t *pWords)
  { // the similarity bits the last merged-block encode's merge worked from (they stay in the context's pinned staging buffer until the next encode)
    if (!c || !pWords) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const size_t words = c->blocked.lastBlocks * kMatchWords;
    *pWords = words;
    if (pBits && c->blocked.hBits.p) memcpy(pBits, c->blocked.hBits.p, (words < capacityWords ? words : capacityWords) * 8);
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_kernel_timing(limg_hip_context *c, double *pMs4)
  {
    if (!c || !pMs4) return limg_hip_error_ArgumentNull;
    if (c->stream.packTimed)
    { // a stream encode: its scan + pack kernels were enqueued behind the pipeline (limg_hip_stream_api.hip) and belong to slot [3]
      float t = 0;
      if (hipEventSynchronize(c->stream.packTimers[1]) == hipSuccess && hipEventElapsedTime(&t, c->stream.packTimers[0], c->stream.packTimers[1]) == hipSuccess) c->blocked.kernelMs[3] += t;
      c->stream.packTimed = false;
    }
    memcpy(pMs4, c->blocked.kernelMs, sizeof(c->blocked.kernelMs));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_encode3d_stats(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_blocked_encode3d_info *pInfo,
                                                  uint32_t errorFactor, int fastBitCrushing, uint64_t *pCounters30, uint64_t *pPixels)
  { // (see limg_hip_encode3d_stats; upstream: src/limg.cpp:1561-1590 counters, printed by limg_blocked_encode3d_test itself)
    if (!c || !pCounters30) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const int32_t was = c->opt.collect_stats;
    c->opt.collect_stats = 1;
    limg_hip_result r = limg_hip_blocked_encode3d(c, pIn, sizeX, sizeY, hasAlpha, pInfo, errorFactor, fastBitCrushing);
    if (r == limg_hip_success) r = limg_hip_last_stats(c, pCounters30, pPixels);
    c->opt.collect_stats = was;
    return r;
  }

  limg_hip_result limg_hip_blocked_encode3d(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_blocked_encode3d_info *pInfo, uint32_t errorFactor,
                                            int fastBitCrushing)
  {
    if (!c || !pIn || !pInfo) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (sizeX == 0 || sizeY == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = sizeX * sizeY, stride = (px * 4 + 255) & ~(size_t)255;
    limg_hip_result r;
    if ((r = c->host.in.ensure(px * 4)) != limg_hip_success) return r;
    if ((r = c->host.planes.ensure(stride * 13)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->host.in.p, pIn, px * 4, hipMemcpyHostToDevice));
    if (!has_written_planes(*pInfo)) return limg_hip_error_ArgumentNull;
    limg_hip_blocked_encode3d_info d = {};
    size_t i = 0; // 13 written planes, one `stride` each (the uint8 ones use a quarter of theirs)
    for_each_written_plane([&](auto m) { d.*m = (std::decay_t<decltype(d.*m)>)((uint8_t *)c->host.planes.p + stride * i++); });
    if ((r = limg_hip_blocked_encode3d_device(c, (const uint32_t *)c->host.in.p, sizeX, sizeY, hasAlpha, &d, errorFactor, fastBitCrushing, nullptr)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    hipError_t e = hipSuccess;
    for_each_written_plane([&](auto m) { if (e == hipSuccess) e = hipMemcpy(pInfo->*m, d.*m, px * sizeof(*(d.*m)), hipMemcpyDeviceToHost); });
    HIP_TRY(e);
    return limg_hip_success;
  }
}
