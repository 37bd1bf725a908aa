// limg_hip_blocked_api.hip -- the merged-block encoder's entries of the C ABI (reference: limg_blocked_encode3d_test, src/limg.cpp:1774-1885, :2329-2453): pass 1
// through the 8x8 encode, the similarity kernels, and the two-thread pipeline of the host merge (limg_hip_blocked_host.cpp) with the fit / search / store kernels
// (limg_hip_blocked.hip); the host-only merge helpers.
#include "limg_hip_context.h"

#include <chrono>
#include <condition_variable>
#include <functional>

using namespace limg_hip;

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
    *pCount = regs.size();
    if (pRegions)
      for (size_t i = 0; i < regs.size() && i < capacity; i++) pRegions[i] = { regs[i].ox, regs[i].oy, regs[i].rx, regs[i].ry };
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
    if (!c || !pIn || !pInfo) return limg_hip_error_ArgumentNull;
    if (!pInfo->pDecoded || !pInfo->pFactorsA || !pInfo->pFactorsB || !pInfo->pFactorsC || !pInfo->pBitsPerPixel || !pInfo->pShiftABCX || !pInfo->pColAMin || !pInfo->pColAMax ||
        !pInfo->pColBMin || !pInfo->pColBMax || !pInfo->pColCMin || !pInfo->pColCMax || !pInfo->pBlockIndex)
      return limg_hip_error_ArgumentNull;
    if (sizeX == 0 || sizeY == 0 || sizeX > 0x7FFFFFF8ull || sizeY > 0x7FFFFFF8ull || sizeX * sizeY > 0x60000000ull) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const clk::time_point t0 = clk::now();
    const int channels = hasAlpha ? 4 : 3;
    const uint32_t blocksX = (uint32_t)((sizeX + kBlock - 1) / kBlock), blocksY = (uint32_t)((sizeY + kBlock - 1) / kBlock);
    const size_t blocks = (size_t)blocksX * blocksY;
    limg_hip_result r;

    constexpr size_t kInFlight = 32; // batches of the worker (below) whose fit + search kernel has been enqueued and whose chain has not been walked yet
    while (c->workTimers.size() < 4 * kInFlight + 3)
    {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      c->workTimers.push_back(e);
    }
    hipEvent_t *frontTimers = c->workTimers.data() + 4 * kInFlight;

    // pass 1 (src/limg.cpp:1088-1119): every block's own fit = the 8x8 path's E step, records only
    EncodeExtra x1;
    x1.fitOnly = true;
    HIP_TRY(hipEventRecord(frontTimers[0], s));
    if ((r = encode_device(c, pIn, sizeX, sizeY, hasAlpha, nullptr, nullptr, errorFactor, 0, fastBitCrushing, s, x1)) != limg_hip_success) return r;

    BlockedParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.in = pIn; bp.sizeX = (uint32_t)sizeX; bp.sizeY = (uint32_t)sizeY; bp.blocksX = blocksX; bp.blocksY = blocksY; bp.channels = (uint32_t)channels;
    const uint64_t maxPixel = (uint64_t)0x6 * (errorFactor / 2) * 7, maxBlock = (uint64_t)0x4 * (errorFactor / 2) * 7; // src/limg.cpp:2343-2368, same values as the 8x8 path
    bp.maxPixel32 = maxPixel > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)maxPixel;
    bp.maxBlock = maxBlock;
    bp.crushBits = errorFactor != 0; bp.fast = fastBitCrushing != 0;
    const bool forced = c->opt.forced_shift[0] >= 0 && c->opt.forced_shift[0] <= 8 && c->opt.forced_shift[1] >= 0 && c->opt.forced_shift[1] <= 8 &&
                        c->opt.forced_shift[2] >= 0 && c->opt.forced_shift[2] <= 8;
    for (int i = 0; i < 3; i++) bp.forced[i] = forced ? c->opt.forced_shift[i] : -1;
    bp.pass1 = (const limg_hip_block_record *)c->records.p;
    if ((r = c->bMatch.ensure(blocks * kMatchWords * 8)) != limg_hip_success) return r;
    bp.matchBits = (unsigned long long *)c->bMatch.p;
    if ((r = c->bFlags.ensure(blocks)) != limg_hip_success) return r;
    if ((r = c->hFlags.ensure(blocks + 16)) != limg_hip_success) return r; // (+ 16: the merge's scan reads 16 flags at a time)
    bp.matchFlags = (uint8_t *)c->bFlags.p;
    if (TOPT(c, blocked_no_bound) == 0)
    {
      if ((r = c->bBound.ensure(blocks * 16)) != limg_hip_success) return r;
      bp.matchBound = (float *)c->bBound.p;
    }
    uint8_t *hFlags = (uint8_t *)c->hFlags.p;
    bp.info = *pInfo;
    // The similarity bits are produced and copied band by band (block rows) so that the merge, which consumes seeds in raster order, can start
    // after the first band: kernel launches on `s`, copies on a second stream chained by events.
    if ((r = c->hRec.ensure(blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
    if ((r = c->hBits.ensure(blocks * kMatchWords * 8)) != limg_hip_success) return r;
    limg_hip_block_record *hRec = (limg_hip_block_record *)c->hRec.p;
    unsigned long long *hBits = (unsigned long long *)c->hBits.p;
    constexpr uint32_t kBands = 16;
    const uint32_t bandRows = (blocksY + kBands - 1) / kBands, nBands = (blocksY + bandRows - 1) / bandRows;
    if (!c->copyStream) HIP_TRY(hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking));
    while (c->bandEvents.size() < 2 * kBands + 1)
    {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      c->bandEvents.push_back(e);
    }
    hipStream_t cs = c->copyStream;
    // The records go to the host as well, but the merge reads them only for pairs outside the similarity window (a few dozen per image): their copy (64 MB for 8192^2,
    // 1.3 ms of PCIe) is queued BEHIND the first two bands' bits, and the merge waits for it when it first needs a record -- not before it starts.
    hipEvent_t evPass1 = c->bandEvents[2 * kBands];
    HIP_TRY(hipEventRecord(frontTimers[1], s));
    auto copy_records = [&]() -> limg_hip_result
    {
      HIP_TRY(hipMemcpyAsync(hRec, c->records.p, blocks * sizeof(limg_hip_block_record), hipMemcpyDeviceToHost, cs)); // (`cs` has waited for a band's kernel: pass 1 is long done)
      HIP_TRY(hipEventRecord(evPass1, cs)); // "records are on the host"
      return limg_hip_success;
    };
    c->lastBlocks = blocks;
    launch_blocked_bounds(bp, s);
    for (uint32_t b = 0; b < nBands; b++)
    {
      const uint32_t row0 = b * bandRows, rows = min(bandRows, blocksY - row0);
      bp.seedBase = row0 * blocksX; bp.seedCount = rows * blocksX;
      launch_blocked_match(bp, s);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(c->bandEvents[2 * b], s));
      HIP_TRY(hipStreamWaitEvent(cs, c->bandEvents[2 * b], 0));
      HIP_TRY(hipMemcpyAsync(hBits + (size_t)bp.seedBase * kMatchWords, (unsigned long long *)c->bMatch.p + (size_t)bp.seedBase * kMatchWords, (size_t)bp.seedCount * kMatchWords * 8,
                             hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipMemcpyAsync(hFlags + bp.seedBase, (uint8_t *)c->bFlags.p + bp.seedBase, bp.seedCount, hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipEventRecord(c->bandEvents[2 * b + 1], cs));
      if (b == 1 || (b == 0 && nBands == 1))
        if ((r = copy_records()) != limg_hip_success) return r;
    }
    HIP_TRY(hipEventRecord(frontTimers[2], s)); // (`s` holds nothing but the similarity kernels between the two timers: the copies run on `cs`)
    HIP_TRY(hipEventSynchronize(c->bandEvents[1])); // the first band's bits: the merge can start
    const clk::time_point t1 = clk::now();
    uint32_t bandsReady = 0;
    bool bandError = false, recordsHere = false;
    const std::function<void()> needRecords = [&]() {
      if (!recordsHere && hipEventSynchronize(evPass1) != hipSuccess) bandError = true;
      recordsHere = true;
    };
    const std::function<void(uint32_t)> needSeedRow = [&](uint32_t row) {
      while (bandsReady < nBands && row >= bandsReady * bandRows)
      {
        if (hipEventSynchronize(c->bandEvents[2 * bandsReady + 1]) != hipSuccess) bandError = true;
        bandsReady++;
      }
    };

    // Everything after this point is a two-thread pipeline.  This thread runs the greedy raster merge (serial by construction; it only looks the
    // similarity bits up) and publishes finished rectangles every few thousand; a worker thread takes them batch by batch, in creation order:
    // fit + search kernel, copy of the shift words, dither chain walk for the batch (the chain is serial too, but independent of the merge),
    // noise upload, store kernel.  Buffers are sized for the worst case up front so that nothing is reallocated while both threads run.
    const size_t px = sizeX * sizeY;
    const uint64_t capMax = ((uint64_t)px + 3ull * blocks + 3ull) & ~3ull; // every rectangle's scratch slice is rounded up to a multiple of 4
    if (capMax > 0xFFFFFFF0ull) return limg_hip_error_InvalidParameter;
    if ((r = c->hDesc.ensure(blocks * sizeof(RegionDesc))) != limg_hip_success) return r;
    if ((r = c->hOut.ensure(blocks * sizeof(RegionOut))) != limg_hip_success) return r;
    if ((r = c->hNoiseBase.ensure(blocks * 8 + 8)) != limg_hip_success) return r;
    const size_t maxCalls = 3 * blocks; // per dither call: the chain value it starts from (8 B), where its noise bytes go (8 B), its pixel count (4 B)
    if ((r = c->hNoise.ensure(maxCalls * 20 + 64)) != limg_hip_success) return r;
    if ((r = c->bCalls.ensure(maxCalls * 20 + 64)) != limg_hip_success) return r;
    if ((r = c->bRegions.ensure(blocks * sizeof(RegionDesc))) != limg_hip_success) return r;
    if ((r = c->bOut.ensure(blocks * sizeof(RegionOut))) != limg_hip_success) return r;
    if ((r = c->bNoiseBase.ensure(blocks * 8 + 8)) != limg_hip_success) return r;
    if ((r = c->bOrder.ensure(blocks * 4)) != limg_hip_success) return r;
    if ((r = c->bNoise.ensure(3 * px + 64)) != limg_hip_success) return r;
    if ((r = c->bPx.ensure(capMax * 4)) != limg_hip_success) return r;
    if ((r = c->bFac.ensure(capMax * 3)) != limg_hip_success) return r;
    if (!c->workStream) HIP_TRY(hipStreamCreateWithFlags(&c->workStream, hipStreamNonBlocking));
    RegionDesc *desc = (RegionDesc *)c->hDesc.p;
    RegionOut *hOut = (RegionOut *)c->hOut.p;
    unsigned long long *noiseBase = (unsigned long long *)c->hNoiseBase.p;
    unsigned long long *callState = (unsigned long long *)c->hNoise.p, *callOff = callState + maxCalls;
    uint32_t *callPx = (uint32_t *)(callOff + maxCalls);
    unsigned long long *dCallState = (unsigned long long *)c->bCalls.p, *dCallOff = dCallState + maxCalls;
    uint32_t *dCallPx = (uint32_t *)(dCallOff + maxCalls);
    std::vector<uint32_t> npx(blocks);
    bp.scratchPx = (uint32_t *)c->bPx.p; bp.scratchFac = (uint8_t *)c->bFac.p; bp.scratchCap = (uint32_t)capMax;
    {
      // k_blocked_store's 4-pixels-per-lane form: whole blocks (every rectangle row is a multiple of 8 pixels, every scratch / noise offset a multiple of 4) and planes
      // whose rows start 16-byte (32-bit planes) / 4-byte (byte planes) aligned
      const limg_hip_blocked_encode3d_info &bi = bp.info;
      uintptr_t w = 0, b8 = 0;
      const void *words[] = { bi.pDecoded, bi.pShiftABCX, bi.pColAMin, bi.pColAMax, bi.pColBMin, bi.pColBMax, bi.pColCMin, bi.pColCMax, bi.pBlockIndex };
      const void *bytes[] = { bi.pFactorsA, bi.pFactorsB, bi.pFactorsC, bi.pBitsPerPixel };
      for (const void *q : words) w |= (uintptr_t)q;
      for (const void *q : bytes) b8 |= (uintptr_t)q;
      bp.vecStore = (sizeX % kBlock == 0 && sizeY % kBlock == 0 && (w & 15u) == 0 && (b8 & 3u) == 0 && TOPT(c, blocked_no_vec_store) == 0) ? 1 : 0;
    }
    bp.noise = (const uint8_t *)c->bNoise.p;

    struct Pipe { std::mutex m; std::condition_variable cv; size_t ready = 0; bool finished = false; } pipe;
    limg_hip_result workerResult = limg_hip_success;
    double busy[3] = { 0, 0, 0 }; // worker: fit + search (incl. copies), chain walk, store launch
    const bool pcg = c->opt.dither_pcg != 0;
    // One batch = everything the merge has published when the worker looks; one stream for the fit + search kernels.  Measured on one box (profiles/archive/r04_blocked_pipeline.md):
    // batches capped at 8 K ... 64 K rectangles, two or four streams round-robin, a high-priority stream -- all within +-2 ms of this, most of them worse: the GPU
    // (similarity kernels 13 ms + fit / search kernels 13 ms per 8192^2 image) is as busy as the two host threads, so reordering its queue buys nothing.
    constexpr size_t kBatchRegions = (size_t)1 << 30;
    constexpr size_t kWorkStreams = 1;
    while (c->workStreams.size() < kWorkStreams)
    {
      hipStream_t st;
      HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      c->workStreams.push_back(st);
    }
    if (!c->storeStream) HIP_TRY(hipStreamCreateWithFlags(&c->storeStream, hipStreamNonBlocking));
    hipStream_t ss = c->storeStream; // noise expansion + store kernels of a batch: beside the next batch's fit + search kernel, not behind it

    while (c->workEvents.size() < kInFlight)
    {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      c->workEvents.push_back(e);
    }

    double kernelMs[2] = { 0, 0 };
    std::vector<uint8_t> storeTimed(kInFlight, 0); // slot i's store timers hold a finished-or-enqueued interval that has not been added up yet

    std::thread worker([&]() {
      if (hipSetDevice(c->device) != hipSuccess) { workerResult = limg_hip_error_Generic; }
      // The GPU runs AHEAD of this thread: whatever the merge has published goes to the device at once (rectangle table up, fit + search kernel, records and
      // shift words back, one event per batch, up to kInFlight batches), and the chain -- this thread's real work, serial by construction -- is walked batch by batch
      // in creation order as the results arrive.  (Rounds 2-3 kept one batch in flight: every batch's GPU round trip was waited for, 11-20 ms per image.)
      struct Batch { size_t r0 = 0, r1 = 0; size_t ev = 0; };
      std::vector<Batch> queue; // FIFO: [head, queue.size())
      size_t head = 0, issued = 0, evNext = 0;
      uint64_t chain = kDitherSeed, noiseOff = 0;
      size_t callCount = 0;
      bool fin = false;
      constexpr size_t kOrderFrom = 512; // batches from this many rectangles on get the device-side "large rectangles first" order (k_blocked_order)
      auto params_of = [&](const Batch &b) {
        BlockedParams q = bp;
        q.regions = (const RegionDesc *)c->bRegions.p + b.r0; q.nRegions = (uint32_t)(b.r1 - b.r0); q.regionBase = (uint32_t)b.r0;
        q.out = (RegionOut *)c->bOut.p + b.r0;
        q.noiseBase = (const unsigned long long *)c->bNoiseBase.p + b.r0;
        q.order = (b.r1 - b.r0 >= kOrderFrom && TOPT(c, blocked_no_order) == 0) ? (uint32_t *)c->bOrder.p + b.r0 : nullptr; // (a small batch is one round of workgroups anyway)
        return q;
      };
      // Everything the merge has published since the last look goes to the GPU.  mayWait: nothing is left to walk, so wait for the merge.  Called at the top of
      // every round AND between the pieces of a batch's chain walk: a batch's walk takes milliseconds, and what the merge publishes meanwhile should be on the GPU
      // (kernel latency: the life of its largest rectangle, 0.6-2 ms) before this thread comes looking for it -- not be enqueued when the walk is over.
      // A kernel's duration is the life of its largest rectangle whatever the batch's size and the batches of a stream run one after the other, so a look from
      // inside a walk (minNew > 0) takes a batch only when it is worth a launch; a look with nothing else to do takes whatever there is.
      // (same-box A/B of these three and of the merge's first report, tools/r04/run38.sh: photo-noise 27.5-27.7 ms against 28.8-32.0 with "any size, looks every
      //  8192 rectangles, first report at 4096", gradient 20.3-20.4 against 19.9-21.1)
      constexpr size_t kWorthWithOneInFlight = 16384, kWorthFromInsideAWalk = 8192, kWalkPiece = 2048;
      auto enqueue_published = [&](bool mayWait, size_t minNew = 0)
      {
        if (fin || queue.size() - head >= kInFlight) return;
        size_t r0 = 0, r1 = 0;
        {
          std::unique_lock<std::mutex> lk(pipe.m);
          if (mayWait) pipe.cv.wait(lk, [&] { return pipe.ready > issued || pipe.finished; });
          if (pipe.ready > issued && (pipe.ready - issued >= minNew || pipe.finished)) { r0 = issued; r1 = pipe.ready - issued > kBatchRegions ? issued + kBatchRegions : pipe.ready; issued = r1; }
          else if (pipe.ready > issued) {}
          else fin = pipe.finished;
        }
        if (r1 <= r0) return;
        Batch nb; nb.r0 = r0; nb.r1 = r1; nb.ev = evNext; evNext = (evNext + 1) % kInFlight;
        if (storeTimed[nb.ev])
        { // the slot comes round again: its previous batch's store kernels were enqueued kInFlight batches ago
          float t = 0;
          if (hipEventSynchronize(c->workTimers[4 * nb.ev + 3]) == hipSuccess && hipEventElapsedTime(&t, c->workTimers[4 * nb.ev + 2], c->workTimers[4 * nb.ev + 3]) == hipSuccess) kernelMs[1] += t;
          storeTimed[nb.ev] = 0;
        }
        if (workerResult == limg_hip_success)
        {
          const size_t n = r1 - r0;
          const BlockedParams q = params_of(nb);
          hipStream_t bs = c->workStreams[nb.ev % kWorkStreams];
          bool ok = hipMemcpyAsync((RegionDesc *)c->bRegions.p + r0, desc + r0, n * sizeof(RegionDesc), hipMemcpyHostToDevice, bs) == hipSuccess;
          ok = ok && hipEventRecord(c->workTimers[4 * nb.ev], bs) == hipSuccess;
          if (ok) { launch_blocked_order(q, bs); launch_blocked_fit_search(q, bs); ok = hipGetLastError() == hipSuccess; }
          ok = ok && hipEventRecord(c->workTimers[4 * nb.ev + 1], bs) == hipSuccess;
          ok = ok && hipMemcpyAsync(hOut + r0, (RegionOut *)c->bOut.p + r0, n * sizeof(RegionOut), hipMemcpyDeviceToHost, bs) == hipSuccess;
          ok = ok && hipEventRecord(c->workEvents[nb.ev], bs) == hipSuccess;
          if (!ok) workerResult = limg_hip_error_Generic;
        }
        queue.push_back(nb);
      };
      for (;;)
      {
        const clk::time_point w0 = clk::now();
        enqueue_published(head == queue.size(), head == queue.size() ? 0 : kWorthWithOneInFlight); // (with a batch in flight to wait for and walk, small change accumulates meanwhile)
        // 2. the oldest batch in flight: its shift words are (about to be) back
        if (head < queue.size())
        {
          const Batch pending = queue[head++];
          if (workerResult == limg_hip_success)
          {
            bool ok = hipEventSynchronize(c->workEvents[pending.ev]) == hipSuccess;
            {
              float t = 0;
              if (ok && hipEventElapsedTime(&t, c->workTimers[4 * pending.ev], c->workTimers[4 * pending.ev + 1]) == hipSuccess) kernelMs[0] += t;
            }
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
              chain = chain_walk_batch(chain, n, reinterpret_cast<const uint8_t *>(&hOut[w].shiftWord), sizeof(RegionOut), npx.data() + w, noiseBase + w, callState, callOff, callPx,
                                       noiseOff, callCount, maxCalls, pcg);
              if (w + n < pending.r1) enqueue_published(false, kWorthFromInsideAWalk);
            }
            const clk::time_point w2 = clk::now();
            const BlockedParams q = params_of(pending);
            const size_t nc = callCount - call0;
            ok = ok && hipStreamWaitEvent(ss, c->workEvents[pending.ev], 0) == hipSuccess; // this batch's records and shift words are in bOut
            ok = ok && hipEventRecord(c->workTimers[4 * pending.ev + 2], ss) == hipSuccess;
            if (ok && nc)
            {
              ok = hipMemcpyAsync(dCallState + call0, callState + call0, nc * 8, hipMemcpyHostToDevice, ss) == hipSuccess &&
                   hipMemcpyAsync(dCallOff + call0, callOff + call0, nc * 8, hipMemcpyHostToDevice, ss) == hipSuccess &&
                   hipMemcpyAsync(dCallPx + call0, callPx + call0, nc * 4, hipMemcpyHostToDevice, ss) == hipSuccess;
              if (ok) { launch_noise_expand_calls((uint8_t *)c->bNoise.p, dCallState + call0, dCallOff + call0, dCallPx + call0, nc, pcg, ss); ok = hipGetLastError() == hipSuccess; }
            }
            ok = ok && hipMemcpyAsync((unsigned long long *)c->bNoiseBase.p + pending.r0, noiseBase + pending.r0, (pending.r1 - pending.r0) * 8, hipMemcpyHostToDevice, ss) == hipSuccess;
            if (ok) { launch_blocked_store(q, ss); ok = hipGetLastError() == hipSuccess; }
            if (ok && hipEventRecord(c->workTimers[4 * pending.ev + 3], ss) == hipSuccess) storeTimed[pending.ev] = 1;
            const clk::time_point w3 = clk::now();
            busy[0] += ms(w0, w1); busy[1] += ms(w1, w2); busy[2] += ms(w2, w3);
            if (!ok) workerResult = limg_hip_error_Generic;
          }
        }
        if (fin && head == queue.size()) break;
      }
      for (hipStream_t st : c->workStreams)
        if (hipStreamSynchronize(st) != hipSuccess && workerResult == limg_hip_success) workerResult = limg_hip_error_Generic;
      if (hipStreamSynchronize(ss) != hipSuccess && workerResult == limg_hip_success) workerResult = limg_hip_error_Generic;
      for (size_t i = 0; i < kInFlight; i++)
        if (storeTimed[i])
        {
          float t = 0;
          if (hipEventElapsedTime(&t, c->workTimers[4 * i + 2], c->workTimers[4 * i + 3]) == hipSuccess) kernelMs[1] += t;
        }
    });

    // producer: the merge; its progress callback lays the finished rectangles out (pixel counts, scratch slices) and hands them over
    size_t laid = 0;
    uint64_t cap = 0;
    const std::function<void(size_t)> progress = [&](size_t count) {
      const std::vector<HostRegion> &regs = c->lastRegions;
      for (size_t i = laid; i < count; i++)
      {
        const HostRegion &h = regs[i];
        size_t xpx = (size_t)h.rx * kBlock, ypx = (size_t)h.ry * kBlock;
        if (h.ox + h.rx == blocksX && (sizeX % kBlock)) xpx = xpx - kBlock + sizeX % kBlock;
        if (h.oy + h.ry == blocksY && (sizeY % kBlock)) ypx = ypx - kBlock + sizeY % kBlock;
        npx[i] = (uint32_t)(xpx * ypx);
        desc[i] = { h.ox, h.oy, h.rx, h.ry, h.keep, (uint32_t)cap, { 0, 0 } };
        cap += ((uint64_t)npx[i] + 3) & ~3ull;
      }
      laid = count;
      { std::lock_guard<std::mutex> lk(pipe.m); pipe.ready = count; }
      pipe.cv.notify_one();
    };
    bool mergeFailed = false;
    try { blocked_merge(hRec, hBits, blocksX, blocksY, channels, c->lastRegions, &progress, &needSeedRow, hFlags, &needRecords); }
    catch (...) { mergeFailed = true; } // out of host memory: the worker must still be released and joined
    needSeedRow(blocksY - 1); // every band's copy is complete before the staging buffers can be reused
    needRecords();
    const clk::time_point t2 = clk::now();
    { std::lock_guard<std::mutex> lk(pipe.m); pipe.finished = true; }
    pipe.cv.notify_one();
    worker.join();
    const clk::time_point t5 = clk::now();
    {
      float a = 0, b = 0; // (both intervals ended before the merge's last band arrived)
      const bool ok = hipEventElapsedTime(&a, frontTimers[0], frontTimers[1]) == hipSuccess && hipEventElapsedTime(&b, frontTimers[1], frontTimers[2]) == hipSuccess;
      c->blockedKernelMs[0] = ok ? a : 0; c->blockedKernelMs[1] = ok ? b : 0;
    }
    c->blockedKernelMs[2] = kernelMs[0]; c->blockedKernelMs[3] = kernelMs[1];
    c->blockedMs[0] = ms(t0, t1); c->blockedMs[1] = ms(t1, t2); c->blockedMs[2] = busy[0]; c->blockedMs[3] = busy[1]; c->blockedMs[4] = busy[2]; c->blockedMs[5] = ms(t0, t5);
    if (mergeFailed) return limg_hip_error_MemoryAllocationFailure;
    if (bandError) return limg_hip_error_Generic;
    if (workerResult == limg_hip_success && c->opt.collect_stats)
    { // src/limg.cpp:1561-1590 per rectangle: (8 - shift) bits for each of its pixels, and the pixels by shift
      memset(c->statsHost, 0, sizeof(c->statsHost));
      for (size_t i = 0; i < c->lastRegions.size(); i++)
        for (int f = 0; f < 3; f++)
        {
          uint32_t sh = (hOut[i].shiftWord >> (8 * f)) & 0xFFu;
          if (sh > 8) sh = 8;
          c->statsHost[f] += (uint64_t)(8 - sh) * npx[i];
          c->statsHost[3 + 9 * f + sh] += npx[i];
        }
      c->statsState = 2; c->statsPixels = (uint64_t)sizeX * sizeY;
    }
    return workerResult;
  }

  limg_hip_result limg_hip_blocked_regions(limg_hip_context *c, limg_hip_region *pRegions, size_t capacity, size_t *pCount)
  {
    if (!c || !pCount) return limg_hip_error_ArgumentNull;
    *pCount = c->lastRegions.size();
    if (pRegions)
      for (size_t i = 0; i < c->lastRegions.size() && i < capacity; i++) pRegions[i] = { c->lastRegions[i].ox, c->lastRegions[i].oy, c->lastRegions[i].rx, c->lastRegions[i].ry };
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_timing(limg_hip_context *c, double *pMs6)
  {
    if (!c || !pMs6) return limg_hip_error_ArgumentNull;
    memcpy(pMs6, c->blockedMs, sizeof(c->blockedMs));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_match_bits(limg_hip_context *c, uint64_t *pBits, size_t capacityWords, size_t *pWords)
  { // the similarity bits the last merged-block encode's merge worked from (they stay in the context's pinned staging buffer until the next encode)
    if (!c || !pWords) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const size_t words = c->lastBlocks * kMatchWords;
    *pWords = words;
    if (pBits && c->hBits.p) memcpy(pBits, c->hBits.p, (words < capacityWords ? words : capacityWords) * 8);
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_kernel_timing(limg_hip_context *c, double *pMs4)
  {
    if (!c || !pMs4) return limg_hip_error_ArgumentNull;
    memcpy(pMs4, c->blockedKernelMs, sizeof(c->blockedKernelMs));
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
    if ((r = c->in.ensure(px * 4)) != limg_hip_success) return r;
    if ((r = c->planes.ensure(stride * 13)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->in.p, pIn, px * 4, hipMemcpyHostToDevice));
    uint8_t *base = (uint8_t *)c->planes.p;
    limg_hip_blocked_encode3d_info d;
    memset(&d, 0, sizeof(d));
    // 13 written planes, one `stride` each (the uint8 ones use a quarter of theirs)
    void **hostp[13] = { (void **)&pInfo->pDecoded, (void **)&pInfo->pFactorsA, (void **)&pInfo->pFactorsB, (void **)&pInfo->pFactorsC, (void **)&pInfo->pBitsPerPixel,
                         (void **)&pInfo->pShiftABCX, (void **)&pInfo->pColAMin, (void **)&pInfo->pColAMax, (void **)&pInfo->pColBMin, (void **)&pInfo->pColBMax,
                         (void **)&pInfo->pColCMin, (void **)&pInfo->pColCMax, (void **)&pInfo->pBlockIndex };
    void **devp[13] = { (void **)&d.pDecoded, (void **)&d.pFactorsA, (void **)&d.pFactorsB, (void **)&d.pFactorsC, (void **)&d.pBitsPerPixel, (void **)&d.pShiftABCX,
                        (void **)&d.pColAMin, (void **)&d.pColAMax, (void **)&d.pColBMin, (void **)&d.pColBMax, (void **)&d.pColCMin, (void **)&d.pColCMax, (void **)&d.pBlockIndex };
    const bool is8[13] = { false, true, true, true, true, false, false, false, false, false, false, false, false };
    for (int i = 0; i < 13; i++)
    {
      if (!*hostp[i]) return limg_hip_error_ArgumentNull;
      *devp[i] = base + stride * i;
    }
    if ((r = limg_hip_blocked_encode3d_device(c, (const uint32_t *)c->in.p, sizeX, sizeY, hasAlpha, &d, errorFactor, fastBitCrushing, nullptr)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    for (int i = 0; i < 13; i++) HIP_TRY(hipMemcpy(*hostp[i], *devp[i], is8[i] ? px : px * 4, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }
}
