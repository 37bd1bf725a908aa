// limg_hip_stream_api.hip -- the compact stream entries of the C ABI, both versions: encode, batched encode, whole-image decode, header check and the host-pointer
// forms of each.  Version 1: 8x8 encode in compact mode + the packer of limg_hip_stream.hip.  Version 2: the merged-block encoder in compact mode
// (blocked_encode_device without planes, limg_hip_blocked_api.hip) + the scan and pack kernels of limg_hip_blocked_stream.hip; its whole-image decode is a window
// decode.  What the two versions do alike is written once, in the anonymous namespace below.  The window entries: limg_hip_stream_window_api.hip.
#include "limg_hip_context.h"

#include <algorithm>
#include <vector>

using namespace limg_hip;

// ---- shared with limg_hip_stream_window_api.hip (declared in limg_hip_context.h) ----
int limg_hip::device_cus(const limg_hip_context *c) { return c->enc.persistentWorkgroups / 5; }

// the status word the stream decoders share (limg_hip_check_device_status reads it), then the version 1 decode kernel's store sink (see DecodeParams::sink)
limg_hip_result limg_hip::ensure_stream_status(limg_hip_context *c, hipStream_t s)
{
  if (c->stream.status.p) return limg_hip_success;
  const limg_hip_result r = c->stream.status.ensure(256 + 2048);
  if (r != limg_hip_success) return r;
  HIP_TRY(hipMemsetAsync(c->stream.status.p, 0, 8, s));
  return limg_hip_success;
}

namespace
{
  // what the packer's scan left in the stream's header; waits for `s`
  limg_hip_result stream_total_bytes(const uint8_t *dStream, hipStream_t s, size_t *pBytes)
  {
    limg_hip_stream_header h;
    HIP_TRY(hipMemcpyAsync(&h, dStream, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *pBytes = (size_t)h.totalBytes;
    return limg_hip_success;
  }

  // ---- header check: limg_hip_stream_info / limg_hip_blocked_stream_info ----
  limg_hip_result read_header(const uint8_t *pStream, size_t streamBytes, uint32_t version, limg_hip_stream_header &h)
  {
    if (!pStream) return limg_hip_error_ArgumentNull;
    if (streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_OutOfBounds;
    memcpy(&h, pStream, sizeof(h));
    if (h.magic != LIMG_HIP_STREAM_MAGIC || h.version != version || (h.channels != 3 && h.channels != 4)) return limg_hip_error_InvalidParameter;
    return limg_hip_success;
  }
  // `h` (its sizes accepted by the version's bound already) against a table of `entries` entries of `entryBytes`
  limg_hip_result check_header_table(const limg_hip_stream_header &h, uint64_t entries, size_t entryBytes, size_t *pSizeX, size_t *pSizeY, int *pHasAlpha, size_t *pTotalBytes)
  {
    const uint64_t bx = ((uint64_t)h.sizeX + kBlock - 1) / kBlock, by = ((uint64_t)h.sizeY + kBlock - 1) / kBlock;
    if (h.blocksX != bx || h.blocksY != by || entries == 0 || entries > bx * by) return limg_hip_error_InvalidParameter;
    if (h.payloadWords > bx * by * 24 || h.totalBytes != sizeof(h) + entries * entryBytes + h.payloadWords * 8) return limg_hip_error_InvalidParameter;
    if (pSizeX) *pSizeX = h.sizeX;
    if (pSizeY) *pSizeY = h.sizeY;
    if (pHasAlpha) *pHasAlpha = h.channels == 4;
    if (pTotalBytes) *pTotalBytes = (size_t)h.totalBytes;
    return limg_hip_success;
  }

  // ---- host-pointer forms: upload, the version's device entry on the null stream, status, download ----
  // the stream in the context's stream.buf to the caller: *pBytes says what it takes even where `capacity` is too small
  limg_hip_result download_stream(limg_hip_context *c, size_t bytes, uint8_t *pStream, size_t capacity, size_t *pBytes)
  {
    *pBytes = bytes;
    if (bytes > capacity) return limg_hip_error_OutOfBounds;
    HIP_TRY(hipMemcpy(pStream, c->stream.buf.p, bytes, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  // deviceEncode(dIn, dStream, bound, &bytes)
  template <class ENCODE>
  limg_hip_result encode_stream_host(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, uint8_t *pStream, size_t capacity, size_t *pBytes, size_t bound,
                                     ENCODE &&deviceEncode)
  {
    if (bound == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    const size_t px = sizeX * sizeY;
    if ((r = c->host.in.ensure(px * 4)) != limg_hip_success) return r;
    if ((r = c->stream.buf.ensure(bound)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->host.in.p, pIn, px * 4, hipMemcpyHostToDevice));
    size_t bytes = 0;
    if ((r = deviceEncode((const uint32_t *)c->host.in.p, (uint8_t *)c->stream.buf.p, bound, &bytes)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    return download_stream(c, bytes, pStream, capacity, pBytes);
  }

  // sizeX, sizeY, total: from the version's header check.  deviceDecode(dStream, total, dOut, sizeX, sizeY); a refused stream: nothing reaches pOut
  template <class DECODE>
  limg_hip_result decode_stream_host(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t outPixels, size_t sizeX, size_t sizeY, size_t total,
                                     DECODE &&deviceDecode)
  {
    if (total > streamBytes || sizeX * sizeY > outPixels) return limg_hip_error_OutOfBounds;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = c->stream.buf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->host.planes.ensure(sizeX * sizeY * 4)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->stream.buf.p, pStream, total, hipMemcpyHostToDevice));
    if ((r = deviceDecode((const uint8_t *)c->stream.buf.p, total, (uint32_t *)c->host.planes.p, sizeX, sizeY)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(pOut, c->host.planes.p, sizeX * sizeY * 4, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  // ---- size probe and budget search (kernels: limg_hip_rate.hip; the search: limg_hip_rate_step.h) ----
  // the probe kernel's domain: whole 8x8 blocks, the persistent path's float stage (k_fit_tpb), the default search
  bool rate_probe_applies(const limg_hip_context *c, size_t sizeX, size_t sizeY, int fast)
  {
    return (sizeX % kBlock) == 0 && (sizeY % kBlock) == 0 && c->opt.force_split_kernels == 0 && c->opt.legacy_float_stage == 0 && fast != 0;
  }

  uint64_t stream_fixed_bytes(size_t sizeX, size_t sizeY)
  {
    return sizeof(limg_hip_stream_header) + (uint64_t)((sizeX + kBlock - 1) / kBlock) * ((sizeY + kBlock - 1) / kBlock) * sizeof(limg_hip_stream_block);
  }

  // The records of k_fit_tpb (the `fitOnly` route, which the merged-block encoder's pass 1 also takes) and the probe's parameters on them; the state and the counter.
  limg_hip_result rate_probe_setup(limg_hip_context *c, const uint32_t *dIn, size_t sizeX, size_t sizeY, int hasAlpha, int poolThreads, hipStream_t s, RateProbeParams &rp)
  {
    limg_hip_result r;
    if ((r = c->stream.rateState.ensure(sizeof(RateDevice))) != limg_hip_success) return r;
    if ((r = c->stream.rateCounter.ensure(8)) != limg_hip_success) return r;
    EncodeExtra x;
    x.fitOnly = true; x.fitFloatMode = true;
    if ((r = encode_device(c, dIn, sizeX, sizeY, hasAlpha, nullptr, nullptr, 0, poolThreads, 1, s, x)) != limg_hip_success) return r;
    memset(&rp, 0, sizeof(rp));
    rp.io.in = dIn;
    rp.sizeX = (uint32_t)sizeX; rp.sizeY = (uint32_t)sizeY; rp.blocksX = (uint32_t)(sizeX / kBlock); rp.blocksY = (uint32_t)(sizeY / kBlock);
    rp.stripsX = (rp.blocksX + kStripBlocks - 1) / kStripBlocks;
    rp.vecIn = (sizeX % 4 == 0) && (((uintptr_t)dIn) & 15u) == 0; // as encode_params
    rp.recordLimit = TOPT(c, record_limit) > 0 ? TOPT(c, record_limit) - 1 : 2700;
    const bool forced = c->opt.forced_shift[0] >= 0 && c->opt.forced_shift[0] <= 8 && c->opt.forced_shift[1] >= 0 && c->opt.forced_shift[1] <= 8 &&
                        c->opt.forced_shift[2] >= 0 && c->opt.forced_shift[2] <= 8;
    for (int i = 0; i < 3; i++) rp.forced[i] = forced ? c->opt.forced_shift[i] : -1;
    rp.records = (const limg_hip_block_record *)c->enc.records.p; rp.invN = (const float *)c->enc.invN.p;
    rp.state = (const RateDevice *)c->stream.rateState.p; rp.counter = (unsigned long long *)c->stream.rateCounter.p;
    return limg_hip_success;
  }

  // minErrorFactor / maxErrorFactor / maxBytes / pResult of the budget entries -> the bounds of h = errorFactor / 2
  limg_hip_result budget_bounds(size_t maxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, const limg_hip_budget_result *pResult, uint32_t &hLo, uint32_t &hHi)
  {
    const uint32_t lo = minErrorFactor ? minErrorFactor : 2u, hi = maxErrorFactor ? maxErrorFactor : 1024u;
    if ((lo & 1u) || (hi & 1u) || lo < 2u || hi < 2u || lo > hi || maxBytes == 0 || pResult->struct_size < sizeof(limg_hip_budget_result)) return limg_hip_error_InvalidParameter;
    hLo = lo / 2u; hHi = hi / 2u;
    return limg_hip_success;
  }

  // ... of the list entries: the bound rules first (they hold for an empty list too), then every image's budget and result
  limg_hip_result budget_list_checks(size_t count, const size_t *pMaxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, const limg_hip_budget_result *pResults,
                                     uint32_t &hLo, uint32_t &hHi)
  {
    limg_hip_budget_result whole;
    whole.struct_size = sizeof(whole);
    const limg_hip_result r = budget_bounds(1, minErrorFactor, maxErrorFactor, &whole, hLo, hHi);
    if (r != limg_hip_success) return r;
    for (size_t i = 0; i < count; i++)
      if (pMaxBytes[i] == 0 || pResults[i].struct_size < sizeof(limg_hip_budget_result)) return limg_hip_error_InvalidParameter;
    return limg_hip_success;
  }

  // ---- version 2 ----
  // the packer's scratch for the worst case (every block its own rectangle): 4 bytes per block and 8 per 256 blocks; the two timing events
  limg_hip_result ensure_pack_resources(limg_hip_context *c, size_t sizeX, size_t sizeY)
  {
    const size_t blocks = ((sizeX + kBlock - 1) / kBlock) * ((sizeY + kBlock - 1) / kBlock);
    limg_hip_result r;
    if ((r = c->stream.bsUnits.ensure((blocks + 1) * 4)) != limg_hip_success) return r;
    if ((r = c->stream.bsTiles.ensure(((blocks + 255) / 256) * 8)) != limg_hip_success) return r;
    return c->stream.packTimers.ensure(2, hipEventDefault);
  }

  // The stream of the context's last merged-block encode, from what that left in the context's buffers (blocked_encode_device: with or without planes, the store step
  // does not change them): scan + pack on `s`.  pBytes (host, may be NULL) makes the call wait.
  limg_hip_result pack_last(limg_hip_context *c, uint8_t *dStream, size_t *pBytes, hipStream_t s)
  {
    const size_t sizeX = c->blocked.last.sizeX, sizeY = c->blocked.last.sizeY;
    const size_t blocksX = (sizeX + kBlock - 1) / kBlock, blocksY = (sizeY + kBlock - 1) / kBlock, blocks = blocksX * blocksY, nRegions = c->blocked.lastRegions.size();
    if (!c->blocked.last.valid || nRegions == 0 || nRegions > blocks) return limg_hip_error_Generic;
    BlockedStreamParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.sizeX = (uint32_t)sizeX; sp.sizeY = (uint32_t)sizeY; sp.blocksX = (uint32_t)blocksX; sp.blocksY = (uint32_t)blocksY;
    sp.channels = (uint32_t)c->blocked.last.channels; sp.errorFactor = c->blocked.last.errorFactor; sp.flags = c->blocked.last.flags;
    sp.nRegions = (uint32_t)nRegions; sp.nTiles = (uint32_t)((nRegions + 255) / 256); sp.scratchCap = (uint32_t)c->blocked.scratchCap;
    sp.regions = (const RegionDesc *)c->blocked.regions.p; sp.out = (const RegionOut *)c->blocked.out.p; sp.noiseBase = (const unsigned long long *)c->blocked.noiseBase.p;
    sp.scratchFac = (const uint8_t *)c->blocked.fac.p; sp.noise = (const uint8_t *)c->blocked.noise.p;
    sp.stream = dStream; sp.units = (uint32_t *)c->stream.bsUnits.p; sp.tiles = (uint32_t *)c->stream.bsTiles.p;
    HIP_TRY(hipEventRecord(c->stream.packTimers[0], s));
    launch_blocked_stream_pack(sp, device_cus(c), s);
    HIP_TRY(hipEventRecord(c->stream.packTimers[1], s));
    HIP_TRY(hipGetLastError());
    c->stream.packTimed = true;
    return pBytes ? stream_total_bytes(dStream, s, pBytes) : limg_hip_success;
  }
}

extern "C"
{
  size_t limg_hip_stream_bound(size_t sizeX, size_t sizeY)
  {
    if (sizeX == 0 || sizeY == 0 || sizeX > 0x7FFFFFF8ull || sizeY > 0x7FFFFFF8ull) return 0;
    const size_t blocks = ((sizeX + kBlock - 1) / kBlock) * ((sizeY + kBlock - 1) / kBlock);
    if (blocks * 24 > 0xFFFFFFFFull) return 0; // entry.payloadWord is 32 bits
    return sizeof(limg_hip_stream_header) + blocks * sizeof(limg_hip_stream_block) + blocks * 192;
  }

  limg_hip_result limg_hip_encode_stream_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                size_t *pBytes, uint32_t errorFactor, int poolThreads, int fastBitCrushing, void *stream)
  {
    if (!c || !pIn || !pStream) return limg_hip_error_ArgumentNull;
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (capacity < bound) return limg_hip_error_OutOfBounds;
    if (((uintptr_t)pStream & 15u) != 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t px = sizeX * sizeY, planeStride = (px + 255) & ~(size_t)255;
    const size_t blocksX = (sizeX + kBlock - 1) / kBlock, blocksY = (sizeY + kBlock - 1) / kBlock, blocks = blocksX * blocksY;
    const size_t tiles = (blocks + 255) / 256;
    limg_hip_result r;
    if ((r = c->stream.fac.ensure(planeStride * 3)) != limg_hip_success) return r;
    // strip form of the packer (images of whole blocks): the encode kernel leaves one payload-word count per work strip (limg_hip_stream.hip)
    const size_t stripsX = (blocksX + kStripBlocks - 1) / kStripBlocks, nStrips = stripsX * blocksY;
    const bool stripForm = (sizeX % kBlock) == 0 && (sizeY % kBlock) == 0 && c->opt.force_split_kernels == 0;
    if ((r = c->stream.tiles.ensure(tiles * 4)) != limg_hip_success) return r;
    if (stripForm && (r = c->stream.units.ensure(nStrips * 4)) != limg_hip_success) return r;
    if ((r = c->enc.records.ensure(blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
    if ((r = c->enc.shifts.ensure(blocks * 4)) != limg_hip_success) return r;
    limg_hip_encode3d_info info;
    memset(&info, 0, sizeof(info));
    info.pFactorsA = (uint8_t *)c->stream.fac.p; info.pFactorsB = info.pFactorsA + planeStride; info.pFactorsC = info.pFactorsB + planeStride;
    limg_hip_compact_out comp = { (limg_hip_block_record *)c->enc.records.p, (uint32_t *)c->enc.shifts.p };
    EncodeExtra xs;
    xs.streamRaw = true;
    xs.stripWords = stripForm ? (uint32_t *)c->stream.units.p : nullptr;
    if ((r = encode_device(c, pIn, sizeX, sizeY, hasAlpha, &info, &comp, errorFactor, poolThreads, fastBitCrushing, s, xs)) != limg_hip_success) return r;

    StreamParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.sizeX = (uint32_t)sizeX; sp.sizeY = (uint32_t)sizeY; sp.blocksX = (uint32_t)blocksX; sp.blocksY = (uint32_t)blocksY;
    sp.nBlocks = (uint32_t)blocks; sp.nTiles = (uint32_t)tiles; sp.channels = hasAlpha ? 4 : 3; sp.errorFactor = errorFactor;
    sp.flags = (fastBitCrushing ? 1u : 0u) | (c->opt.dither_pcg ? 2u : 0u);
    sp.fac[0] = info.pFactorsA; sp.fac[1] = info.pFactorsB; sp.fac[2] = info.pFactorsC;
    sp.records = comp.pRecords; sp.shifts = comp.pShifts;
    sp.stream = pStream; sp.tileBase = (uint32_t *)c->stream.tiles.p;
    if (stripForm)
    {
      sp.stripWords = (uint32_t *)c->stream.units.p;
      sp.stripsX = (uint32_t)stripsX; sp.nStrips = (uint32_t)nStrips;
      const size_t slots = (size_t)device_cus(c) * 16; // 16 one-wave workgroups per CU (128 vector registers each: 4 per SIMD)
      sp.nWaves = (uint32_t)(nStrips < slots ? nStrips : slots);
    }
    mark(c, s);
    launch_stream_pack(sp, s);
    mark(c, s); mark(c, s); mark(c, s);
    HIP_TRY(hipGetLastError());
    return pBytes ? stream_total_bytes(pStream, s, pBytes) : limg_hip_success;
  }

  limg_hip_result limg_hip_decode_stream_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t sizeX, size_t sizeY, void *stream)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    if (limg_hip_stream_bound(sizeX, sizeY) == 0 || streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_InvalidParameter;
    if (((uintptr_t)pStream & 15u) != 0 || ((uintptr_t)pOut & 15u) != 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    limg_hip_result r;
    if ((r = ensure_stream_status(c, s)) != limg_hip_success) return r;
    DecodeParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.sizeX = (uint32_t)sizeX; dp.sizeY = (uint32_t)sizeY;
    dp.blocksX = (uint32_t)((sizeX + kBlock - 1) / kBlock); dp.blocksY = (uint32_t)((sizeY + kBlock - 1) / kBlock);
    dp.nBlocks = dp.blocksX * dp.blocksY;
    if (streamBytes < sizeof(limg_hip_stream_header) + (size_t)dp.nBlocks * sizeof(limg_hip_stream_block)) return limg_hip_error_OutOfBounds;
    dp.stream = pStream; dp.streamBytes = streamBytes; dp.out = pOut; dp.status = (uint32_t *)c->stream.status.p; dp.sink = (uint32_t *)((uint8_t *)c->stream.status.p + 256);
    mark(c, s);
    launch_stream_decode(dp, device_cus(c), s);
    mark(c, s); mark(c, s); mark(c, s);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  limg_hip_result limg_hip_stream_info(const uint8_t *pStream, size_t streamBytes, size_t *pSizeX, size_t *pSizeY, int *pHasAlpha, size_t *pTotalBytes)
  {
    limg_hip_stream_header h;
    const limg_hip_result r = read_header(pStream, streamBytes, LIMG_HIP_STREAM_VERSION, h);
    if (r != limg_hip_success) return r;
    if (limg_hip_stream_bound(h.sizeX, h.sizeY) == 0) return limg_hip_error_InvalidParameter;
    const uint64_t blocks = (((uint64_t)h.sizeX + kBlock - 1) / kBlock) * (((uint64_t)h.sizeY + kBlock - 1) / kBlock); // one entry per block
    return check_header_table(h, blocks, sizeof(limg_hip_stream_block), pSizeX, pSizeY, pHasAlpha, pTotalBytes);
  }

  limg_hip_result limg_hip_encode_stream(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity, size_t *pBytes,
                                         uint32_t errorFactor, int poolThreads, int fastBitCrushing)
  {
    if (!c || !pIn || !pStream || !pBytes) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    return encode_stream_host(c, pIn, sizeX, sizeY, pStream, capacity, pBytes, limg_hip_stream_bound(sizeX, sizeY), [&](const uint32_t *dIn, uint8_t *dStream, size_t bound, size_t *bytes) {
      return limg_hip_encode_stream_device(c, dIn, sizeX, sizeY, hasAlpha, dStream, bound, bytes, errorFactor, poolThreads, fastBitCrushing, nullptr);
    });
  }

  limg_hip_result limg_hip_decode_stream(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t outPixels)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    size_t sizeX = 0, sizeY = 0, total = 0;
    const limg_hip_result r = limg_hip_stream_info(pStream, streamBytes, &sizeX, &sizeY, nullptr, &total);
    if (r != limg_hip_success) return r;
    return decode_stream_host(c, pStream, streamBytes, pOut, outPixels, sizeX, sizeY, total, [&](const uint8_t *dStream, size_t bytes, uint32_t *dOut, size_t w, size_t h) {
      return limg_hip_decode_stream_device(c, dStream, bytes, dOut, w, h, nullptr);
    });
  }

  // ---- size probe and budget search (contract: include/limg_hip.h) ----
  limg_hip_result limg_hip_stream_sizes_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const uint32_t *pErrorFactors, size_t count,
                                               size_t *pBytes, int poolThreads, int fastBitCrushing, void *stream)
  {
    if (!c || !pIn || !pErrorFactors || !pBytes) return limg_hip_error_ArgumentNull;
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (count == 0) return limg_hip_success;
    if (count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    limg_hip_result r;
    if (!rate_probe_applies(c, sizeX, sizeY, fastBitCrushing))
    { // one ordinary stream encode per entry, into context staging
      if ((r = c->stream.buf.ensure(bound)) != limg_hip_success) return r;
      for (size_t i = 0; i < count; i++)
        if ((r = limg_hip_encode_stream_device(c, pIn, sizeX, sizeY, hasAlpha, (uint8_t *)c->stream.buf.p, bound, &pBytes[i], pErrorFactors[i], poolThreads, fastBitCrushing,
                                               stream)) != limg_hip_success)
          return r;
      return limg_hip_success;
    }
    if ((r = c->stream.rateList.ensure(count * 12)) != limg_hip_success) return r;
    RateProbeParams rp;
    if ((r = rate_probe_setup(c, pIn, sizeX, sizeY, hasAlpha, poolThreads, s, rp)) != limg_hip_success) return r;
    unsigned long long *dBytes = (unsigned long long *)c->stream.rateList.p;
    uint32_t *dList = (uint32_t *)(dBytes + count);
    std::vector<uint32_t> list(pErrorFactors, pErrorFactors + count); // (the caller's array may be pageable and may die when the call returns)
    HIP_TRY(hipMemcpyAsync(dList, list.data(), count * 4, hipMemcpyHostToDevice, s));
    launch_rate_begin((RateDevice *)c->stream.rateState.p, rp.counter, rate_begin(0, 0, 0), list[0], s);
    for (size_t i = 0; i < count; i++)
    {
      launch_rate_probe(rp, hasAlpha ? 4 : 3, c->opt.float_mode == 1, s);
      launch_rate_step((RateDevice *)c->stream.rateState.p, rp.counter, stream_fixed_bytes(sizeX, sizeY), dList, dBytes, (uint32_t)count, s);
    }
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> sizes(count);
    HIP_TRY(hipMemcpyAsync(sizes.data(), dBytes, count * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // (also: `list` is no longer read)
    for (size_t i = 0; i < count; i++) pBytes[i] = (size_t)sizes[i];
    return limg_hip_success;
  }

  limg_hip_result limg_hip_stream_sizes(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const uint32_t *pErrorFactors, size_t count,
                                        size_t *pBytes, int poolThreads, int fastBitCrushing)
  {
    if (!c || !pIn || !pErrorFactors || !pBytes) return limg_hip_error_ArgumentNull;
    if (limg_hip_stream_bound(sizeX, sizeY) == 0) return limg_hip_error_InvalidParameter;
    if (count == 0) return limg_hip_success;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = c->host.in.ensure(sizeX * sizeY * 4)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->host.in.p, pIn, sizeX * sizeY * 4, hipMemcpyHostToDevice));
    if ((r = limg_hip_stream_sizes_device(c, (const uint32_t *)c->host.in.p, sizeX, sizeY, hasAlpha, pErrorFactors, count, pBytes, poolThreads, fastBitCrushing, nullptr)) !=
        limg_hip_success)
      return r;
    return limg_hip_check_device_status(c);
  }

  limg_hip_result limg_hip_encode_stream_budget_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                       size_t maxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                       limg_hip_budget_result *pResult, void *stream)
  {
    if (!c || !pIn || !pStream || !pResult) return limg_hip_error_ArgumentNull;
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (capacity < bound) return limg_hip_error_OutOfBounds;
    if (((uintptr_t)pStream & 15u) != 0) return limg_hip_error_InvalidParameter;
    uint32_t hLo, hHi;
    limg_hip_result r;
    if ((r = budget_bounds(maxBytes, minErrorFactor, maxErrorFactor, pResult, hLo, hHi)) != limg_hip_success) return r;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    RateState st = rate_begin(hLo, hHi, maxBytes);
    size_t bytes = 0;
    bool written = false; // pStream holds the stream at the result
    if (rate_probe_applies(c, sizeX, sizeY, fastBitCrushing))
    { // every launch the search can need, enqueued at once; those behind its end return at once
      RateProbeParams rp;
      if ((r = rate_probe_setup(c, pIn, sizeX, sizeY, hasAlpha, poolThreads, s, rp)) != limg_hip_success) return r;
      launch_rate_begin((RateDevice *)c->stream.rateState.p, rp.counter, st, 2u * st.next, s);
      for (uint32_t i = 0, n = rate_max_probes(hLo, hHi); i < n; i++)
      {
        launch_rate_probe(rp, hasAlpha ? 4 : 3, c->opt.float_mode == 1, s);
        launch_rate_step((RateDevice *)c->stream.rateState.p, rp.counter, stream_fixed_bytes(sizeX, sizeY), nullptr, nullptr, 0, s);
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&st, c->stream.rateState.p, sizeof(st), hipMemcpyDeviceToHost, s)); // (RateDevice starts with the search's state)
      HIP_TRY(hipStreamSynchronize(s));
      if (!st.done) return limg_hip_error_Generic;
    }
    else
      while (!st.done)
      { // the same search, a whole stream encode per size
        const uint32_t h = st.next;
        if ((r = limg_hip_encode_stream_device(c, pIn, sizeX, sizeY, hasAlpha, pStream, capacity, &bytes, 2u * h, poolThreads, fastBitCrushing, stream)) != limg_hip_success) return r;
        rate_step(st, bytes);
        written = st.done && st.next == h;
      }
    if (!written && (r = limg_hip_encode_stream_device(c, pIn, sizeX, sizeY, hasAlpha, pStream, capacity, &bytes, 2u * st.next, poolThreads, fastBitCrushing, stream)) != limg_hip_success)
      return r;
    pResult->errorFactor = 2u * st.next; pResult->probes = st.probes; pResult->withinBudget = st.within; pResult->bytes = bytes;
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode_stream_budget(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                size_t maxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                limg_hip_budget_result *pResult)
  {
    if (!c || !pIn || !pStream || !pResult) return limg_hip_error_ArgumentNull;
    if (limg_hip_stream_bound(sizeX, sizeY) == 0) return limg_hip_error_InvalidParameter;
    uint32_t hLo, hHi;
    const limg_hip_result ok = budget_bounds(maxBytes, minErrorFactor, maxErrorFactor, pResult, hLo, hHi);
    if (ok != limg_hip_success) return ok;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    size_t bytes = 0;
    return encode_stream_host(c, pIn, sizeX, sizeY, pStream, capacity, &bytes, limg_hip_stream_bound(sizeX, sizeY), [&](const uint32_t *dIn, uint8_t *dStream, size_t bound, size_t *n) {
      const limg_hip_result r = limg_hip_encode_stream_budget_device(c, dIn, sizeX, sizeY, hasAlpha, dStream, bound, maxBytes, minErrorFactor, maxErrorFactor, poolThreads,
                                                                     fastBitCrushing, pResult, nullptr);
      if (r == limg_hip_success) *n = (size_t)pResult->bytes;
      return r;
    });
  }

  // ---- batched stream encode: a list of same-shape images, stream i = limg_hip_encode_stream_device of image i ----
  // Lists of whole-block images go chunk by chunk (the plane batch's rule) through ONE compact-mode batched encode -- records, shift words and the strips' payload
  // words in the context's raster arrays, image after image; the factor planes in per-image slices of stream.fac -- and one scan + one pack launch over the chunk.
  limg_hip_result limg_hip_encode_stream_batch_device(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                      uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, uint32_t errorFactor, int poolThreads,
                                                      int fastBitCrushing, void *stream)
  {
    if (!c || !ppIn || !ppStreams) return limg_hip_error_ArgumentNull;
    for (size_t i = 0; i < count; i++)
      if (!ppIn[i] || !ppStreams[i]) return limg_hip_error_ArgumentNull;
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (capacityEach < bound) return limg_hip_error_OutOfBounds;
    for (size_t i = 0; i < count; i++)
      if (((uintptr_t)ppStreams[i] & 15u) != 0) return limg_hip_error_InvalidParameter;
    if (count == 0) return limg_hip_success;
    if (count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t px = sizeX * sizeY, planeStride = (px + 255) & ~(size_t)255;
    const size_t blocksX = (sizeX + kBlock - 1) / kBlock, blocksY = (sizeY + kBlock - 1) / kBlock, blocks = blocksX * blocksY;
    const size_t stripsX = (blocksX + kStripBlocks - 1) / kStripBlocks, imageStrips = stripsX * blocksY;
    // the plane batch's chunk rule (limg_hip_encode3d_batch_device): 1 GiB of records, 32-bit strip ids, the test hook
    size_t chunk = (size_t)(1ull << 30) / (blocks * sizeof(limg_hip_block_record));
    if (chunk * imageStrips > 0x7FFFFFFFull) chunk = 0x7FFFFFFFull / imageStrips;
    if (chunk < 1) chunk = 1;
    if (TOPT(c, batch_chunk) > 0) chunk = (size_t)TOPT(c, batch_chunk);
    const bool ragged = (sizeX % kBlock) != 0 || (sizeY % kBlock) != 0;
    const bool oneByOne = count == 1 || ragged || c->opt.legacy_float_stage != 0 || c->opt.force_split_kernels != 0;
    const size_t most = oneByOne ? 1 : (count < chunk ? count : chunk); // images of the largest chunk
    limg_hip_result r;
    if ((r = c->stream.table.ensure(count * sizeof(StreamImage))) != limg_hip_success) return r;
    if (most > 1)
    { // everything a chunk needs, before the first launch: nothing is grown (and so freed) between the chunks of a list
      if ((r = c->stream.fac.ensure(most * planeStride * 3)) != limg_hip_success) return r;
      if ((r = c->stream.units.ensure(most * imageStrips * 4)) != limg_hip_success) return r;
      if ((r = c->enc.records.ensure(most * blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
      if ((r = c->enc.shifts.ensure(most * blocks * 4)) != limg_hip_success) return r;
    }
    std::vector<StreamImage> images(count);
    for (size_t i = 0; i < count; i++) images[i].stream = ppStreams[i];
    std::vector<ImageIO> table;
    r = limg_hip_success;
    for (size_t i0 = 0; i0 < count && r == limg_hip_success;)
    {
      const size_t n = oneByOne ? 1 : (count - i0 < chunk ? count - i0 : chunk);
      c->stats.accumulate = i0 != 0; // limg_hip_last_stats: all images of the list together, as the plane batch
      if (n == 1)
      { // the single call (images with partial edge blocks, the split path, the float stage inside the encode kernel, a list or a last chunk of one image)
        r = limg_hip_encode_stream_device(c, ppIn[i0], sizeX, sizeY, hasAlpha, ppStreams[i0], capacityEach, nullptr, errorFactor, poolThreads, fastBitCrushing, stream);
        if (r == limg_hip_success && pBytes && !oneByOne) launch_set_stream_table((StreamImage *)c->stream.table.p + i0, &images[i0], 1, s); // (for the sizes below)
      }
      else
      {
        table.assign(n, ImageIO{});
        for (size_t i = 0; i < n; i++)
        {
          uint8_t *fac = (uint8_t *)c->stream.fac.p + i * 3 * planeStride; // 256-byte aligned slices
          table[i].in = ppIn[i0 + i];
          table[i].info.pFactorsA = fac; table[i].info.pFactorsB = fac + planeStride; table[i].info.pFactorsC = fac + 2 * planeStride;
          images[i0 + i].fac[0] = fac; images[i0 + i].fac[1] = fac + planeStride; images[i0 + i].fac[2] = fac + 2 * planeStride;
        }
        limg_hip_compact_out comp = { (limg_hip_block_record *)c->enc.records.p, (uint32_t *)c->enc.shifts.p };
        EncodeExtra x;
        x.batch = table.data(); x.batchCount = n;
        x.streamRaw = true; x.stripWords = (uint32_t *)c->stream.units.p;
        if ((r = encode_device(c, ppIn[i0], sizeX, sizeY, hasAlpha, &table[0].info, &comp, errorFactor, poolThreads, fastBitCrushing, s, x)) != limg_hip_success) break;
        launch_set_stream_table((StreamImage *)c->stream.table.p + i0, &images[i0], n, s);
        StreamBatchParams b;
        memset(&b, 0, sizeof(b));
        b.sizeX = (uint32_t)sizeX; b.sizeY = (uint32_t)sizeY; b.blocksX = (uint32_t)blocksX; b.blocksY = (uint32_t)blocksY; b.nBlocks = (uint32_t)blocks;
        b.channels = hasAlpha ? 4 : 3; b.errorFactor = errorFactor; b.flags = (fastBitCrushing ? 1u : 0u) | (c->opt.dither_pcg ? 2u : 0u);
        b.stripsX = (uint32_t)stripsX; b.imageStrips = (uint32_t)imageStrips; b.nImages = (uint32_t)n; b.nStrips = (uint32_t)(n * imageStrips);
        const size_t slots = (size_t)device_cus(c) * 16; // as the single call: 16 one-wave workgroups per CU -- for the whole chunk
        b.nWaves = (uint32_t)(n * imageStrips < slots ? n * imageStrips : slots);
        b.images = (const StreamImage *)c->stream.table.p + i0;
        b.records = comp.pRecords; b.shifts = comp.pShifts; b.stripWords = (uint32_t *)c->stream.units.p;
        mark(c, s);
        launch_stream_pack_batch(b, s);
        mark(c, s); mark(c, s); mark(c, s);
        const hipError_t launched = hipGetLastError();
        if (launched != hipSuccess) { c->stats.accumulate = false; HIP_TRY(launched); }
      }
      i0 += n;
    }
    c->stats.accumulate = false;
    if (r != limg_hip_success || !pBytes) return r;
    // the sizes: gathered from the headers on the device, ONE download
    if ((r = c->stream.sizes.ensure(count * 8)) != limg_hip_success) return r;
    if (oneByOne) launch_set_stream_table((StreamImage *)c->stream.table.p, images.data(), count, s);
    launch_stream_gather_bytes((const StreamImage *)c->stream.table.p, count, (unsigned long long *)c->stream.sizes.p, s);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> sizes(count);
    HIP_TRY(hipMemcpyAsync(sizes.data(), c->stream.sizes.p, count * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < count; i++) pBytes[i] = (size_t)sizes[i];
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode_stream_batch(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                               uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, uint32_t errorFactor, int poolThreads, int fastBitCrushing)
  {
    if (!c || !ppIn || !ppStreams || !pBytes) return limg_hip_error_ArgumentNull;
    for (size_t i = 0; i < count; i++)
      if (!ppIn[i] || !ppStreams[i]) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (capacityEach < bound) return limg_hip_error_OutOfBounds;
    if (count == 0) return limg_hip_success;
    HIP_TRY(hipSetDevice(c->device));
    // staging: the images side by side in host.in, the streams at worst-case size (rounded up to 256 bytes) side by side in stream.buf
    const size_t px = sizeX * sizeY, slice = (bound + 255) & ~(size_t)255;
    limg_hip_result r;
    if ((r = c->host.in.ensure(count * px * 4)) != limg_hip_success) return r;
    if ((r = c->stream.buf.ensure(count * slice)) != limg_hip_success) return r;
    std::vector<const uint32_t *> dIn(count);
    std::vector<uint8_t *> dStreams(count);
    for (size_t i = 0; i < count; i++)
    {
      dIn[i] = (const uint32_t *)c->host.in.p + i * px;
      dStreams[i] = (uint8_t *)c->stream.buf.p + i * slice;
      HIP_TRY(hipMemcpy((void *)dIn[i], ppIn[i], px * 4, hipMemcpyHostToDevice));
    }
    if ((r = limg_hip_encode_stream_batch_device(c, count, dIn.data(), sizeX, sizeY, hasAlpha, dStreams.data(), slice, pBytes, errorFactor, poolThreads, fastBitCrushing,
                                                 nullptr)) != limg_hip_success)
      return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    for (size_t i = 0; i < count; i++) HIP_TRY(hipMemcpy(ppStreams[i], dStreams[i], pBytes[i], hipMemcpyDeviceToHost)); // totalBytes of each, not the capacity
    return limg_hip_success;
  }

  // ---- budgeted stream encode of a list: result i = limg_hip_encode_stream_budget_device of image i with pMaxBytes[i] (contract: include/limg_hip.h) ----
  // Chunk by chunk (the plane batch's rule): the records of the chunk from ONE k_fit_tpb grid, one search state and one counter per image, the whole chunk's searches
  // as 1 + 2 x rate_max_probes launches and ONE wait; then one stream encode per distinct error factor the searches chose.
  limg_hip_result limg_hip_encode_stream_budget_batch_device(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                             uint8_t *const *ppStreams, size_t capacityEach, const size_t *pMaxBytes, uint32_t minErrorFactor,
                                                             uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing, limg_hip_budget_result *pResults, void *stream)
  {
    if (!c || !ppIn || !ppStreams || !pMaxBytes || !pResults) return limg_hip_error_ArgumentNull;
    for (size_t i = 0; i < count; i++)
      if (!ppIn[i] || !ppStreams[i]) return limg_hip_error_ArgumentNull;
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (capacityEach < bound) return limg_hip_error_OutOfBounds;
    for (size_t i = 0; i < count; i++)
      if (((uintptr_t)ppStreams[i] & 15u) != 0) return limg_hip_error_InvalidParameter;
    uint32_t hLo, hHi;
    limg_hip_result r;
    if ((r = budget_list_checks(count, pMaxBytes, minErrorFactor, maxErrorFactor, pResults, hLo, hHi)) != limg_hip_success) return r;
    if (count == 0) return limg_hip_success;
    if (count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    auto single = [&](size_t i) {
      return limg_hip_encode_stream_budget_device(c, ppIn[i], sizeX, sizeY, hasAlpha, ppStreams[i], capacityEach, pMaxBytes[i], minErrorFactor, maxErrorFactor, poolThreads,
                                                  fastBitCrushing, &pResults[i], stream);
    };
    if (count == 1 || !rate_probe_applies(c, sizeX, sizeY, fastBitCrushing))
    { // no probe kernel (or nothing to share): the loop of single calls
      for (size_t i = 0; i < count; i++)
        if ((r = single(i)) != limg_hip_success) return r;
      return limg_hip_success;
    }
    const size_t blocksX = sizeX / kBlock, blocksY = sizeY / kBlock, blocks = blocksX * blocksY;
    const size_t stripsX = (blocksX + kStripBlocks - 1) / kStripBlocks, imageStrips = stripsX * blocksY;
    // the plane batch's chunk rule (limg_hip_encode3d_batch_device): 1 GiB of records, 32-bit strip ids, the test hook
    size_t chunk = (size_t)(1ull << 30) / (blocks * sizeof(limg_hip_block_record));
    if (chunk * imageStrips > 0x7FFFFFFFull) chunk = 0x7FFFFFFFull / imageStrips;
    if (chunk < 1) chunk = 1;
    if (TOPT(c, batch_chunk) > 0) chunk = (size_t)TOPT(c, batch_chunk);
    const size_t most = count < chunk ? count : chunk;
    if (most > 1)
    {
      if ((r = c->stream.rateState.ensure(most * sizeof(RateDevice))) != limg_hip_success) return r;
      if ((r = c->stream.rateCounter.ensure(most * 8)) != limg_hip_success) return r;
    }
    const uint32_t probes = rate_max_probes(hLo, hHi);
    std::vector<ImageIO> table;
    std::vector<uint64_t> budgets;
    std::vector<RateDevice> states;
    std::vector<uint32_t> order; // the chunk's images sorted by the h their searches chose
    std::vector<const uint32_t *> groupIn;
    std::vector<uint8_t *> groupOut;
    for (size_t i0 = 0; i0 < count;)
    {
      const size_t n = count - i0 < chunk ? count - i0 : chunk;
      if (n == 1)
      { // a chunk (or a last chunk) of one image
        if ((r = single(i0)) != limg_hip_success) return r;
        i0++;
        continue;
      }
      // 1. the chunk's records in the context's float mode, image after image in enc.records: k_fit_tpb's one grid; encode_params puts the image table on the device
      table.assign(n, ImageIO{});
      budgets.resize(n);
      bool vecIn = sizeX % 4 == 0;
      for (size_t i = 0; i < n; i++)
      {
        table[i].in = ppIn[i0 + i];
        budgets[i] = (uint64_t)pMaxBytes[i0 + i];
        vecIn = vecIn && (((uintptr_t)ppIn[i0 + i]) & 15u) == 0; // as encode_params: 16-byte loads only if every image of the chunk allows them
      }
      EncodeExtra x;
      x.fitOnly = true; x.fitFloatMode = true;
      x.batch = table.data(); x.batchCount = n;
      if ((r = encode_device(c, ppIn[i0], sizeX, sizeY, hasAlpha, nullptr, nullptr, 0, poolThreads, 1, s, x)) != limg_hip_success) return r;
      // 2. the searches: begin, then every launch any of them can need; probes of an image whose search is over return at once
      RateProbeBatchParams bp;
      memset(&bp, 0, sizeof(bp));
      bp.batch = (const ImageIO *)c->enc.batchTable.p;
      bp.nImages = (uint32_t)n; bp.imageStrips = (uint32_t)imageStrips;
      bp.sizeX = (uint32_t)sizeX; bp.sizeY = (uint32_t)sizeY; bp.blocksX = (uint32_t)blocksX; bp.blocksY = (uint32_t)blocksY; bp.stripsX = (uint32_t)stripsX;
      bp.vecIn = vecIn ? 1 : 0;
      bp.recordLimit = TOPT(c, record_limit) > 0 ? TOPT(c, record_limit) - 1 : 2700;
      const bool forced = c->opt.forced_shift[0] >= 0 && c->opt.forced_shift[0] <= 8 && c->opt.forced_shift[1] >= 0 && c->opt.forced_shift[1] <= 8 &&
                          c->opt.forced_shift[2] >= 0 && c->opt.forced_shift[2] <= 8;
      for (int i = 0; i < 3; i++) bp.forced[i] = forced ? c->opt.forced_shift[i] : -1;
      bp.records = (const limg_hip_block_record *)c->enc.records.p; bp.invN = (const float *)c->enc.invN.p;
      RateDevice *const dStates = (RateDevice *)c->stream.rateState.p;
      unsigned long long *const dCounters = (unsigned long long *)c->stream.rateCounter.p;
      bp.states = dStates; bp.counters = dCounters;
      launch_rate_begin_batch(dStates, dCounters, budgets.data(), n, hLo, hHi, s);
      for (uint32_t i = 0; i < probes; i++)
      {
        launch_rate_probe_batch(bp, hasAlpha ? 4 : 3, c->opt.float_mode == 1, s);
        launch_rate_step_batch(dStates, dCounters, (uint32_t)n, stream_fixed_bytes(sizeX, sizeY), s);
      }
      HIP_TRY(hipGetLastError());
      states.resize(n);
      HIP_TRY(hipMemcpyAsync(states.data(), dStates, n * sizeof(RateDevice), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (size_t i = 0; i < n; i++)
        if (!states[i].search.done) return limg_hip_error_Generic;
      // 3. the final encodes: the thresholds are kernel arguments of the persistent kernel, so one (batched) stream encode per distinct h
      order.resize(n);
      for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return states[a].search.next < states[b].search.next; });
      for (size_t g0 = 0; g0 < n;)
      {
        const uint32_t h = states[order[g0]].search.next;
        size_t g1 = g0;
        groupIn.clear(); groupOut.clear();
        for (; g1 < n && states[order[g1]].search.next == h; g1++) { groupIn.push_back(ppIn[i0 + order[g1]]); groupOut.push_back(ppStreams[i0 + order[g1]]); }
        if (g1 - g0 == 1) r = limg_hip_encode_stream_device(c, groupIn[0], sizeX, sizeY, hasAlpha, groupOut[0], capacityEach, nullptr, 2u * h, poolThreads, fastBitCrushing, stream);
        else r = limg_hip_encode_stream_batch_device(c, g1 - g0, groupIn.data(), sizeX, sizeY, hasAlpha, groupOut.data(), capacityEach, nullptr, 2u * h, poolThreads,
                                                     fastBitCrushing, stream);
        if (r != limg_hip_success) return r;
        g0 = g1;
      }
      for (size_t i = 0; i < n; i++)
      { // bytes: what the probe measured at the result -- the packer's totalBytes
        const RateState &st = states[i].search;
        limg_hip_budget_result &res = pResults[i0 + i];
        res.errorFactor = 2u * st.next; res.probes = st.probes; res.withinBudget = st.within; res.bytes = st.bestBytes;
      }
      i0 += n;
    }
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode_stream_budget_batch(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                      uint8_t *const *ppStreams, size_t capacityEach, const size_t *pMaxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor,
                                                      int poolThreads, int fastBitCrushing, limg_hip_budget_result *pResults)
  {
    if (!c || !ppIn || !ppStreams || !pMaxBytes || !pResults) return limg_hip_error_ArgumentNull;
    for (size_t i = 0; i < count; i++)
      if (!ppIn[i] || !ppStreams[i]) return limg_hip_error_ArgumentNull;
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    uint32_t hLo, hHi;
    limg_hip_result r;
    if ((r = budget_list_checks(count, pMaxBytes, minErrorFactor, maxErrorFactor, pResults, hLo, hHi)) != limg_hip_success) return r;
    if (count == 0) return limg_hip_success;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    HIP_TRY(hipSetDevice(c->device));
    // staging as limg_hip_encode_stream_batch: the images side by side in host.in, the streams at worst-case size side by side in stream.buf
    const size_t px = sizeX * sizeY, slice = (bound + 255) & ~(size_t)255;
    if ((r = c->host.in.ensure(count * px * 4)) != limg_hip_success) return r;
    if ((r = c->stream.buf.ensure(count * slice)) != limg_hip_success) return r;
    std::vector<const uint32_t *> dIn(count);
    std::vector<uint8_t *> dStreams(count);
    for (size_t i = 0; i < count; i++)
    {
      dIn[i] = (const uint32_t *)c->host.in.p + i * px;
      dStreams[i] = (uint8_t *)c->stream.buf.p + i * slice;
      HIP_TRY(hipMemcpy((void *)dIn[i], ppIn[i], px * 4, hipMemcpyHostToDevice));
    }
    std::vector<limg_hip_budget_result> results(count);
    for (size_t i = 0; i < count; i++) { memset(&results[i], 0, sizeof(results[i])); results[i].struct_size = sizeof(limg_hip_budget_result); }
    if ((r = limg_hip_encode_stream_budget_batch_device(c, count, dIn.data(), sizeX, sizeY, hasAlpha, dStreams.data(), slice, pMaxBytes, minErrorFactor, maxErrorFactor,
                                                        poolThreads, fastBitCrushing, results.data(), nullptr)) != limg_hip_success)
      return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    bool fits = true;
    for (size_t i = 0; i < count; i++)
    { // (the caller's struct_size may be larger than ours: only the members are written)
      pResults[i].errorFactor = results[i].errorFactor; pResults[i].probes = results[i].probes; pResults[i].withinBudget = results[i].withinBudget; pResults[i].bytes = results[i].bytes;
      fits = fits && results[i].bytes <= capacityEach;
    }
    if (!fits) return limg_hip_error_OutOfBounds; // the single host call's rule: the results say what each stream takes, no stream is written
    for (size_t i = 0; i < count; i++) HIP_TRY(hipMemcpy(ppStreams[i], dStreams[i], (size_t)results[i].bytes, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  // ---- version 2: the merged-block encoder's rectangles ----
  size_t limg_hip_blocked_stream_bound(size_t sizeX, size_t sizeY)
  {
    if (limg_hip_stream_bound(sizeX, sizeY) == 0) return 0;
    const size_t blocksX = (sizeX + kBlock - 1) / kBlock, blocksY = (sizeY + kBlock - 1) / kBlock;
    if (blocksX > 65535 || blocksY > 65535) return 0; // ox, oy, rx, ry are 16 bits
    return sizeof(limg_hip_stream_header) + blocksX * blocksY * sizeof(limg_hip_stream_rect) + blocksX * blocksY * 192;
  }

  limg_hip_result limg_hip_blocked_encode_stream_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                        size_t *pBytes, uint32_t errorFactor, int fastBitCrushing, void *stream)
  {
    if (!c || !pIn || !pStream) return limg_hip_error_ArgumentNull;
    const size_t bound = limg_hip_blocked_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (capacity < bound) return limg_hip_error_OutOfBounds;
    if (((uintptr_t)pStream & 15u) != 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = ensure_pack_resources(c, sizeX, sizeY)) != limg_hip_success) return r; // (before the encode: the context-memory figure does not depend on the content)
    // the whole pipeline up to the store step; when it returns the rectangles' records, shift words, factor and noise bytes are complete in the context
    if ((r = blocked_encode_device(c, pIn, sizeX, sizeY, hasAlpha, nullptr, errorFactor, fastBitCrushing, (hipStream_t)stream)) != limg_hip_success) return r;
    return pack_last(c, pStream, pBytes, (hipStream_t)stream);
  }

  limg_hip_result limg_hip_blocked_last_stream(limg_hip_context *c, uint8_t *pStream, size_t capacity, size_t *pBytes)
  {
    if (!c || !pStream || !pBytes) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (!c->blocked.last.valid) return limg_hip_error_InvalidParameter; // no merged-block encode on this context, or the last one failed
    const size_t bound = limg_hip_blocked_stream_bound(c->blocked.last.sizeX, c->blocked.last.sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = ensure_pack_resources(c, c->blocked.last.sizeX, c->blocked.last.sizeY)) != limg_hip_success) return r;
    if ((r = c->stream.buf.ensure(bound)) != limg_hip_success) return r;
    size_t bytes = 0;
    if ((r = pack_last(c, (uint8_t *)c->stream.buf.p, &bytes, nullptr)) != limg_hip_success) return r;
    return download_stream(c, bytes, pStream, capacity, pBytes);
  }

  limg_hip_result limg_hip_blocked_decode_stream_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t sizeX, size_t sizeY, void *stream)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    if (limg_hip_blocked_stream_bound(sizeX, sizeY) == 0 || streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_InvalidParameter;
    if (((uintptr_t)pStream & 15u) != 0 || ((uintptr_t)pOut & 15u) != 0) return limg_hip_error_InvalidParameter;
    // the whole image as a window: (0, 0, sizeX, sizeY) at stride sizeX
    hipStream_t s = (hipStream_t)stream;
    WindowDecodeParams wp;
    const limg_hip_result r = window_params(c, pStream, streamBytes, sizeX, sizeY, limg_hip_blocked_stream_bound(sizeX, sizeY), 0, 0, sizeX, sizeY, pOut, sizeX, s, wp);
    if (r != limg_hip_success) return r;
    return blocked_window_decode(c, wp, s);
  }

  limg_hip_result limg_hip_blocked_stream_info(const uint8_t *pStream, size_t streamBytes, size_t *pSizeX, size_t *pSizeY, int *pHasAlpha, size_t *pTotalBytes, size_t *pRectangles)
  {
    limg_hip_stream_header h;
    const limg_hip_result r = read_header(pStream, streamBytes, LIMG_HIP_STREAM_VERSION_BLOCKED, h);
    if (r != limg_hip_success) return r;
    if (!(h.flags & LIMG_HIP_STREAM_FLAG_MERGED) || limg_hip_blocked_stream_bound(h.sizeX, h.sizeY) == 0) return limg_hip_error_InvalidParameter;
    const uint64_t rects = h.reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES]; // one entry per rectangle
    const limg_hip_result ok = check_header_table(h, rects, sizeof(limg_hip_stream_rect), pSizeX, pSizeY, pHasAlpha, pTotalBytes);
    if (ok == limg_hip_success && pRectangles) *pRectangles = (size_t)rects;
    return ok;
  }

  limg_hip_result limg_hip_blocked_encode_stream(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                 size_t *pBytes, uint32_t errorFactor, int fastBitCrushing)
  {
    if (!c || !pIn || !pStream || !pBytes) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    return encode_stream_host(c, pIn, sizeX, sizeY, pStream, capacity, pBytes, limg_hip_blocked_stream_bound(sizeX, sizeY), [&](const uint32_t *dIn, uint8_t *dStream, size_t bound, size_t *bytes) {
      return limg_hip_blocked_encode_stream_device(c, dIn, sizeX, sizeY, hasAlpha, dStream, bound, bytes, errorFactor, fastBitCrushing, nullptr);
    });
  }

  limg_hip_result limg_hip_blocked_decode_stream(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t outPixels)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    size_t sizeX = 0, sizeY = 0, total = 0;
    const limg_hip_result r = limg_hip_blocked_stream_info(pStream, streamBytes, &sizeX, &sizeY, nullptr, &total, nullptr);
    if (r != limg_hip_success) return r;
    return decode_stream_host(c, pStream, streamBytes, pOut, outPixels, sizeX, sizeY, total, [&](const uint8_t *dStream, size_t bytes, uint32_t *dOut, size_t w, size_t h) {
      return limg_hip_blocked_decode_stream_device(c, dStream, bytes, dOut, w, h, nullptr);
    });
  }
}
