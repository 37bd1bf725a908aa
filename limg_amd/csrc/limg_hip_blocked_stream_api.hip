// limg_hip_blocked_stream_api.hip -- the version 2 stream entries of the C ABI: the merged-block encoder in compact mode (blocked_encode_device without planes,
// limg_hip_blocked_api.hip) followed by the scan + pack kernels of limg_hip_blocked_stream.hip; decode; header check; their host-pointer forms.
#include "limg_hip_context.h"

using namespace limg_hip;

namespace
{
  // the status word the stream decoders share (limg_hip_check_device_status reads it), as limg_hip_decode_stream_device sets it up
  limg_hip_result ensure_stream_status(limg_hip_context *c, hipStream_t s)
  {
    if (c->streamStatus.p) return limg_hip_success;
    const limg_hip_result r = c->streamStatus.ensure(256 + 2048);
    if (r != limg_hip_success) return r;
    HIP_TRY(hipMemsetAsync(c->streamStatus.p, 0, 8, s));
    return limg_hip_success;
  }

  // the packer's scratch for the worst case (every block its own rectangle): 4 bytes per block and 8 per 256 blocks; the two timing events
  limg_hip_result ensure_pack_resources(limg_hip_context *c, size_t sizeX, size_t sizeY)
  {
    const size_t blocks = ((sizeX + kBlock - 1) / kBlock) * ((sizeY + kBlock - 1) / kBlock);
    limg_hip_result r;
    if ((r = c->bsUnits.ensure((blocks + 1) * 4)) != limg_hip_success) return r;
    if ((r = c->bsTiles.ensure(((blocks + 255) / 256) * 8)) != limg_hip_success) return r;
    for (hipEvent_t e; c->packTimers.size() < 2; c->packTimers.push_back(e)) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDefault));
    return limg_hip_success;
  }

  // The stream of the context's last merged-block encode, from what that left in the context's buffers (blocked_encode_device: with or without planes, the store step
  // does not change them): scan + pack on `s`.  pBytes (host, may be NULL) makes the call wait.
  limg_hip_result pack_last(limg_hip_context *c, uint8_t *dStream, size_t *pBytes, hipStream_t s)
  {
    const size_t sizeX = c->lastBlocked.sizeX, sizeY = c->lastBlocked.sizeY;
    const size_t blocksX = (sizeX + kBlock - 1) / kBlock, blocksY = (sizeY + kBlock - 1) / kBlock, blocks = blocksX * blocksY, nRegions = c->lastRegions.size();
    if (!c->lastBlocked.valid || nRegions == 0 || nRegions > blocks) return limg_hip_error_Generic;
    BlockedStreamParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.sizeX = (uint32_t)sizeX; sp.sizeY = (uint32_t)sizeY; sp.blocksX = (uint32_t)blocksX; sp.blocksY = (uint32_t)blocksY;
    sp.channels = (uint32_t)c->lastBlocked.channels; sp.errorFactor = c->lastBlocked.errorFactor; sp.flags = c->lastBlocked.flags;
    sp.nRegions = (uint32_t)nRegions; sp.nTiles = (uint32_t)((nRegions + 255) / 256); sp.scratchCap = (uint32_t)c->blockedScratchCap;
    sp.regions = (const RegionDesc *)c->bRegions.p; sp.out = (const RegionOut *)c->bOut.p; sp.noiseBase = (const unsigned long long *)c->bNoiseBase.p;
    sp.scratchFac = (const uint8_t *)c->bFac.p; sp.noise = (const uint8_t *)c->bNoise.p;
    sp.stream = dStream; sp.units = (uint32_t *)c->bsUnits.p; sp.tiles = (uint32_t *)c->bsTiles.p;
    HIP_TRY(hipEventRecord(c->packTimers[0], s));
    launch_blocked_stream_pack(sp, s);
    HIP_TRY(hipEventRecord(c->packTimers[1], s));
    HIP_TRY(hipGetLastError());
    c->packTimed = true;
    if (pBytes)
    {
      limg_hip_stream_header h;
      HIP_TRY(hipMemcpyAsync(&h, dStream, sizeof(h), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      *pBytes = (size_t)h.totalBytes;
    }
    return limg_hip_success;
  }
}

extern "C"
{
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
    if (!c->lastBlocked.valid) return limg_hip_error_InvalidParameter; // no merged-block encode on this context, or the last one failed
    const size_t bound = limg_hip_blocked_stream_bound(c->lastBlocked.sizeX, c->lastBlocked.sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = ensure_pack_resources(c, c->lastBlocked.sizeX, c->lastBlocked.sizeY)) != limg_hip_success) return r;
    if ((r = c->streamBuf.ensure(bound)) != limg_hip_success) return r;
    size_t bytes = 0;
    if ((r = pack_last(c, (uint8_t *)c->streamBuf.p, &bytes, nullptr)) != limg_hip_success) return r;
    *pBytes = bytes;
    if (bytes > capacity) return limg_hip_error_OutOfBounds; // *pBytes tells the caller what it takes
    HIP_TRY(hipMemcpy(pStream, c->streamBuf.p, bytes, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_decode_stream_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t sizeX, size_t sizeY, void *stream)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    if (limg_hip_blocked_stream_bound(sizeX, sizeY) == 0 || streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_InvalidParameter;
    if (((uintptr_t)pStream & 15u) != 0 || ((uintptr_t)pOut & 15u) != 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    BlockedDecodeParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.sizeX = (uint32_t)sizeX; dp.sizeY = (uint32_t)sizeY;
    dp.blocksX = (uint32_t)((sizeX + kBlock - 1) / kBlock); dp.blocksY = (uint32_t)((sizeY + kBlock - 1) / kBlock);
    dp.nBlocks = dp.blocksX * dp.blocksY;
    limg_hip_result r;
    if ((r = ensure_stream_status(c, s)) != limg_hip_success) return r;
    if ((r = c->bsMap.ensure((size_t)dp.nBlocks * 4)) != limg_hip_success) return r;
    if ((r = c->bsState.ensure(64)) != limg_hip_success) return r;
    HIP_TRY(hipMemsetAsync(c->bsMap.p, 0xFF, (size_t)dp.nBlocks * 4, s)); // no block has a rectangle yet
    HIP_TRY(hipMemsetAsync(c->bsState.p, 0, 64, s));
    dp.stream = pStream; dp.streamBytes = streamBytes; dp.out = pOut;
    dp.map = (uint32_t *)c->bsMap.p; dp.status = (uint32_t *)c->streamStatus.p; dp.state = (uint32_t *)c->bsState.p;
    launch_blocked_stream_decode(dp, s);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_stream_info(const uint8_t *pStream, size_t streamBytes, size_t *pSizeX, size_t *pSizeY, int *pHasAlpha, size_t *pTotalBytes, size_t *pRectangles)
  {
    if (!pStream) return limg_hip_error_ArgumentNull;
    if (streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_OutOfBounds;
    limg_hip_stream_header h;
    memcpy(&h, pStream, sizeof(h));
    if (h.magic != LIMG_HIP_STREAM_MAGIC || h.version != LIMG_HIP_STREAM_VERSION_BLOCKED || (h.channels != 3 && h.channels != 4)) return limg_hip_error_InvalidParameter;
    if (!(h.flags & LIMG_HIP_STREAM_FLAG_MERGED) || limg_hip_blocked_stream_bound(h.sizeX, h.sizeY) == 0) return limg_hip_error_InvalidParameter;
    const uint64_t bx = ((uint64_t)h.sizeX + kBlock - 1) / kBlock, by = ((uint64_t)h.sizeY + kBlock - 1) / kBlock, rects = h.reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES];
    if (h.blocksX != bx || h.blocksY != by || rects == 0 || rects > bx * by) return limg_hip_error_InvalidParameter;
    if (h.payloadWords > bx * by * 24 || h.totalBytes != sizeof(h) + rects * sizeof(limg_hip_stream_rect) + h.payloadWords * 8) return limg_hip_error_InvalidParameter;
    if (pSizeX) *pSizeX = h.sizeX;
    if (pSizeY) *pSizeY = h.sizeY;
    if (pHasAlpha) *pHasAlpha = h.channels == 4;
    if (pTotalBytes) *pTotalBytes = (size_t)h.totalBytes;
    if (pRectangles) *pRectangles = (size_t)rects;
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_encode_stream(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                 size_t *pBytes, uint32_t errorFactor, int fastBitCrushing)
  {
    if (!c || !pIn || !pStream || !pBytes) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const size_t bound = limg_hip_blocked_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    const size_t px = sizeX * sizeY;
    if ((r = c->in.ensure(px * 4)) != limg_hip_success) return r;
    if ((r = c->streamBuf.ensure(bound)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->in.p, pIn, px * 4, hipMemcpyHostToDevice));
    size_t bytes = 0;
    if ((r = limg_hip_blocked_encode_stream_device(c, (const uint32_t *)c->in.p, sizeX, sizeY, hasAlpha, (uint8_t *)c->streamBuf.p, bound, &bytes, errorFactor, fastBitCrushing,
                                                   nullptr)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    *pBytes = bytes;
    if (bytes > capacity) return limg_hip_error_OutOfBounds; // *pBytes tells the caller what it takes
    HIP_TRY(hipMemcpy(pStream, c->streamBuf.p, bytes, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_decode_stream(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t outPixels)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    size_t sizeX = 0, sizeY = 0, total = 0, rects = 0;
    limg_hip_result r;
    if ((r = limg_hip_blocked_stream_info(pStream, streamBytes, &sizeX, &sizeY, nullptr, &total, &rects)) != limg_hip_success) return r;
    if (total > streamBytes || sizeX * sizeY > outPixels) return limg_hip_error_OutOfBounds;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = c->streamBuf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->planes.ensure(sizeX * sizeY * 4)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->streamBuf.p, pStream, total, hipMemcpyHostToDevice));
    if ((r = limg_hip_blocked_decode_stream_device(c, (const uint8_t *)c->streamBuf.p, total, (uint32_t *)c->planes.p, sizeX, sizeY, nullptr)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r; // a refused stream: nothing was decoded, pOut keeps what it held
    HIP_TRY(hipMemcpy(pOut, c->planes.p, sizeX * sizeY * 4, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }
}
