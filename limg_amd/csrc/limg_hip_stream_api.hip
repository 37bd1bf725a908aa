// limg_hip_stream_api.hip -- the compact stream entries of the C ABI but for version 1's encode family (limg_hip_stream_encode_api.hip) and the window entries
// (limg_hip_stream_window_api.hip): what every stream unit shares, both versions' header checks and whole-image decodes with their host-pointer forms, and version 2's
// encode -- the merged-block encoder in compact mode (blocked_encode_device without planes, limg_hip_blocked_api.hip) + the scan and pack kernels of
// limg_hip_blocked_stream.hip; its whole-image decode is a window decode.  Version 1's decode kernel: limg_hip_stream.hip.
#include "limg_hip_context.h"

using namespace limg_hip;

// ---- shared with the other stream units (declared in limg_hip_context.h) ----
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

limg_hip_result limg_hip::stream_total_bytes(const uint8_t *dStream, hipStream_t s, size_t *pBytes)
{
  limg_hip_stream_header h;
  HIP_TRY(hipMemcpyAsync(&h, dStream, sizeof(h), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *pBytes = (size_t)h.totalBytes;
  return limg_hip_success;
}

limg_hip_result limg_hip::download_stream(limg_hip_context *c, size_t bytes, uint8_t *pStream, size_t capacity, size_t *pBytes)
{
  *pBytes = bytes;
  if (bytes > capacity) return limg_hip_error_OutOfBounds;
  HIP_TRY(hipMemcpy(pStream, c->stream.buf.p, bytes, hipMemcpyDeviceToHost));
  return limg_hip_success;
}

namespace
{
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

  // ---- host-pointer decode: upload, the version's device entry on the null stream, status, download (the encode's counterpart: encode_stream_host) ----
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
    const EncodeShape sh(sizeX, sizeY);
    if (!sh.valid) return 0;
    const size_t blocks = sh.blocks;
    if (blocks * 24 > 0xFFFFFFFFull) return 0; // entry.payloadWord is 32 bits
    return sizeof(limg_hip_stream_header) + blocks * sizeof(limg_hip_stream_block) + blocks * 192;
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
    Timeline tl(c, s, 4);
    tl.mark();
    launch_stream_decode(dp, device_cus(c), s);
    tl.close();
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
