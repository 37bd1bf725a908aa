// limg_hip_stream_api.hip -- the compact stream entries of the C ABI: encode (8x8 encode in compact mode + the packer of limg_hip_stream.hip), decode, header check,
// and their host-pointer forms.
#include "limg_hip_context.h"

using namespace limg_hip;

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
    if ((r = c->streamFac.ensure(planeStride * 3)) != limg_hip_success) return r;
    // strip form of the packer (images of whole blocks): the encode kernel leaves one payload-word count per work strip (limg_hip_stream.hip)
    const size_t stripsX = (blocksX + kStripBlocks - 1) / kStripBlocks, nStrips = stripsX * blocksY;
    const bool stripForm = (sizeX % kBlock) == 0 && (sizeY % kBlock) == 0 && !c->forceSplit;
    if ((r = c->streamTiles.ensure(tiles * 4)) != limg_hip_success) return r;
    if (stripForm && (r = c->streamUnits.ensure(nStrips * 4)) != limg_hip_success) return r;
    if ((r = c->records.ensure(blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
    if ((r = c->shifts.ensure(blocks * 4)) != limg_hip_success) return r;
    limg_hip_encode3d_info info;
    memset(&info, 0, sizeof(info));
    info.pFactorsA = (uint8_t *)c->streamFac.p; info.pFactorsB = info.pFactorsA + planeStride; info.pFactorsC = info.pFactorsB + planeStride;
    limg_hip_compact_out comp = { (limg_hip_block_record *)c->records.p, (uint32_t *)c->shifts.p };
    EncodeExtra xs;
    xs.streamRaw = true;
    xs.stripWords = stripForm ? (uint32_t *)c->streamUnits.p : nullptr;
    if ((r = encode_device(c, pIn, sizeX, sizeY, hasAlpha, &info, &comp, errorFactor, poolThreads, fastBitCrushing, s, xs)) != limg_hip_success) return r;

    StreamParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.sizeX = (uint32_t)sizeX; sp.sizeY = (uint32_t)sizeY; sp.blocksX = (uint32_t)blocksX; sp.blocksY = (uint32_t)blocksY;
    sp.nBlocks = (uint32_t)blocks; sp.nTiles = (uint32_t)tiles; sp.channels = hasAlpha ? 4 : 3; sp.errorFactor = errorFactor;
    sp.flags = (fastBitCrushing ? 1u : 0u) | (c->opt.dither_pcg ? 2u : 0u);
    sp.fac[0] = info.pFactorsA; sp.fac[1] = info.pFactorsB; sp.fac[2] = info.pFactorsC;
    sp.records = comp.pRecords; sp.shifts = comp.pShifts;
    sp.stream = pStream; sp.tileBase = (uint32_t *)c->streamTiles.p;
    if (stripForm)
    {
      sp.stripWords = (uint32_t *)c->streamUnits.p;
      sp.stripsX = (uint32_t)stripsX; sp.nStrips = (uint32_t)nStrips;
      const size_t slots = (size_t)(c->persistentWorkgroups / 5) * 16; // 16 one-wave workgroups per CU (128 vector registers each: 4 per SIMD)
      sp.nWaves = (uint32_t)(nStrips < slots ? nStrips : slots);
    }
    mark(c, s);
    launch_stream_pack(sp, s);
    mark(c, s); mark(c, s); mark(c, s);
    HIP_TRY(hipGetLastError());
    if (pBytes)
    {
      limg_hip_stream_header h;
      HIP_TRY(hipMemcpyAsync(&h, pStream, sizeof(h), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      *pBytes = (size_t)h.totalBytes;
    }
    return limg_hip_success;
  }

  limg_hip_result limg_hip_decode_stream_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t sizeX, size_t sizeY, void *stream)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    if (limg_hip_stream_bound(sizeX, sizeY) == 0 || streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_InvalidParameter;
    if (((uintptr_t)pStream & 15u) != 0 || ((uintptr_t)pOut & 15u) != 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    limg_hip_result r;
    if (!c->streamStatus.p)
    {
      if ((r = c->streamStatus.ensure(256 + 2048)) != limg_hip_success) return r; // the status word, then the decode kernel's store sink (see DecodeParams::sink)
      HIP_TRY(hipMemsetAsync(c->streamStatus.p, 0, 8, s));
    }
    DecodeParams dp;
    memset(&dp, 0, sizeof(dp));
    dp.sizeX = (uint32_t)sizeX; dp.sizeY = (uint32_t)sizeY;
    dp.blocksX = (uint32_t)((sizeX + kBlock - 1) / kBlock); dp.blocksY = (uint32_t)((sizeY + kBlock - 1) / kBlock);
    dp.nBlocks = dp.blocksX * dp.blocksY;
    if (streamBytes < sizeof(limg_hip_stream_header) + (size_t)dp.nBlocks * sizeof(limg_hip_stream_block)) return limg_hip_error_OutOfBounds;
    dp.stream = pStream; dp.streamBytes = streamBytes; dp.out = pOut; dp.status = (uint32_t *)c->streamStatus.p; dp.sink = (uint32_t *)((uint8_t *)c->streamStatus.p + 256);
    mark(c, s);
    launch_stream_decode(dp, s);
    mark(c, s); mark(c, s); mark(c, s);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  limg_hip_result limg_hip_stream_info(const uint8_t *pStream, size_t streamBytes, size_t *pSizeX, size_t *pSizeY, int *pHasAlpha, size_t *pTotalBytes)
  {
    if (!pStream) return limg_hip_error_ArgumentNull;
    if (streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_OutOfBounds;
    limg_hip_stream_header h;
    memcpy(&h, pStream, sizeof(h));
    if (h.magic != LIMG_HIP_STREAM_MAGIC || h.version != LIMG_HIP_STREAM_VERSION || (h.channels != 3 && h.channels != 4)) return limg_hip_error_InvalidParameter;
    if (limg_hip_stream_bound(h.sizeX, h.sizeY) == 0) return limg_hip_error_InvalidParameter;
    const uint64_t bx = ((uint64_t)h.sizeX + kBlock - 1) / kBlock, by = ((uint64_t)h.sizeY + kBlock - 1) / kBlock;
    if (h.blocksX != bx || h.blocksY != by) return limg_hip_error_InvalidParameter;
    if (h.payloadWords > bx * by * 24 || h.totalBytes != sizeof(h) + bx * by * sizeof(limg_hip_stream_block) + h.payloadWords * 8) return limg_hip_error_InvalidParameter;
    if (pSizeX) *pSizeX = h.sizeX;
    if (pSizeY) *pSizeY = h.sizeY;
    if (pHasAlpha) *pHasAlpha = h.channels == 4;
    if (pTotalBytes) *pTotalBytes = (size_t)h.totalBytes;
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode_stream(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity, size_t *pBytes,
                                         uint32_t errorFactor, int poolThreads, int fastBitCrushing)
  {
    if (!c || !pIn || !pStream || !pBytes) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    const size_t px = sizeX * sizeY;
    if ((r = c->in.ensure(px * 4)) != limg_hip_success) return r;
    if ((r = c->streamBuf.ensure(bound)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->in.p, pIn, px * 4, hipMemcpyHostToDevice));
    size_t bytes = 0;
    if ((r = limg_hip_encode_stream_device(c, (const uint32_t *)c->in.p, sizeX, sizeY, hasAlpha, (uint8_t *)c->streamBuf.p, bound, &bytes, errorFactor, poolThreads,
                                           fastBitCrushing, nullptr)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    *pBytes = bytes;
    if (bytes > capacity) return limg_hip_error_OutOfBounds; // *pBytes tells the caller what it takes
    HIP_TRY(hipMemcpy(pStream, c->streamBuf.p, bytes, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_decode_stream(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t outPixels)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    size_t sizeX = 0, sizeY = 0, total = 0;
    limg_hip_result r;
    if ((r = limg_hip_stream_info(pStream, streamBytes, &sizeX, &sizeY, nullptr, &total)) != limg_hip_success) return r;
    if (total > streamBytes || sizeX * sizeY > outPixels) return limg_hip_error_OutOfBounds;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = c->streamBuf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->planes.ensure(sizeX * sizeY * 4)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->streamBuf.p, pStream, total, hipMemcpyHostToDevice));
    if ((r = limg_hip_decode_stream_device(c, (const uint8_t *)c->streamBuf.p, total, (uint32_t *)c->planes.p, sizeX, sizeY, nullptr)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(pOut, c->planes.p, sizeX * sizeY * 4, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }
}
