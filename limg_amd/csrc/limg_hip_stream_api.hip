// limg_hip_stream_api.hip -- the compact stream entries of the C ABI, both versions.  Version 1: 8x8 encode in compact mode + the packer of limg_hip_stream.hip.
// Version 2: the merged-block encoder in compact mode (blocked_encode_device without planes, limg_hip_blocked_api.hip) + the scan and pack kernels of
// limg_hip_blocked_stream.hip.  Decode, header check and the host-pointer forms of each; what the two versions do alike is written once, in the namespace below.
#include "limg_hip_context.h"

#include <algorithm>
#include <type_traits>
#include <vector>

using namespace limg_hip;

namespace
{
  int device_cus(const limg_hip_context *c) { return c->persistentWorkgroups / 5; }

  // the status word the stream decoders share (limg_hip_check_device_status reads it), then the version 1 decode kernel's store sink (see DecodeParams::sink)
  limg_hip_result ensure_stream_status(limg_hip_context *c, hipStream_t s)
  {
    if (c->streamStatus.p) return limg_hip_success;
    const limg_hip_result r = c->streamStatus.ensure(256 + 2048);
    if (r != limg_hip_success) return r;
    HIP_TRY(hipMemsetAsync(c->streamStatus.p, 0, 8, s));
    return limg_hip_success;
  }

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
  // the stream in the context's streamBuf to the caller: *pBytes says what it takes even where `capacity` is too small
  limg_hip_result download_stream(limg_hip_context *c, size_t bytes, uint8_t *pStream, size_t capacity, size_t *pBytes)
  {
    *pBytes = bytes;
    if (bytes > capacity) return limg_hip_error_OutOfBounds;
    HIP_TRY(hipMemcpy(pStream, c->streamBuf.p, bytes, hipMemcpyDeviceToHost));
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
    if ((r = c->in.ensure(px * 4)) != limg_hip_success) return r;
    if ((r = c->streamBuf.ensure(bound)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->in.p, pIn, px * 4, hipMemcpyHostToDevice));
    size_t bytes = 0;
    if ((r = deviceEncode((const uint32_t *)c->in.p, (uint8_t *)c->streamBuf.p, bound, &bytes)) != limg_hip_success) return r;
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
    if ((r = c->streamBuf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->planes.ensure(sizeX * sizeY * 4)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->streamBuf.p, pStream, total, hipMemcpyHostToDevice));
    if ((r = deviceDecode((const uint8_t *)c->streamBuf.p, total, (uint32_t *)c->planes.p, sizeX, sizeY)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(pOut, c->planes.p, sizeX * sizeY * 4, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  // ---- version 2 ----
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
    launch_blocked_stream_pack(sp, device_cus(c), s);
    HIP_TRY(hipEventRecord(c->packTimers[1], s));
    HIP_TRY(hipGetLastError());
    c->packTimed = true;
    return pBytes ? stream_total_bytes(dStream, s, pBytes) : limg_hip_success;
  }

  // ---- window decode: limg_hip_*decode_stream_window* (kernels: limg_hip_stream_window.hip) ----
  // Where a window's pixels go: packed RGBA8 (planes == 0: elemBytes 4, one element per pixel) or `planes` planes of float / _Float16 (the tensor entries).
  struct WindowOut
  {
    void *p;
    size_t rowStride, planeStride; // in elements
    uint32_t elemBytes, planes;
  };
  WindowOut window_out(const limg_hip_window &w, const limg_hip_tensor_format *) { return { w.pOut, w.outStridePixels, 0, 4u, 0u }; }
  WindowOut window_out(const limg_hip_tensor_window &w, const limg_hip_tensor_format *f)
  {
    return { w.pOut, w.rowStride, w.planeStride, f->type == LIMG_HIP_TENSOR_F16 ? 2u : 4u, f->planes };
  }
  WindowOut window_out(const limg_hip_scaled_window &w, const limg_hip_tensor_format *) { return { w.pOut, w.outStridePixels, 0, 4u, 0u }; }
  WindowOut window_out(const limg_hip_scaled_tensor_window &w, const limg_hip_tensor_format *f)
  {
    return { w.pOut, w.rowStride, w.planeStride, f->type == LIMG_HIP_TENSOR_F16 ? 2u : 4u, f->planes };
  }
  // the four window types: which go to planes, which carry a level (the others are level 0)
  template <class WIN> struct WindowKind { static constexpr bool tensor = false, scaled = false; };
  template <> struct WindowKind<limg_hip_tensor_window> { static constexpr bool tensor = true, scaled = false; };
  template <> struct WindowKind<limg_hip_scaled_window> { static constexpr bool tensor = false, scaled = true; };
  template <> struct WindowKind<limg_hip_scaled_tensor_window> { static constexpr bool tensor = true, scaled = true; };
  template <class WIN> size_t window_level(const WIN &w)
  {
    if constexpr (WindowKind<WIN>::scaled) return w.log2Scale;
    else return 0;
  }
  bool tensor_format_ok(const limg_hip_tensor_format *f) { return (f->type == LIMG_HIP_TENSOR_F32 || f->type == LIMG_HIP_TENSOR_F16) && (f->planes == 3u || f->planes == 4u); }

  // the window's size and the output's strides: what every window entry, device or host, checks first
  limg_hip_result window_out_check(size_t width, size_t height, const WindowOut &o)
  {
    if (width == 0 || height == 0 || o.rowStride < width) return limg_hip_error_InvalidParameter;
    if (o.planes)
    { // planeStride >= (height - 1) * rowStride + width, without overflow
      if (height > 1 && o.rowStride > ((size_t)-1 - width) / (height - 1)) return limg_hip_error_InvalidParameter;
      if (o.planeStride < (height - 1) * o.rowStride + width) return limg_hip_error_InvalidParameter;
    }
    return limg_hip_success;
  }
  bool out_aligned(const WindowOut &o) { return ((uintptr_t)o.p & (o.elemBytes - 1u)) == 0; }
  bool window_inside(size_t sizeX, size_t sizeY, size_t x0, size_t y0, size_t width, size_t height)
  {
    return !(x0 >= sizeX || width > sizeX - x0 || y0 >= sizeY || height > sizeY - y0);
  }

  // the checks and the parameters the two versions share, without touching the device; `bound`: the version's limg_hip_*stream_bound(sizeX, sizeY).  status, map and
  // state are the caller's to set.  level: the scaled entries' log2Scale -- the window is then in level coordinates, inside (sizeX >> level) x (sizeY >> level), and wp
  // gets its source footprint (x0 .. height times 1 << level: inside the image, so nothing overflows) with vecOut stated on the window itself.
  limg_hip_result window_fill(const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t bound, size_t x0, size_t y0, size_t width, size_t height,
                              const WindowOut &o, WindowDecodeParams &wp, size_t level = 0)
  {
    if (level > 3 || window_out_check(width, height, o) != limg_hip_success || bound == 0 || streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_InvalidParameter;
    if (((uintptr_t)pStream & 15u) != 0 || !out_aligned(o)) return limg_hip_error_InvalidParameter;
    if (!window_inside(sizeX >> level, sizeY >> level, x0, y0, width, height)) return limg_hip_error_OutOfBounds;
    const size_t outX0 = x0;
    x0 <<= level; y0 <<= level; width <<= level; height <<= level;
    memset(&wp, 0, sizeof(wp));
    wp.sizeX = (uint32_t)sizeX; wp.sizeY = (uint32_t)sizeY;
    wp.blocksX = (uint32_t)((sizeX + kBlock - 1) / kBlock); wp.blocksY = (uint32_t)((sizeY + kBlock - 1) / kBlock);
    wp.nBlocks = wp.blocksX * wp.blocksY;
    wp.stream = pStream; wp.streamBytes = streamBytes;
    wp.x0 = (uint32_t)x0; wp.y0 = (uint32_t)y0; wp.width = (uint32_t)width; wp.height = (uint32_t)height;
    wp.bx0 = (uint32_t)(x0 / kBlock); wp.by0 = (uint32_t)(y0 / kBlock);
    wp.wbx = (uint32_t)((x0 + width - 1) / kBlock) - wp.bx0 + 1; wp.wby = (uint32_t)((y0 + height - 1) / kBlock) - wp.by0 + 1;
    wp.out = (uint32_t *)o.p; wp.outStride = o.rowStride; wp.planeStride = o.planeStride;
    const size_t per = 16u / o.elemBytes; // elements per 16-byte store (planeStride is 0 for RGBA)
    wp.vecOut = ((uintptr_t)o.p & 15u) == 0 && o.rowStride % per == 0 && o.planeStride % per == 0 && outX0 % per == 0;
    wp.log2Scale = (uint32_t)level;
    return limg_hip_success;
  }

  limg_hip_result window_params(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t bound, size_t x0, size_t y0, size_t width,
                                size_t height, uint32_t *pOut, size_t outStridePixels, hipStream_t s, WindowDecodeParams &wp)
  {
    limg_hip_result r = window_fill(pStream, streamBytes, sizeX, sizeY, bound, x0, y0, width, height, WindowOut{ pOut, outStridePixels, 0, 4u, 0u }, wp);
    if (r != limg_hip_success) return r;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = ensure_stream_status(c, s)) != limg_hip_success) return r;
    wp.status = (uint32_t *)c->streamStatus.p;
    return limg_hip_success;
  }

  // Version 2's one decode, the full image's and a window's: wp from window_params; the map of the window's blocks (not the image's) and the call's state words, then
  // the two kernels
  limg_hip_result blocked_window_decode(limg_hip_context *c, WindowDecodeParams &wp, hipStream_t s)
  {
    const size_t mapBytes = (size_t)wp.wbx * wp.wby * 4;
    limg_hip_result r;
    if ((r = c->bsMap.ensure(mapBytes)) != limg_hip_success) return r;
    if ((r = c->bsState.ensure(64)) != limg_hip_success) return r;
    HIP_TRY(hipMemsetAsync(c->bsMap.p, 0xFF, mapBytes, s)); // no block has a rectangle yet
    HIP_TRY(hipMemsetAsync(c->bsState.p, 0, 64, s));
    wp.map = (uint32_t *)c->bsMap.p; wp.state = (uint32_t *)c->bsState.p;
    launch_blocked_stream_window_decode(wp, device_cus(c), s);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  // info(&sizeX, &sizeY, &total): the version's header check.  deviceDecode(dStream, total, sizeX, sizeY, dOut): into context staging at stride `width`; only a stream
  // that passed reaches pOut
  template <class INFO, class DECODE>
  limg_hip_result decode_window_host(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height, uint32_t *pOut,
                                     size_t outStridePixels, INFO &&info, DECODE &&deviceDecode)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (width == 0 || height == 0 || outStridePixels < width) return limg_hip_error_InvalidParameter;
    size_t sizeX = 0, sizeY = 0, total = 0;
    limg_hip_result r = info(&sizeX, &sizeY, &total);
    if (r != limg_hip_success) return r;
    if (total > streamBytes) return limg_hip_error_OutOfBounds;
    if (x0 >= sizeX || width > sizeX - x0 || y0 >= sizeY || height > sizeY - y0) return limg_hip_error_OutOfBounds;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = c->streamBuf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->planes.ensure(width * height * 4)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->streamBuf.p, pStream, total, hipMemcpyHostToDevice));
    if ((r = deviceDecode((const uint8_t *)c->streamBuf.p, total, sizeX, sizeY, (uint32_t *)c->planes.p)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy2D(pOut, outStridePixels * 4, c->planes.p, width * 4, width * 4, height, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  // ---- batched window decode: limg_hip_*decode_stream_windows* (kernels: limg_hip_stream_window.hip) ----
  size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

  // One call: every job checked on the host before anything touches the device, then the job table built in a pinned slot of the context's ring, copied on `s`,
  // and the version's one (two) launches.  blocked: version 2.  JOB: limg_hip_window_job (packed RGBA8; pFormat is not looked at) or limg_hip_tensor_window_job
  // (planes of pFormat's type): the same checks, table and launches but for where the pixels go; their _scaled_ twins: the same again with the job's level handed to
  // window_fill and the scaled kernels launched.
  template <class JOB>
  limg_hip_result decode_windows_device(limg_hip_context *c, const JOB *pJobs, size_t count, const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, hipStream_t s,
                                        bool blocked)
  {
    typedef decltype(JOB::window) WIN;
    constexpr bool tensor = WindowKind<WIN>::tensor, scaled = WindowKind<WIN>::scaled;
    if (!c || !pJobs || (tensor && !pFormat)) return limg_hip_error_ArgumentNull;
    if (count == 0 || count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    if (tensor && !tensor_format_ok(pFormat)) return limg_hip_error_InvalidParameter;
    // pass 1: the single-window entry's checks, job by job in its order; the sums the table's layout needs
    unsigned long long units = 0, blocks = 0;
    WindowDecodeParams wp;
    for (size_t i = 0; i < count; i++)
    {
      const JOB &j = pJobs[i];
      if (!j.pStream || !j.window.pOut) return limg_hip_error_ArgumentNull;
      const size_t bound = blocked ? limg_hip_blocked_stream_bound(j.sizeX, j.sizeY) : limg_hip_stream_bound(j.sizeX, j.sizeY);
      const limg_hip_result r = window_fill(j.pStream, j.streamBytes, j.sizeX, j.sizeY, bound, j.window.x0, j.window.y0, j.window.width, j.window.height,
                                            window_out(j.window, pFormat), wp, window_level(j.window));
      if (r != limg_hip_success) return r;
      if (!blocked && j.streamBytes < sizeof(limg_hip_stream_header) + (size_t)wp.nBlocks * sizeof(limg_hip_stream_block)) return limg_hip_error_OutOfBounds;
      units += (unsigned long long)((wp.wbx + (blocked ? 7u : 63u)) / (blocked ? 8u : 64u)) * wp.wby;
      blocks += (unsigned long long)wp.wbx * wp.wby;
    }
    if (units > 0xFFFFFFFFull || blocks > 0xFFFFFFFFull) return limg_hip_error_InvalidParameter;

    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = ensure_stream_status(c, s)) != limg_hip_success) return r;
    // the slot: [jobs | unitBase | groups | groupJobs | groupItemBase] is uploaded; [state | map] behind it exists on the device only (version 2)
    const size_t oJobs = 0, oUnitBase = align16(oJobs + count * sizeof(WindowDecodeParams)), oGroups = align16(oUnitBase + (count + 1) * 4);
    const size_t oGroupJobs = blocked ? align16(oGroups + count * sizeof(WindowGroup)) : oGroups, oItemBase = blocked ? align16(oGroupJobs + count * 4) : oGroups;
    const size_t upload = blocked ? align16(oItemBase + (count + 1) * 4) : oGroups;
    const size_t oState = upload, oMap = align16(oState + (blocked ? count * 8 : 0)), total = oMap + (blocked ? (size_t)blocks * 4 : 0);
    limg_hip_context::WindowSlot &slot = c->windowSlots[c->windowSlotNext];
    c->windowSlotNext = (c->windowSlotNext + 1) % limg_hip_context::kWindowSlots;
    if (slot.busy)
    { // the call that used this slot last: its copy has left the pinned table and its kernels are done with the device copy
      HIP_TRY(hipEventSynchronize(slot.done));
      slot.busy = false;
    }
    if (!slot.done) HIP_TRY(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    if ((r = slot.host.ensure(upload)) != limg_hip_success) return r;
    if ((r = slot.dev.ensure(total)) != limg_hip_success) return r;
    uint8_t *hb = (uint8_t *)slot.host.p, *db = (uint8_t *)slot.dev.p;
    WindowDecodeParams *jobs = (WindowDecodeParams *)(hb + oJobs);
    uint32_t *unitBase = (uint32_t *)(hb + oUnitBase);

    // pass 2: the table (the checks of pass 1 cannot fail again)
    uint32_t unitAt = 0, blockAt = 0;
    for (size_t i = 0; i < count; i++)
    {
      const JOB &j = pJobs[i];
      const size_t bound = blocked ? limg_hip_blocked_stream_bound(j.sizeX, j.sizeY) : limg_hip_stream_bound(j.sizeX, j.sizeY);
      (void)window_fill(j.pStream, j.streamBytes, j.sizeX, j.sizeY, bound, j.window.x0, j.window.y0, j.window.width, j.window.height, window_out(j.window, pFormat), jobs[i],
                        window_level(j.window));
      jobs[i].status = (uint32_t *)c->streamStatus.p;
      if (blocked)
      {
        jobs[i].state = (uint32_t *)(db + oState) + 2 * i;
        jobs[i].map = (uint32_t *)(db + oMap) + blockAt;
      }
      unitBase[i] = unitAt;
      unitAt += ((jobs[i].wbx + (blocked ? 7u : 63u)) / (blocked ? 8u : 64u)) * jobs[i].wby;
      blockAt += jobs[i].wbx * jobs[i].wby;
    }
    unitBase[count] = unitAt;
    WindowBatchParams b;
    memset(&b, 0, sizeof(b));
    b.jobs = (const WindowDecodeParams *)(db + oJobs); b.unitBase = (const uint32_t *)(db + oUnitBase);
    b.count = (uint32_t)count; b.totalUnits = unitAt;
    b.status = (uint32_t *)c->streamStatus.p; b.jobStatus = pJobStatus;
    if (blocked)
    { // groups: the jobs sorted by stream (in place, in the table: no allocation), then one group per run of equal keys
      WindowGroup *groups = (WindowGroup *)(hb + oGroups);
      uint32_t *groupJobs = (uint32_t *)(hb + oGroupJobs), *itemBase = (uint32_t *)(hb + oItemBase);
      for (size_t i = 0; i < count; i++) groupJobs[i] = (uint32_t)i;
      auto less = [jobs](uint32_t x, uint32_t y) {
        const WindowDecodeParams &a = jobs[x], &bb = jobs[y];
        if (a.stream != bb.stream) return (uintptr_t)a.stream < (uintptr_t)bb.stream;
        if (a.streamBytes != bb.streamBytes) return a.streamBytes < bb.streamBytes;
        if (a.sizeX != bb.sizeX) return a.sizeX < bb.sizeX;
        if (a.sizeY != bb.sizeY) return a.sizeY < bb.sizeY;
        return x < y;
      };
      std::sort(groupJobs, groupJobs + count, less);
      uint32_t nGroups = 0;
      unsigned long long items = 0;
      for (size_t i = 0; i < count; i++)
      {
        const WindowDecodeParams &a = jobs[groupJobs[i]];
        if (i == 0 || a.stream != groups[nGroups - 1].stream || a.streamBytes != groups[nGroups - 1].streamBytes || a.sizeX != groups[nGroups - 1].sizeX ||
            a.sizeY != groups[nGroups - 1].sizeY)
        {
          WindowGroup &g = groups[nGroups];
          memset(&g, 0, sizeof(g));
          g.sizeX = a.sizeX; g.sizeY = a.sizeY; g.blocksX = a.blocksX; g.blocksY = a.blocksY; g.nBlocks = a.nBlocks;
          g.firstJob = (uint32_t)i; g.stream = a.stream; g.streamBytes = a.streamBytes;
          itemBase[nGroups++] = (uint32_t)items;
          items += (a.nBlocks + 63u) / 64u; // 64 rectangles per item, at most nBlocks rectangles
        }
        groups[nGroups - 1].nJobs++;
      }
      if (items > 0xFFFFFFFFull) return limg_hip_error_InvalidParameter;
      itemBase[nGroups] = (uint32_t)items;
      b.groups = (const WindowGroup *)(db + oGroups); b.groupJobs = (const uint32_t *)(db + oGroupJobs); b.groupItemBase = (const uint32_t *)(db + oItemBase);
      b.nGroups = nGroups; b.totalItems = (uint32_t)items;
    }
    HIP_TRY(hipMemcpyAsync(db, hb, upload, hipMemcpyHostToDevice, s));
    slot.busy = true; // from here on the slot is in flight, whatever fails below
    if (blocked)
    {
      HIP_TRY(hipMemsetAsync(db + oState, 0, count * 8, s));
      HIP_TRY(hipMemsetAsync(db + oMap, 0xFF, (size_t)blocks * 4, s)); // no block has a rectangle yet
    }
    if (pJobStatus) HIP_TRY(hipMemsetAsync(pJobStatus, 0, count * 4, s));
    if (scaled)
    {
      if (blocked) launch_blocked_stream_windows_scaled(b, tensor ? pFormat : nullptr, device_cus(c), s);
      else launch_stream_windows_scaled(b, tensor ? pFormat : nullptr, device_cus(c), s);
    }
    else if (tensor)
    {
      if (blocked) launch_blocked_stream_windows_tensor(b, *pFormat, device_cus(c), s);
      else launch_stream_windows_tensor(b, *pFormat, device_cus(c), s);
    }
    else if (blocked) launch_blocked_stream_windows_decode(b, device_cus(c), s);
    else launch_stream_windows_decode(b, device_cus(c), s);
    const hipError_t launched = hipGetLastError();
    HIP_TRY(hipEventRecord(slot.done, s));
    HIP_TRY(launched);
    return limg_hip_success;
  }

  // the staged form of a window: densely packed in context memory
  void stage_window(limg_hip_window &w, void *p) { w.pOut = (uint32_t *)p; w.outStridePixels = w.width; }
  void stage_window(limg_hip_tensor_window &w, void *p) { w.pOut = p; w.rowStride = w.width; w.planeStride = w.width * w.height; }
  void stage_window(limg_hip_scaled_window &w, void *p) { w.pOut = (uint32_t *)p; w.outStridePixels = w.width; }
  void stage_window(limg_hip_scaled_tensor_window &w, void *p) { w.pOut = p; w.rowStride = w.width; w.planeStride = w.width * w.height; }
  template <class WIN> struct JobOf { typedef limg_hip_window_job type; };
  template <> struct JobOf<limg_hip_tensor_window> { typedef limg_hip_tensor_window_job type; };
  template <> struct JobOf<limg_hip_scaled_window> { typedef limg_hip_scaled_window_job type; };
  template <> struct JobOf<limg_hip_scaled_tensor_window> { typedef limg_hip_scaled_tensor_window_job type; };

  // `count` windows of ONE host stream.  info(&sizeX, &sizeY, &total): the version's header check.  WIN: limg_hip_window or limg_hip_tensor_window (with pFormat), or
  // their _scaled_ twins: every window then carries its level and is stated, checked and staged in that level's coordinates.
  template <class WIN, class INFO>
  limg_hip_result decode_windows_host(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const WIN *pWindows, size_t count,
                                      const limg_hip_tensor_format *pFormat, bool blocked, INFO &&info)
  {
    typedef typename JobOf<WIN>::type JOB;
    constexpr bool tensor = WindowKind<WIN>::tensor;
    if (!c || !pStream || !pWindows || (tensor && !pFormat)) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (count == 0 || count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    if (tensor && !tensor_format_ok(pFormat)) return limg_hip_error_InvalidParameter;
    for (size_t i = 0; i < count; i++)
    {
      const WIN &w = pWindows[i];
      if (!w.pOut) return limg_hip_error_ArgumentNull;
      if (window_level(w) > 3) return limg_hip_error_InvalidParameter;
      const limg_hip_result ok = window_out_check(w.width, w.height, window_out(w, pFormat));
      if (ok != limg_hip_success) return ok;
      if (tensor && !out_aligned(window_out(w, pFormat))) return limg_hip_error_InvalidParameter;
    }
    size_t sizeX = 0, sizeY = 0, total = 0;
    limg_hip_result r = info(&sizeX, &sizeY, &total);
    if (r != limg_hip_success) return r;
    if (total > streamBytes) return limg_hip_error_OutOfBounds;
    const size_t eb = window_out(pWindows[0], pFormat).elemBytes, planes = tensor ? pFormat->planes : 1;
    const size_t per = 16 / eb;
    size_t elems = 0; // staging: every window at its own width (plane after plane), on a 16-byte boundary
    for (size_t i = 0; i < count; i++)
    {
      const WIN &w = pWindows[i];
      if (!window_inside(sizeX >> window_level(w), sizeY >> window_level(w), w.x0, w.y0, w.width, w.height)) return limg_hip_error_OutOfBounds;
      elems += (planes * w.width * w.height + per - 1) / per * per;
    }
    JOB *jobs = new (std::nothrow) JOB[count];
    if (!jobs) return limg_hip_error_MemoryAllocationFailure;
    struct Free { JOB *p; ~Free() { delete[] p; } } freeJobs = { jobs };
    HIP_TRY(hipSetDevice(c->device));
    if ((r = c->streamBuf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->planes.ensure(elems * eb)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->streamBuf.p, pStream, total, hipMemcpyHostToDevice)); // once, for all windows
    size_t at = 0;
    for (size_t i = 0; i < count; i++)
    {
      const WIN &w = pWindows[i];
      jobs[i].pStream = (const uint8_t *)c->streamBuf.p; jobs[i].streamBytes = total; jobs[i].sizeX = sizeX; jobs[i].sizeY = sizeY;
      jobs[i].window = w;
      stage_window(jobs[i].window, (uint8_t *)c->planes.p + at * eb);
      at += (planes * w.width * w.height + per - 1) / per * per;
    }
    if ((r = decode_windows_device(c, jobs, count, pFormat, nullptr, nullptr, blocked)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r; // a stream refused for any window: no pOut is touched
    for (size_t i = 0; i < count; i++)
    {
      const WIN &w = pWindows[i];
      const WindowOut o = window_out(w, pFormat);
      for (size_t pl = 0; pl < planes; pl++)
        HIP_TRY(hipMemcpy2D((uint8_t *)o.p + pl * o.planeStride * eb, o.rowStride * eb, (const uint8_t *)jobs[i].window.pOut + pl * w.width * w.height * eb, w.width * eb,
                            w.width * eb, w.height, hipMemcpyDeviceToHost));
    }
    return limg_hip_success;
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
    dp.stream = pStream; dp.streamBytes = streamBytes; dp.out = pOut; dp.status = (uint32_t *)c->streamStatus.p; dp.sink = (uint32_t *)((uint8_t *)c->streamStatus.p + 256);
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

  // ---- batched stream encode: a list of same-shape images, stream i = limg_hip_encode_stream_device of image i ----
  // Lists of whole-block images go chunk by chunk (the plane batch's rule) through ONE compact-mode batched encode -- records, shift words and the strips' payload
  // words in the context's raster arrays, image after image; the factor planes in per-image slices of streamFac -- and one scan + one pack launch over the chunk.
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
    const bool oneByOne = count == 1 || ragged || c->opt.legacy_float_stage != 0 || c->forceSplit;
    const size_t most = oneByOne ? 1 : (count < chunk ? count : chunk); // images of the largest chunk
    limg_hip_result r;
    if ((r = c->streamTable.ensure(count * sizeof(StreamImage))) != limg_hip_success) return r;
    if (most > 1)
    { // everything a chunk needs, before the first launch: nothing is grown (and so freed) between the chunks of a list
      if ((r = c->streamFac.ensure(most * planeStride * 3)) != limg_hip_success) return r;
      if ((r = c->streamUnits.ensure(most * imageStrips * 4)) != limg_hip_success) return r;
      if ((r = c->records.ensure(most * blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
      if ((r = c->shifts.ensure(most * blocks * 4)) != limg_hip_success) return r;
    }
    std::vector<StreamImage> images(count);
    for (size_t i = 0; i < count; i++) images[i].stream = ppStreams[i];
    std::vector<ImageIO> table;
    r = limg_hip_success;
    for (size_t i0 = 0; i0 < count && r == limg_hip_success;)
    {
      const size_t n = oneByOne ? 1 : (count - i0 < chunk ? count - i0 : chunk);
      c->statsAccumulate = i0 != 0; // limg_hip_last_stats: all images of the list together, as the plane batch
      if (n == 1)
      { // the single call (images with partial edge blocks, the split path, the float stage inside the encode kernel, a list or a last chunk of one image)
        r = limg_hip_encode_stream_device(c, ppIn[i0], sizeX, sizeY, hasAlpha, ppStreams[i0], capacityEach, nullptr, errorFactor, poolThreads, fastBitCrushing, stream);
        if (r == limg_hip_success && pBytes && !oneByOne) launch_set_stream_table((StreamImage *)c->streamTable.p + i0, &images[i0], 1, s); // (for the sizes below)
      }
      else
      {
        table.assign(n, ImageIO{});
        for (size_t i = 0; i < n; i++)
        {
          uint8_t *fac = (uint8_t *)c->streamFac.p + i * 3 * planeStride; // 256-byte aligned slices
          table[i].in = ppIn[i0 + i];
          table[i].info.pFactorsA = fac; table[i].info.pFactorsB = fac + planeStride; table[i].info.pFactorsC = fac + 2 * planeStride;
          images[i0 + i].fac[0] = fac; images[i0 + i].fac[1] = fac + planeStride; images[i0 + i].fac[2] = fac + 2 * planeStride;
        }
        limg_hip_compact_out comp = { (limg_hip_block_record *)c->records.p, (uint32_t *)c->shifts.p };
        EncodeExtra x;
        x.batch = table.data(); x.batchCount = n;
        x.streamRaw = true; x.stripWords = (uint32_t *)c->streamUnits.p;
        if ((r = encode_device(c, ppIn[i0], sizeX, sizeY, hasAlpha, &table[0].info, &comp, errorFactor, poolThreads, fastBitCrushing, s, x)) != limg_hip_success) break;
        launch_set_stream_table((StreamImage *)c->streamTable.p + i0, &images[i0], n, s);
        StreamBatchParams b;
        memset(&b, 0, sizeof(b));
        b.sizeX = (uint32_t)sizeX; b.sizeY = (uint32_t)sizeY; b.blocksX = (uint32_t)blocksX; b.blocksY = (uint32_t)blocksY; b.nBlocks = (uint32_t)blocks;
        b.channels = hasAlpha ? 4 : 3; b.errorFactor = errorFactor; b.flags = (fastBitCrushing ? 1u : 0u) | (c->opt.dither_pcg ? 2u : 0u);
        b.stripsX = (uint32_t)stripsX; b.imageStrips = (uint32_t)imageStrips; b.nImages = (uint32_t)n; b.nStrips = (uint32_t)(n * imageStrips);
        const size_t slots = (size_t)device_cus(c) * 16; // as the single call: 16 one-wave workgroups per CU -- for the whole chunk
        b.nWaves = (uint32_t)(n * imageStrips < slots ? n * imageStrips : slots);
        b.images = (const StreamImage *)c->streamTable.p + i0;
        b.records = comp.pRecords; b.shifts = comp.pShifts; b.stripWords = (uint32_t *)c->streamUnits.p;
        mark(c, s);
        launch_stream_pack_batch(b, s);
        mark(c, s); mark(c, s); mark(c, s);
        const hipError_t launched = hipGetLastError();
        if (launched != hipSuccess) { c->statsAccumulate = false; HIP_TRY(launched); }
      }
      i0 += n;
    }
    c->statsAccumulate = false;
    if (r != limg_hip_success || !pBytes) return r;
    // the sizes: gathered from the headers on the device, ONE download
    if ((r = c->streamSizes.ensure(count * 8)) != limg_hip_success) return r;
    if (oneByOne) launch_set_stream_table((StreamImage *)c->streamTable.p, images.data(), count, s);
    launch_stream_gather_bytes((const StreamImage *)c->streamTable.p, count, (unsigned long long *)c->streamSizes.p, s);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> sizes(count);
    HIP_TRY(hipMemcpyAsync(sizes.data(), c->streamSizes.p, count * 8, hipMemcpyDeviceToHost, s));
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
    // staging: the images side by side in `in`, the streams at worst-case size (rounded up to 256 bytes) side by side in streamBuf
    const size_t px = sizeX * sizeY, slice = (bound + 255) & ~(size_t)255;
    limg_hip_result r;
    if ((r = c->in.ensure(count * px * 4)) != limg_hip_success) return r;
    if ((r = c->streamBuf.ensure(count * slice)) != limg_hip_success) return r;
    std::vector<const uint32_t *> dIn(count);
    std::vector<uint8_t *> dStreams(count);
    for (size_t i = 0; i < count; i++)
    {
      dIn[i] = (const uint32_t *)c->in.p + i * px;
      dStreams[i] = (uint8_t *)c->streamBuf.p + i * slice;
      HIP_TRY(hipMemcpy((void *)dIn[i], ppIn[i], px * 4, hipMemcpyHostToDevice));
    }
    if ((r = limg_hip_encode_stream_batch_device(c, count, dIn.data(), sizeX, sizeY, hasAlpha, dStreams.data(), slice, pBytes, errorFactor, poolThreads, fastBitCrushing,
                                                 nullptr)) != limg_hip_success)
      return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    for (size_t i = 0; i < count; i++) HIP_TRY(hipMemcpy(ppStreams[i], dStreams[i], pBytes[i], hipMemcpyDeviceToHost)); // totalBytes of each, not the capacity
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
    if (!c->lastBlocked.valid) return limg_hip_error_InvalidParameter; // no merged-block encode on this context, or the last one failed
    const size_t bound = limg_hip_blocked_stream_bound(c->lastBlocked.sizeX, c->lastBlocked.sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = ensure_pack_resources(c, c->lastBlocked.sizeX, c->lastBlocked.sizeY)) != limg_hip_success) return r;
    if ((r = c->streamBuf.ensure(bound)) != limg_hip_success) return r;
    size_t bytes = 0;
    if ((r = pack_last(c, (uint8_t *)c->streamBuf.p, &bytes, nullptr)) != limg_hip_success) return r;
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

  // ---- window decode, both versions ----
  limg_hip_result limg_hip_decode_stream_window_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0, size_t y0,
                                                       size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, void *stream)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    hipStream_t s = (hipStream_t)stream;
    WindowDecodeParams wp;
    const limg_hip_result r = window_params(c, pStream, streamBytes, sizeX, sizeY, limg_hip_stream_bound(sizeX, sizeY), x0, y0, width, height, pOut, outStridePixels, s, wp);
    if (r != limg_hip_success) return r;
    if (streamBytes < sizeof(limg_hip_stream_header) + (size_t)wp.nBlocks * sizeof(limg_hip_stream_block)) return limg_hip_error_OutOfBounds;
    launch_stream_window_decode(wp, device_cus(c), s);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  limg_hip_result limg_hip_blocked_decode_stream_window_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0, size_t y0,
                                                               size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, void *stream)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    hipStream_t s = (hipStream_t)stream;
    WindowDecodeParams wp;
    const limg_hip_result r = window_params(c, pStream, streamBytes, sizeX, sizeY, limg_hip_blocked_stream_bound(sizeX, sizeY), x0, y0, width, height, pOut, outStridePixels, s, wp);
    if (r != limg_hip_success) return r;
    return blocked_window_decode(c, wp, s);
  }

  limg_hip_result limg_hip_decode_stream_window(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height,
                                                uint32_t *pOut, size_t outStridePixels)
  {
    return decode_window_host(c, pStream, streamBytes, x0, y0, width, height, pOut, outStridePixels,
                              [&](size_t *w, size_t *h, size_t *total) { return limg_hip_stream_info(pStream, streamBytes, w, h, nullptr, total); },
                              [&](const uint8_t *dStream, size_t bytes, size_t w, size_t h, uint32_t *dOut) {
                                return limg_hip_decode_stream_window_device(c, dStream, bytes, w, h, x0, y0, width, height, dOut, width, nullptr);
                              });
  }

  limg_hip_result limg_hip_blocked_decode_stream_window(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height,
                                                        uint32_t *pOut, size_t outStridePixels)
  {
    return decode_window_host(c, pStream, streamBytes, x0, y0, width, height, pOut, outStridePixels,
                              [&](size_t *w, size_t *h, size_t *total) { return limg_hip_blocked_stream_info(pStream, streamBytes, w, h, nullptr, total, nullptr); },
                              [&](const uint8_t *dStream, size_t bytes, size_t w, size_t h, uint32_t *dOut) {
                                return limg_hip_blocked_decode_stream_window_device(c, dStream, bytes, w, h, x0, y0, width, height, dOut, width, nullptr);
                              });
  }

  // ---- batched window decode, both versions ----
  limg_hip_result limg_hip_decode_stream_windows_device(limg_hip_context *c, const limg_hip_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream)
  {
    return decode_windows_device(c, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream, false);
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows_device(limg_hip_context *c, const limg_hip_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream)
  {
    return decode_windows_device(c, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream, true);
  }

  limg_hip_result limg_hip_decode_stream_windows(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_window *pWindows, size_t count)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, nullptr, false,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_stream_info(pStream, streamBytes, w, h, nullptr, total); });
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_window *pWindows, size_t count)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, nullptr, true,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_blocked_stream_info(pStream, streamBytes, w, h, nullptr, total, nullptr); });
  }

  // ---- batched window decode into planar float tensors, both versions ----
  limg_hip_result limg_hip_decode_stream_windows_tensor_device(limg_hip_context *c, const limg_hip_tensor_window_job *pJobs, size_t count, const limg_hip_tensor_format *pFormat,
                                                               uint32_t *pJobStatus, void *stream)
  {
    return decode_windows_device(c, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream, false);
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows_tensor_device(limg_hip_context *c, const limg_hip_tensor_window_job *pJobs, size_t count,
                                                                       const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  {
    return decode_windows_device(c, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream, true);
  }

  limg_hip_result limg_hip_decode_stream_windows_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_tensor_window *pWindows, size_t count,
                                                        const limg_hip_tensor_format *pFormat)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, pFormat, false,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_stream_info(pStream, streamBytes, w, h, nullptr, total); });
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_tensor_window *pWindows,
                                                                size_t count, const limg_hip_tensor_format *pFormat)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, pFormat, true,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_blocked_stream_info(pStream, streamBytes, w, h, nullptr, total, nullptr); });
  }

  // ---- reduced-scale window decode, both versions, RGBA8 and tensors: the job types with a level ----
  limg_hip_result limg_hip_decode_stream_windows_scaled_device(limg_hip_context *c, const limg_hip_scaled_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream)
  {
    return decode_windows_device(c, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream, false);
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_device(limg_hip_context *c, const limg_hip_scaled_window_job *pJobs, size_t count, uint32_t *pJobStatus,
                                                                       void *stream)
  {
    return decode_windows_device(c, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream, true);
  }

  limg_hip_result limg_hip_decode_stream_windows_scaled_tensor_device(limg_hip_context *c, const limg_hip_scaled_tensor_window_job *pJobs, size_t count,
                                                                      const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  {
    return decode_windows_device(c, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream, false);
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_tensor_device(limg_hip_context *c, const limg_hip_scaled_tensor_window_job *pJobs, size_t count,
                                                                              const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  {
    return decode_windows_device(c, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream, true);
  }

  limg_hip_result limg_hip_decode_stream_windows_scaled(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_window *pWindows, size_t count)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, nullptr, false,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_stream_info(pStream, streamBytes, w, h, nullptr, total); });
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_window *pWindows,
                                                                size_t count)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, nullptr, true,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_blocked_stream_info(pStream, streamBytes, w, h, nullptr, total, nullptr); });
  }

  limg_hip_result limg_hip_decode_stream_windows_scaled_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_tensor_window *pWindows,
                                                               size_t count, const limg_hip_tensor_format *pFormat)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, pFormat, false,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_stream_info(pStream, streamBytes, w, h, nullptr, total); });
  }

  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes,
                                                                       const limg_hip_scaled_tensor_window *pWindows, size_t count, const limg_hip_tensor_format *pFormat)
  {
    return decode_windows_host(c, pStream, streamBytes, pWindows, count, pFormat, true,
                               [&](size_t *w, size_t *h, size_t *total) { return limg_hip_blocked_stream_info(pStream, streamBytes, w, h, nullptr, total, nullptr); });
  }
}
