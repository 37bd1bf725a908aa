// limg_hip_stream_window_api.hip -- the window decode entries of the C ABI (limg_hip_*decode_stream_window*; kernels: limg_hip_stream_window.hip): one window or a
// table of them, into packed RGBA8 or planar float tensors, at full or reduced scale, from device or host memory, of either stream version.  Three things vary and each
// is stated once: the stream version (StreamVersion: two constants), the public window struct (window_view / stage_window) and where the pixels go (WindowOut).
// The error entries (limg_hip_*decode_stream_windows_error*, limg_hip_stream_compare, limg_hip_error_sum_for_psnr) are the batched RGBA8 entries with a window whose
// pixels come from the caller -- the original the decode is compared with -- and a sum per job as the only thing written.
// No kernel lives here.
#include "limg_hip_context.h"

#include <math.h>

#include <algorithm>
#include <type_traits>

using namespace limg_hip;

namespace
{
  // ---- what the host needs to know about a stream version ----
  struct StreamVersion
  {
    size_t (*bound)(size_t sizeX, size_t sizeY);                                                                        // limg_hip_*stream_bound
    limg_hip_result (*info)(const uint8_t *pStream, size_t bytes, size_t *pSizeX, size_t *pSizeY, size_t *pTotalBytes); // the header check
    uint32_t unitLog2; // a decode unit is a run of up to 64 (version 1) or 8 (version 2) blocks of one block row of the window: log2 of that width
    bool rectangles;   // the table holds rectangles: decoding needs the block -> rectangle map, the state words and, batched, the stream groups
    bool tableExtent;  // one entry per block: streamBytes >= header + nBlocks * entry is known, and checked, on the host
  };
  const StreamVersion kVersion1 = { limg_hip_stream_bound,
                                    [](const uint8_t *p, size_t n, size_t *w, size_t *h, size_t *total) { return limg_hip_stream_info(p, n, w, h, nullptr, total); }, 6u, false, true };
  const StreamVersion kVersion2 = { limg_hip_blocked_stream_bound,
                                    [](const uint8_t *p, size_t n, size_t *w, size_t *h, size_t *total) { return limg_hip_blocked_stream_info(p, n, w, h, nullptr, total, nullptr); },
                                    3u, true, false };
  uint32_t window_units(const StreamVersion &v, const WindowDecodeParams &wp) { return ((wp.wbx + (1u << v.unitLog2) - 1u) >> v.unitLog2) * wp.wby; }

  // ---- one view of a window ----
  // Where a window's pixels go: packed RGBA8 (planes == 0: elemBytes 4, one element per pixel) or `planes` planes of float / _Float16 (the tensor entries).
  struct WindowOut
  {
    void *p;
    size_t rowStride, planeStride; // in elements
    uint32_t elemBytes, planes;
  };
  // any of the four public window structs; level: the scaled ones' log2Scale (the others are level 0), the window is in that level's coordinates
  // ... or of the two resized ones: x0 .. height is then the SOURCE rectangle in full-resolution pixels, level may be LIMG_HIP_RESIZE_AUTO, and the output has a
  // size of its own
  struct WindowView
  {
    size_t x0, y0, width, height, level;
    WindowOut out;
    bool resized;
    size_t outW, outH;
    uint32_t flags;
  };
  template <class WIN, class = void> struct IsPlanar : std::false_type {}; // limg_hip_[scaled_]tensor_window: rowStride and planeStride, pixels of the format's type
  template <class WIN> struct IsPlanar<WIN, std::void_t<decltype(WIN::planeStride)>> : std::true_type {};
  template <class WIN, class = void> struct IsScaled : std::false_type {}; // limg_hip_scaled_[tensor_]window: log2Scale
  template <class WIN> struct IsScaled<WIN, std::void_t<decltype(WIN::log2Scale)>> : std::true_type {};
  template <class WIN, class = void> struct IsResized : std::false_type {}; // limg_hip_resized_[tensor_]window: outWidth, outHeight, flags
  template <class WIN> struct IsResized<WIN, std::void_t<decltype(WIN::outWidth)>> : std::true_type {};
  template <class WIN, class = void> struct IsError : std::false_type {}; // limg_hip_error_window: pOriginal and its stride where the others have pOut -- read, never written
  template <class WIN> struct IsError<WIN, std::void_t<decltype(WIN::pOriginal)>> : std::true_type {};

  // the window's pixels: the output of every entry but the error ones, whose window names the original
  template <class WIN> void *window_pixels(const WIN &w)
  {
    if constexpr (IsError<WIN>::value) return (void *)w.pOriginal;
    else return (void *)w.pOut;
  }
  template <class WIN> WindowView window_view(const WIN &w, const limg_hip_tensor_format *f)
  {
    WindowView v = { w.x0, w.y0, w.width, w.height, 0, { window_pixels(w), 0, 0, 4u, 0u } };
    if constexpr (IsPlanar<WIN>::value) v.out = { w.pOut, w.rowStride, w.planeStride, f->type == LIMG_HIP_TENSOR_F16 ? 2u : 4u, f->planes };
    else if constexpr (IsError<WIN>::value) v.out.rowStride = w.originalStridePixels;
    else v.out.rowStride = w.outStridePixels;
    if constexpr (IsScaled<WIN>::value) v.level = w.log2Scale;
    if constexpr (IsResized<WIN>::value) { v.resized = true; v.outW = w.outWidth; v.outH = w.outHeight; v.flags = w.flags; }
    return v;
  }
  // ... and back: the staged form of a window, densely packed at `p`
  template <class WIN> void stage_window(WIN &w, void *p)
  {
    size_t width = w.width, height = w.height;
    if constexpr (IsResized<WIN>::value) { width = w.outWidth; height = w.outHeight; }
    if constexpr (IsError<WIN>::value) { w.pOriginal = (const uint32_t *)p; w.originalStridePixels = width; }
    else
    {
      w.pOut = (decltype(w.pOut))p;
      if constexpr (IsPlanar<WIN>::value) { w.rowStride = width; w.planeStride = width * height; }
      else w.outStridePixels = width;
    }
  }
  WindowView rgba_view(size_t x0, size_t y0, size_t width, size_t height, uint32_t *pOut, size_t outStridePixels)
  {
    return { x0, y0, width, height, 0, { pOut, outStridePixels, 0, 4u, 0u } };
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
  bool window_inside(size_t sizeX, size_t sizeY, const WindowView &w)
  {
    return !(w.x0 >= sizeX || w.width > sizeX - w.x0 || w.y0 >= sizeY || w.height > sizeY - w.y0);
  }

  // ---- the same three checks for any view: a resized one states its strides on the output's size and carries a level that may be AUTO ----
  size_t out_width(const WindowView &w) { return w.resized ? w.outW : w.width; }
  size_t out_height(const WindowView &w) { return w.resized ? w.outH : w.height; }
  // what is checked where a zero width is
  limg_hip_result view_size_check(const WindowView &w)
  {
    if (!w.resized) return w.level > 3 ? limg_hip_error_InvalidParameter : window_out_check(w.width, w.height, w.out);
    if ((w.level > 3 && w.level != LIMG_HIP_RESIZE_AUTO) || (w.flags & ~LIMG_HIP_RESIZE_FLIP_X) != 0 || w.width == 0 || w.height == 0) return limg_hip_error_InvalidParameter;
    if (w.outW == 0 || w.outW > 32768 || w.outH == 0 || w.outH > 32768) return limg_hip_error_InvalidParameter;
    return window_out_check(w.outW, w.outH, w.out);
  }
  // a resized view's level: AUTO is the deepest level that leaves at least one level pixel per output pixel on both axes
  uint32_t resize_level(const WindowView &w)
  {
    if (w.level != LIMG_HIP_RESIZE_AUTO) return (uint32_t)w.level;
    uint32_t L = 0;
    while (L < 3 && (w.width >> (L + 1)) >= w.outW && (w.height >> (L + 1)) >= w.outH) L++;
    return L;
  }
  // scaled: the window inside the level's image; resized: the rectangle inside the image, and its first column and row among those the level keeps
  bool view_inside(size_t sizeX, size_t sizeY, const WindowView &w)
  {
    if (!w.resized) return window_inside(sizeX >> w.level, sizeY >> w.level, w);
    if (!window_inside(sizeX, sizeY, w)) return false;
    const uint32_t L = resize_level(w);
    const size_t RX = sizeX >> L, RY = sizeY >> L;
    return RX != 0 && RY != 0 && (w.x0 >> L) <= RX - 1 && (w.y0 >> L) <= RY - 1;
  }

  // the checks and the parameters the two versions share, without touching the device; `bound`: the version's limg_hip_*stream_bound(sizeX, sizeY).  status, map and
  // state are the caller's to set.  A window at level > 0 lies inside (sizeX >> level) x (sizeY >> level), and wp gets its source footprint (x0 .. height times
  // 1 << level: inside the image, so nothing overflows) with vecOut stated on the window itself.
  limg_hip_result window_fill(const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t bound, const WindowView &w, WindowDecodeParams &wp)
  {
    const WindowOut &o = w.out;
    if (view_size_check(w) != limg_hip_success || bound == 0 || streamBytes < sizeof(limg_hip_stream_header)) return limg_hip_error_InvalidParameter;
    if (((uintptr_t)pStream & 15u) != 0 || !out_aligned(o)) return limg_hip_error_InvalidParameter;
    if (!view_inside(sizeX, sizeY, w)) return limg_hip_error_OutOfBounds;
    const size_t level = w.resized ? resize_level(w) : w.level;
    size_t x0 = w.x0 << level, y0 = w.y0 << level, width = w.width << level, height = w.height << level;
    if (w.resized)
    { // the footprint: the level pixels lo .. hi of both axes, in full-resolution pixels
      const size_t lox = w.x0 >> level, loy = w.y0 >> level;
      const size_t hix = resize_hi((uint32_t)w.x0, (uint32_t)w.width, (uint32_t)level, (uint32_t)sizeX), hiy = resize_hi((uint32_t)w.y0, (uint32_t)w.height, (uint32_t)level, (uint32_t)sizeY);
      x0 = lox << level; y0 = loy << level; width = (hix - lox + 1) << level; height = (hiy - loy + 1) << level;
    }
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
    wp.vecOut = !w.resized && ((uintptr_t)o.p & 15u) == 0 && o.rowStride % per == 0 && o.planeStride % per == 0 && w.x0 % per == 0; // (resized: one element per store)
    wp.log2Scale = (uint32_t)level;
    return limg_hip_success;
  }
}

limg_hip_result limg_hip::window_params(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t bound, size_t x0, size_t y0,
                                        size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, hipStream_t s, WindowDecodeParams &wp)
{
  limg_hip_result r = window_fill(pStream, streamBytes, sizeX, sizeY, bound, rgba_view(x0, y0, width, height, pOut, outStridePixels), wp);
  if (r != limg_hip_success) return r;
  HIP_TRY(hipSetDevice(c->device));
  if ((r = ensure_stream_status(c, s)) != limg_hip_success) return r;
  wp.status = (uint32_t *)c->stream.status.p;
  return limg_hip_success;
}

// the map of the window's blocks (not the image's) and the call's state words, then the two kernels
limg_hip_result limg_hip::blocked_window_decode(limg_hip_context *c, WindowDecodeParams &wp, hipStream_t s)
{
  const size_t mapBytes = (size_t)wp.wbx * wp.wby * 4;
  limg_hip_result r;
  if ((r = c->stream.bsMap.ensure(mapBytes)) != limg_hip_success) return r;
  if ((r = c->stream.bsState.ensure(64)) != limg_hip_success) return r;
  HIP_TRY(hipMemsetAsync(c->stream.bsMap.p, 0xFF, mapBytes, s)); // no block has a rectangle yet
  HIP_TRY(hipMemsetAsync(c->stream.bsState.p, 0, 64, s));
  wp.map = (uint32_t *)c->stream.bsMap.p; wp.state = (uint32_t *)c->stream.bsState.p;
  launch_blocked_stream_window_decode(wp, device_cus(c), s);
  HIP_TRY(hipGetLastError());
  return limg_hip_success;
}

namespace
{
  // ---- one window: limg_hip_*decode_stream_window[_device] ----
  limg_hip_result decode_window_device(limg_hip_context *c, const StreamVersion &v, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0, size_t y0,
                                       size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, hipStream_t s)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    WindowDecodeParams wp;
    const limg_hip_result r = window_params(c, pStream, streamBytes, sizeX, sizeY, v.bound(sizeX, sizeY), x0, y0, width, height, pOut, outStridePixels, s, wp);
    if (r != limg_hip_success) return r;
    if (v.rectangles) return blocked_window_decode(c, wp, s);
    if (streamBytes < sizeof(limg_hip_stream_header) + (size_t)wp.nBlocks * sizeof(limg_hip_stream_block)) return limg_hip_error_OutOfBounds;
    launch_stream_window_decode(wp, device_cus(c), s);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  // the host form: the stream into context memory, the window into context staging at stride `width`; only a stream that passed reaches pOut
  limg_hip_result decode_window_host(limg_hip_context *c, const StreamVersion &v, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height,
                                     uint32_t *pOut, size_t outStridePixels)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const WindowView w = rgba_view(x0, y0, width, height, pOut, outStridePixels);
    limg_hip_result r = window_out_check(width, height, w.out);
    if (r != limg_hip_success) return r;
    size_t sizeX = 0, sizeY = 0, total = 0;
    if ((r = v.info(pStream, streamBytes, &sizeX, &sizeY, &total)) != limg_hip_success) return r;
    if (total > streamBytes || !window_inside(sizeX, sizeY, w)) return limg_hip_error_OutOfBounds;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = c->stream.buf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->host.planes.ensure(width * height * 4)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->stream.buf.p, pStream, total, hipMemcpyHostToDevice));
    if ((r = decode_window_device(c, v, (const uint8_t *)c->stream.buf.p, total, sizeX, sizeY, x0, y0, width, height, (uint32_t *)c->host.planes.p, width, nullptr)) != limg_hip_success)
      return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy2D(pOut, outStridePixels * 4, c->host.planes.p, width * 4, width * 4, height, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  // ---- batched: limg_hip_*decode_stream_windows* ----
  size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

  // A resized job's output tiles: the largest tiles, at most kResizeTileEdge on a side, whose level-L footprint -- the taps of a tile's first and last output column
  // and row, by the kernel's own arithmetic -- holds at most `cap` level pixels for EVERY tile of the job; the side with the wider footprint shrinks by an eighth until it does.
  // A tile of one output pixel taps 2 x 2 at most, so the search ends (cap >= 4).  wp: the job's filled parameters (its footprint and level).
  void plan_tiles(const WindowView &w, const WindowDecodeParams &wp, uint32_t cap, ResizeJob &rj)
  {
    const uint32_t L = wp.log2Scale, lox = wp.x0 >> L, hix = lox + (wp.width >> L) - 1u, loy = wp.y0 >> L, hiy = loy + (wp.height >> L) - 1u;
    memset(&rj, 0, sizeof(rj));
    rj.outW = (uint32_t)w.outW; rj.outH = (uint32_t)w.outH;
    rj.x0 = (uint32_t)w.x0; rj.y0 = (uint32_t)w.y0; rj.srcW = (uint32_t)w.width; rj.srcH = (uint32_t)w.height;
    rj.flags = w.flags;
    const unsigned long long step = (unsigned long long)rj.srcH << 18;
    rj.stepQ = step / rj.outH; rj.stepR = (uint32_t)(step % rj.outH);
    // the widest footprint of a tile of `t` outputs along an axis (a mirrored axis cuts its tiles from the other end)
    auto span = [L](uint32_t out, uint32_t t, bool flip, uint32_t s0, uint32_t len, uint32_t lo, uint32_t hi) {
      uint32_t worst = 0;
      for (uint32_t X0 = 0; X0 < out; X0 += t)
      {
        const uint32_t n = std::min(t, out - X0), first = flip ? out - X0 - n : X0;
        worst = std::max(worst, resize_axis(first + n - 1u, s0, len, out, L, lo, hi).b - resize_axis(first, s0, len, out, L, lo, hi).a + 1u);
      }
      return worst;
    };
    uint32_t tw = std::min(rj.outW, kResizeTileEdge), th = std::min(rj.outH, kResizeTileEdge);
    for (;;)
    {
      const uint32_t fw = span(rj.outW, tw, (rj.flags & LIMG_HIP_RESIZE_FLIP_X) != 0, rj.x0, rj.srcW, lox, hix), fh = span(rj.outH, th, false, rj.y0, rj.srcH, loy, hiy);
      if ((unsigned long long)fw * fh <= cap) break;
      if ((fw >= fh && tw > 1u) || th == 1u) tw -= std::max(1u, tw / 8u);
      else th -= std::max(1u, th / 8u);
    }
    rj.tileW = tw; rj.tileH = th; rj.tilesX = (rj.outW + tw - 1u) / tw;
  }
  unsigned long long tile_count(const ResizeJob &rj) { return (unsigned long long)rj.tilesX * ((rj.outH + rj.tileH - 1u) / rj.tileH); }

  // One call: every job checked on the host before anything touches the device, then the job table built in a pinned slot of the context's ring, copied on `s`,
  // and the version's one (two) launches.  JOB: any of the four public job types -- its window says whether the pixels go to planes of pFormat's type (else pFormat is
  // not looked at) and whether it carries a level, which then selects the scaled kernels: the same checks, table and launches otherwise.  The error job type: its
  // window names the original, which is checked as an output is and never written; pErrorSums (device, count) is zeroed on `s` and is all the launch writes.
  template <class JOB>
  limg_hip_result decode_windows_device(limg_hip_context *c, const StreamVersion &v, const JOB *pJobs, size_t count, const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus,
                                        hipStream_t s, uint64_t *pErrorSums = nullptr)
  {
    typedef decltype(JOB::window) WIN;
    constexpr bool tensor = IsPlanar<WIN>::value, scaled = IsScaled<WIN>::value, resized = IsResized<WIN>::value, error = IsError<WIN>::value;
    if (!c || !pJobs || (tensor && !pFormat) || (error && !pErrorSums)) return limg_hip_error_ArgumentNull;
    if (count == 0 || count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    if (tensor && !tensor_format_ok(pFormat)) return limg_hip_error_InvalidParameter;
    const bool rects = v.rectangles;
    auto fill = [&v, pFormat](const JOB &j, WindowDecodeParams &wp) {
      return window_fill(j.pStream, j.streamBytes, j.sizeX, j.sizeY, v.bound(j.sizeX, j.sizeY), window_view(j.window, pFormat), wp);
    };
    // pass 1: the single-window entry's checks, job by job in its order; the sums the table's layout needs
    unsigned long long units = 0, blocks = 0, tiles = 0;
    // (the resized entries) the tile capacity the host plans with: the kernel's, or the test build's smaller one
    const uint32_t tileCap = TOPT(c, resize_tile_pixels) > 0 ? std::max(4u, std::min((uint32_t)TOPT(c, resize_tile_pixels), kResizeTilePixels)) : kResizeTilePixels;
    WindowDecodeParams wp;
    ResizeJob rj;
    for (size_t i = 0; i < count; i++)
    {
      const JOB &j = pJobs[i];
      if (!j.pStream || !window_pixels(j.window)) return limg_hip_error_ArgumentNull;
      const limg_hip_result r = fill(j, wp);
      if (r != limg_hip_success) return r;
      if (v.tableExtent && j.streamBytes < sizeof(limg_hip_stream_header) + (size_t)wp.nBlocks * sizeof(limg_hip_stream_block)) return limg_hip_error_OutOfBounds;
      units += window_units(v, wp);
      blocks += (unsigned long long)wp.wbx * wp.wby;
      if (resized)
      {
        plan_tiles(window_view(j.window, pFormat), wp, tileCap, rj);
        tiles += tile_count(rj);
      }
    }
    if (units > 0xFFFFFFFFull || blocks > 0xFFFFFFFFull || tiles > 0xFFFFFFFFull) return limg_hip_error_InvalidParameter;

    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = ensure_stream_status(c, s)) != limg_hip_success) return r;
    // the slot: [jobs | unitBase | groups | groupJobs | groupItemBase | resize | tileBase] is uploaded (the last two: the resized entries' second per-job table and
    // the prefix of its tile counts); [state | map] behind it exists on the device only (version 2)
    const size_t oJobs = 0, oUnitBase = align16(oJobs + count * sizeof(WindowDecodeParams)), oGroups = align16(oUnitBase + (count + 1) * 4);
    const size_t oGroupJobs = rects ? align16(oGroups + count * sizeof(WindowGroup)) : oGroups, oItemBase = rects ? align16(oGroupJobs + count * 4) : oGroups;
    const size_t oResize = rects ? align16(oItemBase + (count + 1) * 4) : oGroups, oTileBase = resized ? align16(oResize + count * sizeof(ResizeJob)) : oResize;
    const size_t upload = resized ? align16(oTileBase + (count + 1) * 4) : oResize;
    const size_t oState = upload, oMap = align16(oState + (rects ? count * 8 : 0)), total = oMap + (rects ? (size_t)blocks * 4 : 0);
    limg_hip_context::WindowSlot &slot = c->window.slots[c->window.next];
    c->window.next = (c->window.next + 1) % limg_hip_context::kWindowSlots;
    if (slot.busy)
    { // the call that used this slot last: its copy has left the pinned table and its kernels are done with the device copy
      HIP_TRY(hipEventSynchronize(slot.done));
      slot.busy = false;
    }
    if ((r = slot.done.ensure(hipEventDisableTiming)) != limg_hip_success) return r;
    if ((r = slot.host.ensure(upload)) != limg_hip_success) return r;
    if ((r = slot.dev.ensure(total)) != limg_hip_success) return r;
    uint8_t *hb = (uint8_t *)slot.host.p, *db = (uint8_t *)slot.dev.p;
    WindowDecodeParams *jobs = (WindowDecodeParams *)(hb + oJobs);
    uint32_t *unitBase = (uint32_t *)(hb + oUnitBase);

    // pass 2: the table (the checks of pass 1 cannot fail again)
    uint32_t unitAt = 0, blockAt = 0, tileAt = 0;
    ResizeJob *resize = (ResizeJob *)(hb + oResize);
    uint32_t *tileBase = (uint32_t *)(hb + oTileBase);
    for (size_t i = 0; i < count; i++)
    {
      (void)fill(pJobs[i], jobs[i]);
      if (resized)
      {
        plan_tiles(window_view(pJobs[i].window, pFormat), jobs[i], tileCap, resize[i]);
        tileBase[i] = tileAt;
        tileAt += (uint32_t)tile_count(resize[i]);
      }
      jobs[i].status = (uint32_t *)c->stream.status.p;
      if (rects)
      {
        jobs[i].state = (uint32_t *)(db + oState) + 2 * i;
        jobs[i].map = (uint32_t *)(db + oMap) + blockAt;
      }
      unitBase[i] = unitAt;
      unitAt += window_units(v, jobs[i]);
      blockAt += jobs[i].wbx * jobs[i].wby;
    }
    unitBase[count] = unitAt;
    if (resized) tileBase[count] = tileAt;
    WindowBatchParams b;
    memset(&b, 0, sizeof(b));
    b.jobs = (const WindowDecodeParams *)(db + oJobs); b.unitBase = (const uint32_t *)(db + oUnitBase);
    b.count = (uint32_t)count; b.totalUnits = unitAt;
    b.status = (uint32_t *)c->stream.status.p; b.jobStatus = pJobStatus;
    b.errorSums = (unsigned long long *)pErrorSums;
    if (rects)
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
    if (rects)
    {
      HIP_TRY(hipMemsetAsync(db + oState, 0, count * 8, s));
      HIP_TRY(hipMemsetAsync(db + oMap, 0xFF, (size_t)blocks * 4, s)); // no block has a rectangle yet
    }
    if (pJobStatus) HIP_TRY(hipMemsetAsync(pJobStatus, 0, count * 4, s));
    if (error)
    {
      HIP_TRY(hipMemsetAsync(pErrorSums, 0, count * 8, s));
      (rects ? launch_blocked_stream_windows_error : launch_stream_windows_error)(b, device_cus(c), s);
    }
    else if (resized)
    { // a workgroup per output tile; version 2's map kernel first, as it is
      const WindowResizeParams rp = { b, (const ResizeJob *)(db + oResize), (const uint32_t *)(db + oTileBase), tileAt };
      (rects ? launch_blocked_stream_windows_resized : launch_stream_windows_resized)(rp, tensor ? pFormat : nullptr, device_cus(c), s);
    }
    else
      (rects ? launch_blocked_stream_windows : launch_stream_windows)(b, scaled, tensor ? pFormat : nullptr, device_cus(c), s);
    const hipError_t launched = hipGetLastError();
    HIP_TRY(hipEventRecord(slot.done, s));
    HIP_TRY(launched);
    return limg_hip_success;
  }

  // `count` windows of ONE host stream, JOB as above: every window is stated, checked and staged in its level's coordinates.  The error job type: the staged windows
  // are the originals, which go UP in front of the call, and what comes down behind the status check are the `count` sums (pErrorSums, host), staged behind them.
  template <class JOB>
  limg_hip_result decode_windows_host(limg_hip_context *c, const StreamVersion &v, const uint8_t *pStream, size_t streamBytes, const decltype(JOB::window) *pWindows, size_t count,
                                      const limg_hip_tensor_format *pFormat, uint64_t *pErrorSums = nullptr)
  {
    constexpr bool tensor = IsPlanar<decltype(JOB::window)>::value, error = IsError<decltype(JOB::window)>::value;
    if (!c || !pStream || !pWindows || (tensor && !pFormat) || (error && !pErrorSums)) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (count == 0 || count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    if (tensor && !tensor_format_ok(pFormat)) return limg_hip_error_InvalidParameter;
    for (size_t i = 0; i < count; i++)
    {
      const WindowView w = window_view(pWindows[i], pFormat);
      if (!w.out.p) return limg_hip_error_ArgumentNull;
      const limg_hip_result ok = view_size_check(w);
      if (ok != limg_hip_success) return ok;
      if (tensor && !out_aligned(w.out)) return limg_hip_error_InvalidParameter;
    }
    size_t sizeX = 0, sizeY = 0, total = 0;
    limg_hip_result r = v.info(pStream, streamBytes, &sizeX, &sizeY, &total);
    if (r != limg_hip_success) return r;
    if (total > streamBytes) return limg_hip_error_OutOfBounds;
    const size_t eb = window_view(pWindows[0], pFormat).out.elemBytes, planes = tensor ? pFormat->planes : 1;
    const size_t per = 16 / eb;
    size_t elems = 0; // staging: every window at its own width (plane after plane), on a 16-byte boundary
    for (size_t i = 0; i < count; i++)
    {
      const WindowView w = window_view(pWindows[i], pFormat);
      if (!view_inside(sizeX, sizeY, w)) return limg_hip_error_OutOfBounds;
      elems += (planes * out_width(w) * out_height(w) + per - 1) / per * per;
    }
    JOB *jobs = new (std::nothrow) JOB[count];
    if (!jobs) return limg_hip_error_MemoryAllocationFailure;
    struct Free { JOB *p; ~Free() { delete[] p; } } freeJobs = { jobs };
    HIP_TRY(hipSetDevice(c->device));
    if ((r = c->stream.buf.ensure(total + 16)) != limg_hip_success) return r;
    if ((r = c->host.planes.ensure(elems * eb + (error ? count * 8 : 0))) != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->stream.buf.p, pStream, total, hipMemcpyHostToDevice)); // once, for all windows
    uint64_t *dSums = error ? (uint64_t *)((uint8_t *)c->host.planes.p + elems * eb) : nullptr; // (elems * eb is a multiple of 16)
    size_t at = 0;
    for (size_t i = 0; i < count; i++)
    {
      jobs[i].pStream = (const uint8_t *)c->stream.buf.p; jobs[i].streamBytes = total; jobs[i].sizeX = sizeX; jobs[i].sizeY = sizeY;
      jobs[i].window = pWindows[i];
      stage_window(jobs[i].window, (uint8_t *)c->host.planes.p + at * eb);
      const WindowView w = window_view(pWindows[i], pFormat);
      if (error) HIP_TRY(hipMemcpy2D(window_pixels(jobs[i].window), w.width * 4, w.out.p, w.out.rowStride * 4, w.width * 4, w.height, hipMemcpyHostToDevice));
      at += (planes * out_width(w) * out_height(w) + per - 1) / per * per;
    }
    if ((r = decode_windows_device(c, v, jobs, count, pFormat, nullptr, nullptr, dSums)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r; // a stream refused for any window: no pOut (no sum) is touched
    if (error)
    { // (the copy waits for the null stream's kernels)
      HIP_TRY(hipMemcpy(pErrorSums, dSums, count * 8, hipMemcpyDeviceToHost));
      return limg_hip_success;
    }
    for (size_t i = 0; i < count; i++)
    {
      const WindowView w = window_view(pWindows[i], pFormat);
      const size_t ow = out_width(w), oh = out_height(w);
      for (size_t pl = 0; pl < planes; pl++)
        HIP_TRY(hipMemcpy2D((uint8_t *)w.out.p + pl * w.out.planeStride * eb, w.out.rowStride * eb, (const uint8_t *)window_pixels(jobs[i].window) + pl * ow * oh * eb, ow * eb, ow * eb, oh,
                            hipMemcpyDeviceToHost));
    }
    return limg_hip_success;
  }
}

// every entry: its version's constant, its job type, the caller's arguments
extern "C"
{
  // ---- one window ----
  limg_hip_result limg_hip_decode_stream_window_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0, size_t y0,
                                                       size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, void *stream)
  { return decode_window_device(c, kVersion1, pStream, streamBytes, sizeX, sizeY, x0, y0, width, height, pOut, outStridePixels, (hipStream_t)stream); }
  limg_hip_result limg_hip_blocked_decode_stream_window_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0, size_t y0,
                                                               size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, void *stream)
  { return decode_window_device(c, kVersion2, pStream, streamBytes, sizeX, sizeY, x0, y0, width, height, pOut, outStridePixels, (hipStream_t)stream); }
  limg_hip_result limg_hip_decode_stream_window(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height, uint32_t *pOut,
                                                size_t outStridePixels)
  { return decode_window_host(c, kVersion1, pStream, streamBytes, x0, y0, width, height, pOut, outStridePixels); }
  limg_hip_result limg_hip_blocked_decode_stream_window(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height,
                                                        uint32_t *pOut, size_t outStridePixels)
  { return decode_window_host(c, kVersion2, pStream, streamBytes, x0, y0, width, height, pOut, outStridePixels); }

  // ---- batched, packed RGBA8 ----
  limg_hip_result limg_hip_decode_stream_windows_device(limg_hip_context *c, const limg_hip_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion1, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_device(limg_hip_context *c, const limg_hip_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion2, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_decode_stream_windows(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_window *pWindows, size_t count)
  { return decode_windows_host<limg_hip_window_job>(c, kVersion1, pStream, streamBytes, pWindows, count, nullptr); }
  limg_hip_result limg_hip_blocked_decode_stream_windows(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_window *pWindows, size_t count)
  { return decode_windows_host<limg_hip_window_job>(c, kVersion2, pStream, streamBytes, pWindows, count, nullptr); }

  // ---- batched, the error against an original instead of the pixels ----
  limg_hip_result limg_hip_decode_stream_windows_error_device(limg_hip_context *c, const limg_hip_error_window_job *pJobs, size_t count, uint64_t *pErrorSums, uint32_t *pJobStatus,
                                                              void *stream)
  { return decode_windows_device(c, kVersion1, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream, pErrorSums); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_error_device(limg_hip_context *c, const limg_hip_error_window_job *pJobs, size_t count, uint64_t *pErrorSums,
                                                                      uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion2, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream, pErrorSums); }
  limg_hip_result limg_hip_decode_stream_windows_error(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_error_window *pWindows, size_t count,
                                                       uint64_t *pErrorSums)
  { return decode_windows_host<limg_hip_error_window_job>(c, kVersion1, pStream, streamBytes, pWindows, count, nullptr, pErrorSums); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_error(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_error_window *pWindows,
                                                               size_t count, uint64_t *pErrorSums)
  { return decode_windows_host<limg_hip_error_window_job>(c, kVersion2, pStream, streamBytes, pWindows, count, nullptr, pErrorSums); }

  // the whole image of a host stream of either version against a host original: limg_hip_compare(original, decode) without the decode
  double limg_hip_stream_compare(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const uint32_t *pOriginal, size_t pixels, double *pMse, double *pMax)
  {
    if (!c || !pStream || !pOriginal || streamBytes < sizeof(limg_hip_stream_header)) return NAN;
    uint32_t version; // (the caller's bytes need no alignment)
    memcpy(&version, pStream + offsetof(limg_hip_stream_header, version), sizeof(version));
    const bool rects = version == LIMG_HIP_STREAM_VERSION_BLOCKED;
    size_t sizeX = 0, sizeY = 0;
    int hasAlpha = 0;
    if ((rects ? limg_hip_blocked_stream_info(pStream, streamBytes, &sizeX, &sizeY, &hasAlpha, nullptr, nullptr)
               : limg_hip_stream_info(pStream, streamBytes, &sizeX, &sizeY, &hasAlpha, nullptr)) != limg_hip_success || sizeX * sizeY != pixels)
      return NAN;
    const limg_hip_error_window whole = { 0, 0, sizeX, sizeY, pOriginal, sizeX };
    uint64_t err = 0;
    if (decode_windows_host<limg_hip_error_window_job>(c, rects ? kVersion2 : kVersion1, pStream, streamBytes, &whole, 1, nullptr, &err) != limg_hip_success) return NAN;
    const double maxError = 255.0 * 255.0 * (hasAlpha ? 12.0 : 9.0), mse = (double)err / (double)pixels; // limg_hip_compare_device's constants
    if (pMse) *pMse = mse;
    if (pMax) *pMax = maxError;
    return 10.0 * log10(maxError / mse);
  }

  // the largest error sum whose PSNR over sizeX x sizeY pixels is still `psnr` dB: PSNR >= psnr <=> errorSum <= this
  uint64_t limg_hip_error_sum_for_psnr(size_t sizeX, size_t sizeY, int hasAlpha, double psnr)
  {
    if (psnr != psnr || sizeX == 0 || sizeY == 0) return 0;
    const double v = floor(255.0 * 255.0 * (hasAlpha ? 12.0 : 9.0) * (double)sizeX * (double)sizeY / pow(10.0, psnr / 10.0));
    return v >= 18446744073709551616.0 ? UINT64_MAX : v > 0.0 ? (uint64_t)v : 0;
  }

  // ---- batched, planar float tensors ----
  limg_hip_result limg_hip_decode_stream_windows_tensor_device(limg_hip_context *c, const limg_hip_tensor_window_job *pJobs, size_t count, const limg_hip_tensor_format *pFormat,
                                                               uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion1, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_tensor_device(limg_hip_context *c, const limg_hip_tensor_window_job *pJobs, size_t count,
                                                                       const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion2, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_decode_stream_windows_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_tensor_window *pWindows, size_t count,
                                                        const limg_hip_tensor_format *pFormat)
  { return decode_windows_host<limg_hip_tensor_window_job>(c, kVersion1, pStream, streamBytes, pWindows, count, pFormat); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_tensor_window *pWindows,
                                                                size_t count, const limg_hip_tensor_format *pFormat)
  { return decode_windows_host<limg_hip_tensor_window_job>(c, kVersion2, pStream, streamBytes, pWindows, count, pFormat); }

  // ---- batched, reduced scale, RGBA8 and tensors: the job types with a level ----
  limg_hip_result limg_hip_decode_stream_windows_scaled_device(limg_hip_context *c, const limg_hip_scaled_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion1, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_device(limg_hip_context *c, const limg_hip_scaled_window_job *pJobs, size_t count, uint32_t *pJobStatus,
                                                                       void *stream)
  { return decode_windows_device(c, kVersion2, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_decode_stream_windows_scaled(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_window *pWindows, size_t count)
  { return decode_windows_host<limg_hip_scaled_window_job>(c, kVersion1, pStream, streamBytes, pWindows, count, nullptr); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_window *pWindows,
                                                                size_t count)
  { return decode_windows_host<limg_hip_scaled_window_job>(c, kVersion2, pStream, streamBytes, pWindows, count, nullptr); }
  limg_hip_result limg_hip_decode_stream_windows_scaled_tensor_device(limg_hip_context *c, const limg_hip_scaled_tensor_window_job *pJobs, size_t count,
                                                                      const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion1, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_tensor_device(limg_hip_context *c, const limg_hip_scaled_tensor_window_job *pJobs, size_t count,
                                                                              const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion2, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_decode_stream_windows_scaled_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_tensor_window *pWindows,
                                                               size_t count, const limg_hip_tensor_format *pFormat)
  { return decode_windows_host<limg_hip_scaled_tensor_window_job>(c, kVersion1, pStream, streamBytes, pWindows, count, pFormat); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes,
                                                                       const limg_hip_scaled_tensor_window *pWindows, size_t count, const limg_hip_tensor_format *pFormat)
  { return decode_windows_host<limg_hip_scaled_tensor_window_job>(c, kVersion2, pStream, streamBytes, pWindows, count, pFormat); }

  // ---- batched, resized, RGBA8 and tensors: the job types with a source rectangle and an output size ----
  limg_hip_result limg_hip_decode_stream_windows_resized_device(limg_hip_context *c, const limg_hip_resized_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion1, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_resized_device(limg_hip_context *c, const limg_hip_resized_window_job *pJobs, size_t count, uint32_t *pJobStatus,
                                                                        void *stream)
  { return decode_windows_device(c, kVersion2, pJobs, count, nullptr, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_decode_stream_windows_resized(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_resized_window *pWindows, size_t count)
  { return decode_windows_host<limg_hip_resized_window_job>(c, kVersion1, pStream, streamBytes, pWindows, count, nullptr); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_resized(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_resized_window *pWindows,
                                                                 size_t count)
  { return decode_windows_host<limg_hip_resized_window_job>(c, kVersion2, pStream, streamBytes, pWindows, count, nullptr); }
  limg_hip_result limg_hip_decode_stream_windows_resized_tensor_device(limg_hip_context *c, const limg_hip_resized_tensor_window_job *pJobs, size_t count,
                                                                       const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion1, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_resized_tensor_device(limg_hip_context *c, const limg_hip_resized_tensor_window_job *pJobs, size_t count,
                                                                               const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream)
  { return decode_windows_device(c, kVersion2, pJobs, count, pFormat, pJobStatus, (hipStream_t)stream); }
  limg_hip_result limg_hip_decode_stream_windows_resized_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, const limg_hip_resized_tensor_window *pWindows,
                                                                size_t count, const limg_hip_tensor_format *pFormat)
  { return decode_windows_host<limg_hip_resized_tensor_window_job>(c, kVersion1, pStream, streamBytes, pWindows, count, pFormat); }
  limg_hip_result limg_hip_blocked_decode_stream_windows_resized_tensor(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes,
                                                                        const limg_hip_resized_tensor_window *pWindows, size_t count, const limg_hip_tensor_format *pFormat)
  { return decode_windows_host<limg_hip_resized_tensor_window_job>(c, kVersion2, pStream, streamBytes, pWindows, count, pFormat); }
}
