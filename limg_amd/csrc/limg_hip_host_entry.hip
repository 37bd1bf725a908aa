// limg_hip_host_entry.hip -- the host-pointer entries of the 8x8 encode (limg_hip_encode3d, limg_hip_encode3d_perf): the caller's image goes up and its planes
// come down through the context's staging buffers; from 4 Mpixels on in row bands, so that the copies hide the kernels.
#include "limg_hip_context.h"

#include <atomic>
#include <condition_variable>

using namespace limg_hip;

namespace
{
  struct Band { size_t y0, y1; }; // rows [y0, y1) of the image

  // from 4 Mpixels on (below, the whole call is a few milliseconds and the bands' launches would not pay), whole blocks, at least 64 block rows, no statistics:
  // the host-pointer entries work in row bands
  bool banded_host_entry(const limg_hip_context *c, size_t sizeX, size_t sizeY)
  {
    return sizeX * sizeY >= ((size_t)4 << 20) && sizeX % kBlock == 0 && sizeY % kBlock == 0 && sizeY >= 64 * kBlock && c->opt.collect_stats == 0;
  }

  // 8 bands of whole block rows (the last one takes the rest) -> their number
  uint32_t even_bands(size_t sizeY, Band *bands)
  {
    const size_t want = 8, rows = ((sizeY / kBlock + want - 1) / want) * kBlock;
    uint32_t nb = 0;
    for (size_t y = 0; y < sizeY; y += rows) { bands[nb].y0 = y; bands[nb].y1 = y + rows < sizeY ? y + rows : sizeY; nb++; }
    return nb;
  }

  // the banded paths' two streams (kernels, copies) and one event per band
  limg_hip_result band_streams(limg_hip_context *c, uint32_t nb)
  {
    hipStream_t s;
    limg_hip_result r;
    if ((r = c->host.stream.get(s)) != limg_hip_success || (r = c->host.copyStream.get(s)) != limg_hip_success) return r;
    return c->host.events.ensure(nb, hipEventDisableTiming);
  }

  // The host-pointer entry in ROW BANDS: what every relinked caller of limg_encode3d_test hits moves 4 B/px up and 35 B/px down over PCIe, and
  // the download alone (2.35 GB for 8192^2) is ~43 ms at wire rate against 1.4 ms of kernels.  Upload, encode and download one after the other: 50.4 ms.  Here the
  // image goes up and is encoded band by band on the calling thread while a second host thread brings every finished band's rows of the 11 planes down (PCIe is full
  // duplex; blocking copies from / to the caller's pageable memory already run at wire rate, so no staging copy is added): the upload and the kernels of band k + 1
  // hide under the download of band k.
  //   * poolThreads == 0 (one dither chain through the image, src/limg.cpp:2110): bands of whole block rows through the two exchange-free halves of the chain entry
  //     -- E step + scan of the band, then its F step from the call count of the bands above it (k_chain_base on the device, stream-ordered, no host round trip);
  //   * poolThreads > 0 (src/limg.cpp:2114-2134): every chain restarts at the seed, so a band is a chain: an independent encode of its rows.
  // Images with partial edge blocks, small images and encodes that collect statistics take the plain path.
  limg_hip_result host_encode_banded(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, void *const *hp, void *const *dp,
                                     uint32_t errorFactor, int poolThreads, int fastBitCrushing)
  {
    const size_t blocksX = sizeX / kBlock;
    const Partition pt = partition(sizeY, poolThreads);
    const bool chains = pt.chainCount > 1 && pt.chainRows != 0;
    Band bands[64];
    uint32_t nb = 0;
    if (chains)
    {
      if (pt.chainCount > 64) return limg_hip_error_InvalidParameter; // (the caller falls back to the plain path)
      for (uint32_t k = 0; k < pt.chainCount; k++)
      {
        bands[nb].y0 = (size_t)k * pt.chainRows * kBlock;
        bands[nb].y1 = k + 1 < pt.chainCount ? (size_t)(k + 1) * pt.chainRows * kBlock : sizeY;
        nb++;
      }
    }
    else nb = even_bands(sizeY, bands);
    limg_hip_result r;
    if ((r = band_streams(c, nb)) != limg_hip_success) return r;
    if ((r = c->host.words.ensure((2 * 64 + 2) * 8)) != limg_hip_success) return r;
    unsigned long long *dCalls = (unsigned long long *)c->host.words.p, *dBase = dCalls + 64;
    hipStream_t s = c->host.stream;
    if ((r = ensure_device_status(c, s)) != limg_hip_success) return r;
    HIP_TRY(hipMemsetAsync(dCalls, 0, 2 * 64 * 8, s));

    // the downloads: a second host thread, band after band, as their events fire
    std::atomic<uint32_t> ready(0);      // bands whose kernels are enqueued and whose event is recorded
    std::atomic<int> failed(0);
    std::mutex m;
    std::condition_variable cv;
    auto download = [&]() {
      if (hipSetDevice(c->device) != hipSuccess) { failed = 1; return; }
      for (uint32_t b = 0; b < nb; b++)
      {
        {
          std::unique_lock<std::mutex> lk(m);
          cv.wait(lk, [&] { return ready.load() > b || failed.load() != 0; });
        }
        if (failed.load() != 0) return;
        if (hipEventSynchronize(c->host.events[b]) != hipSuccess) { failed = 1; return; }
        const size_t o = bands[b].y0 * sizeX, n = (bands[b].y1 - bands[b].y0) * sizeX;
        for (int i = 0; i < 11; i++)
        {
          const size_t es = i < 8 ? 4 : 1;
          // (on a stream of its own: blocking hipMemcpy calls of two threads share the null stream and run one after the other -- measured: every upload waited
          // for the download in front of it)
          if (hipMemcpyAsync((uint8_t *)hp[i] + o * es, (const uint8_t *)dp[i] + o * es, n * es, hipMemcpyDeviceToHost, c->host.copyStream) != hipSuccess) { failed = 1; return; }
        }
        if (hipStreamSynchronize(c->host.copyStream) != hipSuccess) { failed = 1; return; }
      }
    };
    std::thread *copier = nullptr;
    try { copier = new std::thread(download); }
    catch (...) { copier = nullptr; }

    limg_hip_result result = limg_hip_success;
    for (uint32_t b = 0; b < nb && result == limg_hip_success && failed.load() == 0; b++)
    {
      const size_t y0 = bands[b].y0, rows = bands[b].y1 - y0, o = y0 * sizeX;
      const uint32_t *dIn = (const uint32_t *)c->host.in.p + o;
      if (hipMemcpyAsync((void *)dIn, pIn + o, rows * sizeX * 4, hipMemcpyHostToDevice, s) != hipSuccess) { result = limg_hip_error_Generic; break; }
      limg_hip_encode3d_info d = *reinterpret_cast<const limg_hip_encode3d_info *>(dp);
      advance_planes(d, o);
      if (chains) result = encode_device(c, dIn, sizeX, rows, hasAlpha, &d, nullptr, errorFactor, 0, fastBitCrushing, s);
      else
      {
        const size_t before = (y0 / kBlock) * blocksX;
        result = limg_hip_encode3d_chain_device(c, dIn, sizeX, rows, hasAlpha, &d, errorFactor, fastBitCrushing, 1, (uint64_t *)(dCalls + b), nullptr, before, s);
        if (result == limg_hip_success)
        {
          launch_chain_base(dCalls, (int)b, (int)nb, dBase + b, (uint32_t *)c->enc.devStatus.p + 1, s);
          result = limg_hip_encode3d_chain_device(c, dIn, sizeX, rows, hasAlpha, &d, errorFactor, fastBitCrushing, 2, nullptr, (const uint64_t *)(dBase + b), before, s);
        }
      }
      if (result == limg_hip_success && hipEventRecord(c->host.events[b], s) != hipSuccess) result = limg_hip_error_Generic;
      if (result != limg_hip_success) break;
      {
        std::lock_guard<std::mutex> lk(m);
        ready = b + 1;
      }
      cv.notify_all();
      if (!copier)
      { // no second thread to be had: this band comes down here and now (the plain order, band-wise)
        if (hipEventSynchronize(c->host.events[b]) != hipSuccess) { result = limg_hip_error_Generic; break; }
        for (int i = 0; i < 11; i++)
        {
          const size_t es = i < 8 ? 4 : 1;
          if (hipMemcpy((uint8_t *)hp[i] + o * es, (const uint8_t *)dp[i] + o * es, rows * sizeX * es, hipMemcpyDeviceToHost) != hipSuccess) { result = limg_hip_error_Generic; break; }
        }
      }
    }
    if (result != limg_hip_success)
    {
      std::lock_guard<std::mutex> lk(m);
      failed = 1;
    }
    cv.notify_all();
    if (copier) { copier->join(); delete copier; }
    if (result == limg_hip_success && failed.load() != 0) result = limg_hip_error_Generic;
    const limg_hip_result status = limg_hip_check_device_status(c); // (also waits for whatever is still enqueued)
    return result != limg_hip_success ? result : status;
  }

  // Nothing is stored, so nothing depends on the dither chain (src/limg.cpp:2140-2173: fit + search only): the image goes up in row bands on one stream and every
  // band's fit + search runs on a second one as soon as its rows have arrived -- the kernels (1.2 ms for 8192^2) hide under the upload (5 ms)
  limg_hip_result perf_banded(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint32_t errorFactor, int fastBitCrushing)
  {
    Band bands[64];
    const uint32_t nb = even_bands(sizeY, bands);
    limg_hip_result r;
    if ((r = band_streams(c, nb)) != limg_hip_success) return r;
    limg_hip_result result = limg_hip_success;
    for (uint32_t b = 0; b < nb; b++)
    {
      const size_t rows = bands[b].y1 - bands[b].y0, o = bands[b].y0 * sizeX;
      if (hipMemcpyAsync((uint32_t *)c->host.in.p + o, pIn + o, rows * sizeX * 4, hipMemcpyHostToDevice, c->host.copyStream) != hipSuccess ||
          hipEventRecord(c->host.events[b], c->host.copyStream) != hipSuccess || hipStreamWaitEvent(c->host.stream, c->host.events[b], 0) != hipSuccess)
      {
        result = limg_hip_error_Generic;
        break;
      }
      if ((result = encode_device(c, (const uint32_t *)c->host.in.p + o, sizeX, rows, hasAlpha, nullptr, nullptr, errorFactor, 0, fastBitCrushing, c->host.stream)) != limg_hip_success) break;
    }
    const limg_hip_result status = limg_hip_check_device_status(c); // (also waits for whatever is still enqueued: uploads from the caller's pIn among it)
    return result != limg_hip_success ? result : status;
  }
}

extern "C"
{
  limg_hip_result limg_hip_encode3d(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_encode3d_info *pInfo, uint32_t errorFactor,
                                    int poolThreads, int fastBitCrushing)
  {
    if (!c || !pIn || !pInfo) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (sizeX == 0 || sizeY == 0) return limg_hip_error_InvalidParameter;
    void *const *hp = reinterpret_cast<void *const *>(pInfo);
    for (int i = 0; i < 11; i++)
      if (!hp[i]) return limg_hip_error_ArgumentNull;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = sizeX * sizeY;
    limg_hip_result r;
    if ((r = c->host.in.ensure(px * 4)) != limg_hip_success) return r;
    if ((r = c->host.planes.ensure(px * 35 + 11 * 256)) != limg_hip_success) return r;
    limg_hip_encode3d_info d;
    uint8_t *base = (uint8_t *)c->host.planes.p;
    void **dp = reinterpret_cast<void **>(&d);
    size_t off = 0;
    for (int i = 0; i < 11; i++)
    {
      dp[i] = base + off;
      off += (i < 8 ? px * 4 : px);
      off = (off + 255) & ~(size_t)255;
    }
    // (independent chains are the bands: at most 64 of them, at least 8 block rows each)
    const Partition pt = partition(sizeY, poolThreads);
    const bool chains = pt.chainCount > 1 && pt.chainRows != 0;
    if (banded_host_entry(c, sizeX, sizeY) && c->opt.force_split_kernels == 0 && (!chains || (pt.chainCount <= 64 && pt.chainRows >= 8)))
      return host_encode_banded(c, pIn, sizeX, sizeY, hasAlpha, hp, dp, errorFactor, poolThreads, fastBitCrushing);
    HIP_TRY(hipMemcpy(c->host.in.p, pIn, px * 4, hipMemcpyHostToDevice));
    if ((r = encode_device(c, (const uint32_t *)c->host.in.p, sizeX, sizeY, hasAlpha, &d, nullptr, errorFactor, poolThreads, fastBitCrushing, nullptr)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    for (int i = 0; i < 11; i++) HIP_TRY(hipMemcpy(hp[i], dp[i], i < 8 ? px * 4 : px, hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode3d_perf(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint32_t errorFactor, int poolThreads,
                                         int fastBitCrushing)
  {
    if (!c || !pIn) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if (sizeX == 0 || sizeY == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    const size_t px = sizeX * sizeY;
    limg_hip_result r;
    if ((r = c->host.in.ensure(px * 4)) != limg_hip_success) return r;
    if (banded_host_entry(c, sizeX, sizeY))
      return perf_banded(c, pIn, sizeX, sizeY, hasAlpha, errorFactor, fastBitCrushing);
    HIP_TRY(hipMemcpy(c->host.in.p, pIn, px * 4, hipMemcpyHostToDevice));
    if ((r = encode_device(c, (const uint32_t *)c->host.in.p, sizeX, sizeY, hasAlpha, nullptr, nullptr, errorFactor, poolThreads, fastBitCrushing, nullptr)) != limg_hip_success) return r;
    HIP_TRY(hipDeviceSynchronize());
    return limg_hip_success;
  }
}
