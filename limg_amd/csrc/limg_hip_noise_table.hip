// limg_hip_noise_table.hip -- the dither noise table on the device and the chain checkpoints it is filled from; the host-only noise helpers of the C ABI.
#include "limg_hip_context.h"

using namespace limg_hip;

namespace limg_hip
{
  constexpr size_t kNoiseChunk = 1u << 16; // table growth granularity (entries)

  // How far the GPU-filled noise table reaches: the far checkpoints' last value + one far stretch (2^27 calls).
  size_t checkpoint_reach()
  {
    size_t farCount = 0, farEvery = 0;
    (void)noise_checkpoints_far_host(&farCount, &farEvery);
    return farCount * farEvery;
  }

  // Dense chain values (every LIMG_NOISE_CHECKPOINT_EVERY = 1024 calls) number first .. first + count - 1 into pOut: the embedded dense table where it reaches (16 Mi
  // calls), beyond it the embedded FAR values (every 65536 calls) walked on foot -- 65536 calls of 8 AES rounds per far value = 0.5 ms, far values independent of each
  // other: on up to 16 host threads.  false beyond the far table's reach.
  bool dense_checkpoints_host(size_t first, size_t count, uint64_t *pOut)
  {
    size_t ckCount = 0, ckEvery = 0, farCount = 0, farEvery = 0;
    const uint64_t *ck = noise_checkpoints_host(&ckCount, &ckEvery);
    const uint64_t *far = noise_checkpoints_far_host(&farCount, &farEvery);
    const size_t perFar = farEvery / ckEvery;
    if (count == 0) return true;
    if (first + count > farCount * perFar) return false;
    size_t k = 0;
    for (; k < count && first + k < ckCount; k++) pOut[k] = ck[first + k];
    if (k == count) return true;
    const size_t j0 = (first + k) / perFar, j1 = (first + count - 1) / perFar + 1; // far stretches touched
    unsigned threads = std::thread::hardware_concurrency();
    if (threads == 0 || threads > 16) threads = 16;
    if (threads > j1 - j0) threads = (unsigned)(j1 - j0);
    uint64_t scratch[16][64]; // one far stretch's dense values per thread (nothing may throw inside the threads)
    if (perFar > 64) return false;
    auto work = [&](unsigned t) {
      uint64_t *tmp = scratch[t];
      for (size_t j = j0 + t; j < j1; j += threads)
      {
        (void)chain_checkpoints(far[j], farEvery, ckEvery, tmp, false);
        for (size_t q = 0; q < perFar; q++)
        {
          const size_t idx = j * perFar + q;
          if (idx >= first + k && idx < first + count) pOut[idx - first] = tmp[q];
        }
      }
    };
    run_on_threads(threads, work);
    return true;
  }

  // Dense chain checkpoints covering dither calls [0, calls) on the device (c->noise.ck): the embedded table once per context, more when an image reaches beyond it
  // (more than 5.59 M blocks: the missing values come from the far table, dense_checkpoints_host).  Blocking copies: whichever stream fills a noise table later
  // finds them there (an asynchronous copy on the first caller's stream would order nothing for a second stream), and a failed copy leaves no buffer behind that
  // later encodes would trust.  (A buffer that grows is freed first: hipFree waits for the fill kernels that may still read it.)
  limg_hip_result ensure_checkpoints(limg_hip_context *c, size_t calls)
  {
    size_t ckCount = 0, ckEvery = 0;
    const uint64_t *ck = noise_checkpoints_host(&ckCount, &ckEvery);
    size_t need = (calls + ckEvery - 1) / ckEvery;
    if (need < ckCount) need = ckCount;
    if (c->noise.ck.p && need <= c->noise.ckCount) return limg_hip_success;
    if (calls > checkpoint_reach()) return limg_hip_error_InvalidParameter;
    const uint64_t *src = ck;
    if (need > ckCount)
    {
      try
      {
        std::vector<uint64_t> &v = c->noise.ckHost;
        if (v.empty()) v.assign(ck, ck + ckCount);
        const size_t have = v.size();
        if (need > have)
        {
          v.resize(need);
          if (!dense_checkpoints_host(have, need - have, v.data() + have)) { v.resize(have); return limg_hip_error_InvalidParameter; }
        }
        src = v.data();
      }
      catch (...) { c->noise.ckHost.clear(); return limg_hip_error_MemoryAllocationFailure; }
    }
    limg_hip_result r;
    c->noise.ckCount = 0;
    if ((r = c->noise.ck.ensure(need * 8)) != limg_hip_success) return r;
    if (hipMemcpy(c->noise.ck.p, src, need * 8, hipMemcpyHostToDevice) != hipSuccess)
    {
      c->noise.ck.release();
      fprintf(stderr, "limg_hip: upload of the dither chain checkpoints failed\n");
      return limg_hip_error_Generic;
    }
    c->noise.ckCount = need;
    return limg_hip_success;
  }

  limg_hip_result grow_noise_table(limg_hip_context *c, size_t entries, hipStream_t stream)
  {
    const bool pcg = c->opt.dither_pcg != 0;
    if (pcg != c->noise.pcg) c->noise.count = 0;
    if (entries <= c->noise.count) return limg_hip_success;
    const size_t want = ((entries + kNoiseChunk - 1) / kNoiseChunk) * kNoiseChunk;
    if (!pcg && want <= checkpoint_reach() && c->opt.host_noise_table == 0)
    { // the AES stream, on the GPU from the embedded chain checkpoints (limg_hip_noise_gpu.hip): stream-ordered, ~1 ms, nothing crosses PCIe but the 128 KiB of
      // checkpoints, once per context (images of more than 5.59 M blocks: 8 bytes more per 1024 calls beyond the embedded dense table's 16 Mi, made from the far
      // table on host threads -- ~20 ms for the 50 M calls of a 32768^2 image, where walking the whole chain on one host thread and uploading 3.2 GB took 1.5 s).
      // A larger table than the one at hand is filled from scratch (its prefix is the same stream).
      limg_hip_result r;
      if ((r = ensure_checkpoints(c, want)) != limg_hip_success) return r;
      HIP_TRY(hipStreamSynchronize(stream)); // earlier encodes on this stream may still read the table that is about to be replaced
      if ((r = c->noise.table.ensure(want * 64)) != limg_hip_success) return r;
      launch_noise_fill((uint8_t *)c->noise.table.p, (const uint64_t *)c->noise.ck.p, want, stream);
      HIP_TRY(hipGetLastError());
      c->noise.count = want;
      c->noise.pcg = false;
      return limg_hip_success;
    }
    // PCG dither (a test / fallback mode), tables beyond the far checkpoints' reach (2^27 calls: images of more than 44.7 M blocks) or limg_hip_options.host_noise_table:
    // (re)generate on the host; one-time cost per context and image size class
    std::vector<uint8_t> host(want * 64);
    uint64_t h = kDitherSeed;
    h = fill_noise_table(h, host.data(), want, pcg);
    HIP_TRY(hipStreamSynchronize(stream));
    const limg_hip_result r = c->noise.table.ensure(want * 64);
    if (r != limg_hip_success) return r;
    HIP_TRY(hipMemcpy(c->noise.table.p, host.data(), want * 64, hipMemcpyHostToDevice));
    c->noise.count = want;
    c->noise.pcg = pcg;
    c->noise.next = h;
    return limg_hip_success;
  }

  // The chain value the dither call number `calls` of a chain of full 8x8 blocks starts from: the nearest embedded checkpoint, then at most 1023 calls on foot.
  bool chain_value_at(uint64_t calls, uint64_t *pValue)
  {
    size_t ckCount = 0, ckEvery = 0, farCount = 0, farEvery = 0;
    const uint64_t *ck = noise_checkpoints_host(&ckCount, &ckEvery);
    const uint64_t *far = noise_checkpoints_far_host(&farCount, &farEvery);
    uint64_t h, onFoot;
    if (calls / ckEvery < ckCount) { h = ck[calls / ckEvery]; onFoot = calls % ckEvery; }
    else if (calls / farEvery < farCount) { h = far[calls / farEvery]; onFoot = calls % farEvery; } // beyond the dense table: at most 65535 calls on foot (0.5 ms)
    else return false;
    for (uint64_t i = 0; i < onFoot; i++) h = chain_call(h, 64, nullptr, false, false);
    *pValue = h;
    return true;
  }
}

extern "C"
{
  // ---- host-only helpers (no GPU needed; exposed so the host logic can be tested on CPU-only machines) --------------------
  limg_hip_result limg_hip_noise_table_device(limg_hip_context *c, uint8_t *pOutDevice, size_t calls, void *stream)
  {
    if (!c || !pOutDevice) return limg_hip_error_ArgumentNull;
    if (calls > checkpoint_reach() || ((uintptr_t)pOutDevice & 15u) != 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    if ((r = ensure_checkpoints(c, calls)) != limg_hip_success) return r;
    launch_noise_fill(pOutDevice, (const uint64_t *)c->noise.ck.p, calls, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  limg_hip_result limg_hip_host_noise_table(uint8_t *pOut, size_t calls)
  {
    if (!pOut) return limg_hip_error_ArgumentNull;
    fill_noise_table(kDitherSeed, pOut, calls, false);
    return limg_hip_success;
  }

  uint64_t limg_hip_host_chain_call(uint64_t chainValue, size_t pixelCount, uint8_t *pNoise64, int forceSoftwareAes)
  {
    if (pixelCount > 0xFFFFFFFFull) return 0;
    return chain_call(chainValue, (unsigned)pixelCount, pNoise64, (forceSoftwareAes & 1) != 0, (forceSoftwareAes & 2) != 0);
  }

  uint64_t limg_hip_host_chain_checkpoints(size_t calls, size_t every, uint64_t *pOut, int pcg)
  {
    return chain_checkpoints(kDitherSeed, calls, every, pOut, pcg != 0);
  }

  limg_hip_result limg_hip_host_dense_checkpoints(size_t first, size_t count, uint64_t *pOut)
  {
    if (!pOut) return limg_hip_error_ArgumentNull;
    try { return dense_checkpoints_host(first, count, pOut) ? limg_hip_success : limg_hip_error_OutOfBounds; }
    catch (...) { return limg_hip_error_MemoryAllocationFailure; }
  }
}
