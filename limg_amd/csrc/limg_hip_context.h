// Host-only internals of liblimg_hip.so shared by the host translation units (limg_hip_api.hip and the units it was split into): the context and its buffers,
// the error macro, and the helpers more than one unit calls.  The kernel files include limg_hip_internal.h only.  Not part of the C ABI.
#ifndef LIMG_HIP_CONTEXT_H
#define LIMG_HIP_CONTEXT_H

#include "limg_hip_internal.h"
#include "limg_hip_encode_plan.h"
#include "limg_hip_owned.h"
#ifdef LIMG_HIP_TEST_HOOKS
#include "../../include/limg_hip_test_hooks.h"
#define TOPT(c, member) ((c)->topt.member)
#else
#define TOPT(c, member) 0 /* the product has no test hooks: every use folds to the default */
#endif
#include "limg_hip_rccl.h"

#include <stddef.h>
#include <string.h>
#include <new>
#include <mutex>
#include <thread>

struct limg_hip_context
{
  // The reference's entry points are re-entrant (scratch on the stack, src/limg.cpp:1890-1891; the only globals are CPUID flags, src/limg_simd.cpp:57-60), so a
  // caller may encode from several threads at once.  A context owns device scratch, so the blocking host-pointer entries (what the shim's limg_encode3d_test & co.
  // call) serialise on this mutex: any number of threads may share one context through them.  The asynchronous *_device entries enqueue work that uses that
  // scratch after they return: one context per stream there (documented in limg_hip.h).
  std::recursive_mutex hostEntry;
  int device = 0;
  limg_hip_options opt;
#ifdef LIMG_HIP_TEST_HOOKS
  limg_hip_test_options topt; // liblimg_hip_test.so only (include/limg_hip_test_hooks.h)
#endif
  // Every buffer, stream and event below belongs to the member that names it (limg_hip_owned.h) and goes with it: limg_hip_shutdown is `delete`.  The members are
  // grouped by the family of entries that uses them, each family's buffers next to the words that say what they hold.
  typedef std::atomic<size_t> Bytes;
  Bytes deviceBytes{ 0 }; // limg_hip_context_device_bytes: kept by the DevBufs themselves (declared before them, so it outlives them)
  // ---- the 8x8 encode (limg_hip_encode.hip, limg_hip_encode_ragged.hip), compare, profiling ----
  struct Encode
  {
    Bytes &n; // the context's deviceBytes, in every group: what its DevBufs count into
    DevBuf records{ n }, shifts{ n }, stripCalls{ n }, stripBase{ n }; // per-block / per-strip scratch
    DevBuf invN{ n }; // per block 1 / |normal|^2 of the three factors (k_fit_tpb -> E step)
    DevBuf park{ n }; // persistent kernel: 2 x 8 KiB per workgroup
    DevBuf batchTable{ n }; // batched encode: one ImageIO per image
    Stream fitStream; // batched encode in sub-batches: k_fit_tpb of sub-batch k + 1 runs here, next to the persistent kernel of sub-batch k
    Events pipeEvents; // ... and the events that fork it from / join it to the caller's stream
    DevBuf lookback{ n }; // fused path: ticket (16 B) then one 8-byte descriptor per work strip
    DevBuf accTable{ n }; // accurate search: automaton expanded to 32-byte entries (built on the first accurate encode)
    DevBuf devStatus{ n }; // sticky look-back timeout word: never touched by the per-launch memset, cleared by limg_hip_check_device_status
    DevBuf cmp{ n }; // 8-byte accumulator of limg_hip_compare
    int persistentWorkgroups = 1280; // 5 x the device's CU count (set at init): the unit the launches scale (x 6 / 5 with the float stage in its own kernel)
    // optional per-kernel timing (bench): 4 events per encode, recorded on the caller's stream, read back in one go
    bool profiling = false;
    Events events;
    size_t eventsUsed = 0;
  } enc{ deviceBytes };
  // ---- the dither noise (limg_hip_noise_table.hip; dyn, states: limg_hip_encode_ragged.hip) ----
  struct Noise
  {
    Bytes &n;
    DevBuf table{ n }; // static dither noise table (full-block chains)
    bool pcg = false; // which generator the table was built with
    size_t count = 0; // entries generated so far
    uint64_t next = limg_hip::kDitherSeed; // chain value after the last generated entry
    DevBuf dyn{ n }; // data-dependent chains (images with partial blocks)
    DevBuf states{ n }; // ... their per-call chain values + pixel counts as the host uploads them (k_noise_expand -> dyn)
    DevBuf ck{ n }; // the chain checkpoints (limg_noise_checkpoints.h) on the device: the GPU fills the noise table from them
    size_t ckCount = 0; // ... how many dense values (every 1024th call) are there: the embedded ones, or more (ensure_checkpoints)
    std::vector<uint64_t> ckHost; // ... and, once an image has reached beyond the embedded dense values, the host copy they were uploaded from
  } noise{ deviceBytes };
  // ---- limg_hip_options.collect_stats: the reference's 3 + 27 bit counters of the last encode ----
  struct Stats
  {
    Bytes &n;
    DevBuf counters{ n };
    hipStream_t stream = nullptr;
    int state = 0;           // 0 = none, 1 = on the device (8x8 path), 2 = in `host` (merged-block encoder)
    bool accumulate = false; // a batched encode in several launch pairs: the pairs after the first add to the counters instead of restarting them
    uint64_t host[30] = { 0 };
    uint64_t pixels = 0;
  } stats{ deviceBytes };
  // ---- a dither chain shared between GPUs (limg_hip_encode.hip, limg_hip_multi.hip) ----
  struct Chain
  {
    Bytes &n;
    // multi-GPU (RCCL over xGMI): one communicator per context, created by limg_hip_comm_init
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    DevBuf words{ n }; // [0] this rank's value, [1] its chain base, [8 ...] the all-gathered values
    // limg_hip_encode3d_chain_device: phase 2 is only valid right after phase 1 of the same strip (the context holds the intermediate results)
    const void *in = nullptr;
    size_t x = 0, y = 0, before = 0;
    const void *fac[3] = { nullptr, nullptr, nullptr }; // phase 1 left the pre-dither factor bytes in these planes
    int alpha = 0, fast = 0;
    uint32_t ef = 0;
  } chain{ deviceBytes };
  // ---- staging of the host-pointer entry points (limg_hip_host_entry.hip and every family's host forms) and of the ragged paths' host step ----
  struct Host
  {
    Bytes &n;
    DevBuf in{ n }, planes{ n };
    Stream copyStream;   // ... the downloads of the finished bands (second host thread)
    Stream stream;       // ... in row bands: the bands' kernels run here, their events tell the download thread when a band is done
    Events events;
    DevBuf words{ n }; // ... per band its dither-call total and its chain base (one chain through the bands)
    HostBuf stage;       // pinned staging of the ragged paths' host step (shift words down; chain bases and noise up)
    Event stageEvent;    // ... recorded behind the last asynchronous H2D copy that reads it: waited for before it is written, grown or freed again
    bool stageBusy = false;
    Events raggedEvents; // banded ragged encode: "the shift words of band b are down"
  } host{ deviceBytes };
  // ---- the merged-block encoder (limg_hip_blocked_api.hip; the stream packer reads what its last encode left here) ----
  struct Blocked
  {
    Bytes &n;
    DevBuf flags{ n }, bound{ n };
    DevBuf order{ n }; // per batch the order its workgroups take the rectangles in
    DevBuf match{ n }, regions{ n }, out{ n }, px{ n }, fac{ n }, noise{ n }, noiseBase{ n }; // similarity bits, region table / results, scratch (gathered pixels, factor bytes), noise
    DevBuf calls{ n }; // per dither call: chain value, noise offset, pixel count (host walk -> k_noise_expand_calls)
    HostBuf hFlags, hRec, hBits, hDesc, hOut, hNoise, hNoiseBase;
    Stream searchStream; // the worker thread launches its fit + search batches on this stream
    Stream storeStream;  // ... and the noise expansion + store kernels of a batch on a second one
    Stream copyStream;   // copies of the similarity-bit bands, behind the kernels that produce them
    Events workEvents;   // one per batch of the worker that is in flight on the GPU
    Events bandEvents;
    std::vector<limg_hip::HostRegion> lastRegions;
    std::vector<uint32_t> regionPx; // ... and their pixel counts
    size_t lastBlocks = 0;          // blocks of the last encode (what hBits / lastRegions describe)
    double ms[6] = { 0, 0, 0, 0, 0, 0 };
    double kernelMs[4] = { 0, 0, 0, 0 }; // the last encode, HIP events: pass 1 (k_fit_tpb) / the k_blocked_match launches / the k_blocked_fit_search launches /
                                         // the noise-expansion + store launches (the last two summed over the worker's batches)
    Events workTimers; // [4 i .. 4 i + 3]: begin / end of batch slot i's fit + search kernel, begin / end of its expansion + store kernels;
                       // [4 kInFlight ..]: begin of pass 1, end of pass 1 = begin of the similarity kernels, their end
    size_t scratchCap = 0; // plane stride of `fac` in the last encode (BlockedParams::scratchCap)
    struct { size_t sizeX = 0, sizeY = 0; int channels = 0; uint32_t errorFactor = 0, flags = 0; bool valid = false; } last; // ... its shape and stream flags; valid: it succeeded,
                           // so the buffers hold everything the stream packer reads (limg_hip_blocked_last_stream)
  } blocked{ deviceBytes };
  // ---- the stream packers and decoders (limg_hip_stream_api.hip, limg_hip_stream_encode_api.hip, limg_hip_stream_window_api.hip) ----
  struct Streams
  {
    Bytes &n;
    DevBuf fac{ n }, tiles{ n }, units{ n }, status{ n }, buf{ n }; // stream packer: 3 factor planes, per-tile payload words; decode status word; host-entry staging
    DevBuf rateState{ n }, rateCounter{ n }, rateList{ n }; // size probe (limg_hip_rate.hip): RateDevice; the payload-word counter; the list form's error factors, then its sizes
    DevBuf rated{ n }; // batched stream encode with one error factor per image: one RatedImage (32 bytes) per image of a chunk, the threshold table
    DevBuf table{ n }, sizes{ n }; // batched stream encode: one StreamImage per image of the list; the finished streams' sizes side by side (one download)
    DevBuf errorSums{ n }; // stream encode to a quality target: one error sum per image of a round (one download)
    DevBuf listTable{ n }; // stream encode of a list of mixed shapes: a chunk's tables side by side -- per image its view, ListImage, ImageIO, RatedImage, StreamImage, two prefix words
    // version 2 stream of the merged-block encoder: per rectangle its first 64-pixel run, per tile of rectangles its totals; the decoder's block -> rectangle map and
    // its per-call words
    DevBuf bsUnits{ n }, bsTiles{ n }, bsMap{ n }, bsState{ n };
    DevBuf splice{ n }; // stream splice: the call's fail word, its sources, runs and item prefix, and a payload total per run -- nothing that scales with pixels
    HostBuf spliceHost; // ... the table as the call builds it (pinned), copied to `splice` on the call's stream
    Event spliceDone;   // ... recorded behind the call's last kernel, waited for on the host before the next call touches either
    bool spliceBusy = false;
    Events packTimers;      // begin / end of the last stream encode's scan + pack kernels ...
    bool packTimed = false; // ... which limg_hip_blocked_kernel_timing still has to add to blocked.kernelMs[3]
  } stream{ deviceBytes };
  // ---- batched window decode (limg_hip_*decode_stream_windows*): a call's job table -- and, version 2, its map and per-job state words -- lives in one slot of a
  // small ring, so that a call issued before the previous one has run does not disturb it.  host: pinned, the table as the call builds it; dev: its copy, then state
  // and map; done: recorded behind the call's last kernel and waited for on the host before the slot is used again.
  struct WindowSlot { HostBuf host; DevBuf dev; Event done; bool busy = false; WindowSlot(Bytes &n) : dev(n) {} };
  static constexpr unsigned kWindowSlots = 4;
  struct { WindowSlot slots[kWindowSlots]; unsigned next = 0; } window{ { deviceBytes, deviceBytes, deviceBytes, deviceBytes } };

  // limg_hip_shutdown: an idle device and no communicator, then the members release themselves
  ~limg_hip_context()
  {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (chain.comm && limg_hip::rccl().ok) (void)limg_hip::rccl().CommDestroy(chain.comm);
  }
};

namespace limg_hip
{
  // limg_hip_noise.cpp: the dither chain on the host
  uint64_t chain_call(uint64_t h, unsigned n, uint8_t *noise64, bool forceSoft, bool pcg);
  uint64_t fill_noise_table(uint64_t h, uint8_t *noise, size_t count, bool pcg);
  uint64_t chain_checkpoints(uint64_t h, size_t calls, size_t every, uint64_t *pOut, bool pcg);
  void chain_walk_rows(uint64_t &h, size_t &call, uint32_t by0, uint32_t by1, uint32_t blocksX, uint32_t stripsX, size_t sizeX, size_t sizeY, uint32_t chainCount, uint32_t chainRows,
                       const uint32_t *shifts, uint32_t *stripBase, unsigned long long *states, uint8_t *pixels, size_t maxCalls, bool pcg);
  size_t chain_walk_blocks(uint64_t h0, uint32_t blocksX, uint32_t blocksY, uint32_t stripsX, size_t sizeX, size_t sizeY, uint32_t chainCount, uint32_t chainRows, const uint32_t *shifts,
                           uint32_t *stripBase, unsigned long long *states, uint8_t *pixels, size_t maxCalls, bool pcg);

  // ---- noise table (limg_hip_noise_table.hip) ----
  size_t checkpoint_reach();
  bool dense_checkpoints_host(size_t first, size_t count, uint64_t *pOut);
  limg_hip_result ensure_checkpoints(limg_hip_context *c, size_t calls);
  limg_hip_result grow_noise_table(limg_hip_context *c, size_t entries, hipStream_t stream);
  bool chain_value_at(uint64_t calls, uint64_t *pValue);

  // ---- profiling (limg_hip_api.hip) ----
  void mark(limg_hip_context *c, hipStream_t stream);
  // limg_hip_profile_end reads the events in groups of four, so whatever brackets its kernels records a fixed number of them -- its quota (an encode:
  // EncodePlan::marks; a packer or decoder: 4).  mark() records one at each real boundary while the quota lasts; close() records what is left of it where the
  // stream stands.  More than the quota cannot be recorded, and a closed timeline has recorded exactly its quota.
  class Timeline
  {
    limg_hip_context *c;
    hipStream_t stream;
    int left;
  public:
    Timeline(limg_hip_context *c, hipStream_t stream, int quota) : c(c), stream(stream), left(quota) {}
    void mark() { if (left > 0) { left--; limg_hip::mark(c, stream); } }
    void close() { while (left > 0) mark(); }
  };

  // work(0) .. work(n - 1), each on a host thread of its own where the host lets us start one.  A thread that cannot be created (EAGAIN under a pid / thread limit) or a
  // pool that cannot be allocated must neither leave joinable threads behind (their destructor calls std::terminate) nor send an exception across the extern "C"
  // boundary: whatever did not get a thread runs on the calling thread.  `work` itself must not throw.
  template <class F>
  void run_on_threads(unsigned n, F &&work) noexcept
  {
    std::thread *pool = n > 1 ? new (std::nothrow) std::thread[n - 1] : nullptr; // default-constructed: not joinable
    unsigned started = 0;
    if (pool)
      for (; started < n - 1; started++)
      {
        try { pool[started] = std::thread(work, started + 1); }
        catch (...) { break; }
      }
    work(0u);
    for (unsigned t = started + 1; t < n; t++) work(t);
    for (unsigned t = 0; t < started; t++) pool[t].join();
    delete[] pool;
  }

  // |record value| above which a block takes the generic 32-bit trial: EncodeParams::recordLimit and the probes' (see term_bias in limg_hip_search.h: 3 * 2700 + 1 < 0x2000)
  inline int32_t record_limit(const limg_hip_context *c) { return TOPT(c, record_limit) > 0 ? TOPT(c, record_limit) - 1 : 2700; }
  // images of one shape per launch pair (list_chunk, limg_hip_encode_rules.h) with the test build's batch_chunk; blocks, strips: of one image
  inline size_t batch_hook(const limg_hip_context *c) { return TOPT(c, batch_chunk) > 0 ? (size_t)TOPT(c, batch_chunk) : 0; }
  inline size_t list_chunk(const limg_hip_context *c, size_t blocks, size_t strips) { return list_chunk(blocks, strips, batch_hook(c)); }

  // ---- what the stream entries (limg_hip_stream_api.hip: shared parts, header checks, decode, version 2; limg_hip_stream_encode_api.hip: the version 1 encode family)
  // and the window entries (limg_hip_stream_window_api.hip) share; defined in limg_hip_stream_api.hip ----
  int device_cus(const limg_hip_context *c);
  limg_hip_result stream_total_bytes(const uint8_t *dStream, hipStream_t s, size_t *pBytes); // what the packer's scan left in the stream's header; waits for `s`
  limg_hip_result download_stream(limg_hip_context *c, size_t bytes, uint8_t *pStream, size_t capacity, size_t *pBytes); // stream.buf to the caller; *pBytes = bytes even where `capacity` is too small
  // a host-pointer encode: upload, deviceEncode(dIn, dStream, bound, &bytes) on the null stream, status, download.  bound: the version's limg_hip_*stream_bound
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
  limg_hip_result ensure_stream_status(limg_hip_context *c, hipStream_t s); // the decoders' status word, zeroed on `s` when it is first made
  // one RGBA8 window, checked without touching the device, as kernel parameters with the status word set; bound: the version's limg_hip_*stream_bound(sizeX, sizeY)
  limg_hip_result window_params(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t bound, size_t x0, size_t y0, size_t width,
                                size_t height, uint32_t *pOut, size_t outStridePixels, hipStream_t s, WindowDecodeParams &wp);
  // version 2's one decode, the full image's and a window's: wp from window_params
  limg_hip_result blocked_window_decode(limg_hip_context *c, WindowDecodeParams &wp, hipStream_t s);

  // ---- the 8x8 encode (limg_hip_encode.hip, limg_hip_encode_ragged.hip; its decisions: limg_hip_encode_plan.h) ----
  static_assert(kShapeBlock == (size_t)kBlock && kShapeStripBlocks == (size_t)kStripBlocks, "limg_hip_encode_plan.h counts the kernels' blocks and strips");

  // What the public entries add to the plain (single image, whole encode) call.
  struct EncodeExtra
  {
    bool streamRaw = false, fitOnly = false;
    bool fitFloatMode = false;      // fitOnly: the records in the context's float mode, as a stream encode's k_fit_tpb leaves them (the size probe); false: always the
                                    // exact float stage (pass 1 of the merged-block encoder)
    uint32_t *stripWords = nullptr; // stream mode, images of whole blocks: per work strip the payload words of its blocks (EncodeParams::stripWords)
    int chainPhase = 0; // 0 = whole encode; 1 = E step + scan only (writes *dChainCalls); 2 = F step only (reads *dChainBase).  1 and 2 always take the split path.
    unsigned long long *dChainCalls = nullptr;
    const unsigned long long *dChainBase = nullptr;
    size_t chainBlocksBefore = 0;
    // batch (host array of batchCount entries, batchCount > 1): the images of a batched encode -- same shape, whole 8x8 blocks, all 11 planes (or, from the batched
    // stream encode, the three factor planes only: streamRaw, stripWords and both compact outputs set) -- in one launch
    // pair (or, limg_hip_options.batch_sub_images, a pipeline of launch pairs); dIn / dInfo are then those of image 0.  The caller has checked all of that.
    // With fitOnly (no planes at all): k_fit_tpb's one grid over the list, records and invN image after image in the context's scratch -- the budgeted list's probes.
    const ImageIO *batch = nullptr;
    size_t batchCount = 1;
    // errorFactors (host array of batchCount entries, or NULL): image i of a compact-mode stream list at its own error factor -- k_encode_list_rated instead of the
    // persistent kernel, the `errorFactor` argument unused.  Whole blocks, k_fit_tpb's float stage, the default search; anything else is refused.
    // ratedTable: device memory of the caller's for batchCount RatedImage entries, which this call fills from errorFactors on its stream.
    const uint32_t *errorFactors = nullptr;
    RatedImage *ratedTable = nullptr;
    // ---- a sub-image of a larger encode (the two parts of an image whose last block row is partial: encode_height_ragged) ----
    bool inner = false;            // part of a larger encode: no statistics launch of its own, no reset of the context's chain / statistics state
    bool innerLast = false;        // ... its last block row: no profiling event (the rows above record three, the whole call the fourth)
    const Partition *part = nullptr; // the dither-chain partition of the WHOLE image (a sub-image cannot derive it from its own height)
    size_t scratchRow0 = 0;        // this sub-image's first block row in the per-block scratch (and in the caller's compact outputs)
    size_t scratchRows = 0;        // block rows the scratch must hold (0: this call's own)
    const unsigned long long *dPrevDesc = nullptr; // ragged sub-image: its chain continues the one whose dither-call count is the low word of this look-back descriptor
  };

  limg_hip_result encode_device(limg_hip_context *c, const uint32_t *dIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_encode3d_info *dInfo,
                                const limg_hip_compact_out *compact, uint32_t errorFactor, int poolThreads, int fast, hipStream_t stream, const EncodeExtra &x = EncodeExtra());

  // One encode as encode_device has set it up: what every launch path reads.
  struct EncodeJob
  {
    limg_hip_context *c;
    hipStream_t stream;
    const EncodeExtra &x;
    const limg_hip_encode3d_info *dInfo;
    size_t sizeX, sizeY;
    const EncodePlan &plan;
    Timeline tl; // the path marks its real boundaries, encode_device closes it
    EncodeParams p;
    Partition pt;
    int channels;
    size_t blocks, strips; // of all images of the launch
    const RatedImage *rated = nullptr; // x.errorFactors as the device's threshold table: the persistent launches are k_encode_list_rated's
  };
  // images with partial edge blocks (limg_hip_encode_ragged.hip): the split path's kernels around a dither chain the host walks
  limg_hip_result encode_ragged(EncodeJob &e);

  // the sticky status words (look-back timeout, aborted chain: enc.devStatus), zeroed on `stream` when they are first made
  limg_hip_result ensure_device_status(limg_hip_context *c, hipStream_t stream);
  // the persistent kernel's scratch whatever its parameters: `tickets` (>= 2) tickets of 16 bytes, a look-back descriptor per work strip, the status words, the park slots
  struct PersistentScratch { uint32_t *ticket; unsigned long long *desc; uint32_t *timeout; uint8_t *park; };
  limg_hip_result persistent_scratch(limg_hip_context *c, size_t strips, size_t tickets, hipStream_t stream, PersistentScratch &ps);

  // ---- one chunk of a stream-encode list of mixed shapes (limg_hip_list_plan.h) as a route of the 8x8 encode ----
  static_assert(sizeof(RatedListParams) == 160 && sizeof(ListImage) == 64 && sizeof(ImageIO) == 96 && sizeof(RatedImage) == 32 && sizeof(StreamImage) == 32,
                "the entry sizes tests/test_list_plan_cpu.py asks the table layout for");
  inline ChunkTables chunk_tables(size_t n) { return ChunkTables(n, { sizeof(RatedListParams), sizeof(ListImage), sizeof(ImageIO), sizeof(RatedImage), sizeof(StreamImage), 4, 4 }); }
  struct ListChunkImage { const uint32_t *in; size_t sizeX, sizeY; uint32_t errorFactor; uint8_t *fac[3]; }; // whole blocks (list_item_eligible); fac: its three factor planes
  // The n > 1 images through ONE float-stage grid and ONE persistent launch in compact stream mode, image i at its own error factor: records, invN and shift words
  // in the context's per-block scratch (grown by the caller) and the strips' payload words in stripWords, image after image; then the statistics.  hostTables: the host copy of the
  // chunk's table block (chunk_tables(n).bytes, zeroed, the caller's StreamImage entries written): every other part is filled here, ONE upload to devTables.
  // fitOnly (the meaning of EncodeExtra's fitOnly + fitFloatMode for a mixed chunk): the tables and k_fit_tpb_list alone, in the context's float mode -- records and invN
  // image after image from each image's firstBlock, which is what the chunk's size probes read (k_rate_probe_list).  No noise table, no park slots, no statistics; of
  // the tables the views stay zero; images[i].fac and stripWords may be NULL, nothing reads the thresholds of images[i].errorFactor.
  limg_hip_result encode_list_chunk(limg_hip_context *c, const ListChunkImage *images, size_t n, int hasAlpha, int poolThreads, uint32_t *stripWords, uint8_t *hostTables,
                                    uint8_t *devTables, hipStream_t stream, ListChunkTotals &totals, bool fitOnly = false);

  // ---- the merged-block encoder's pipeline (limg_hip_blocked_api.hip) ----
  // pInfo == nullptr is the COMPACT mode of the stream entry: no plane is stored.  When the call returns, every rectangle's descriptor (regions), record and shift word
  // (out), pre-dither factor bytes (fac, region-major, plane stride scratchCap), noise bytes (noise) and noise offset (noiseBase) are complete in the
  // context's `blocked` buffers, which is what the stream packer reads.
  limg_hip_result blocked_encode_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_blocked_encode3d_info *pInfo,
                                        uint32_t errorFactor, int fastBitCrushing, hipStream_t stream);
}

#endif
