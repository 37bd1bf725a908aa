// Internal declarations shared by the host units (limg_hip_context.h and the files that include it) and the kernel files.  Not part of the C ABI.
#ifndef LIMG_HIP_INTERNAL_H
#define LIMG_HIP_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/limg_hip.h"
#include "limg_hip_blocked_host.h"
#include "limg_hip_rate_step.h"
#include "limg_hip_encode_rules.h"
#include "limg_hip_list_plan.h"

namespace limg_hip
{
  constexpr int kBlock = 8;        // limg_MinBlockSize (reference: src/limg_internal.h:158)
  constexpr int kStripBlocks = 32; // image blocks per workgroup ("work strip": 256 x 8 px)
  constexpr int kThreads = 256;     // threads of a work strip's workgroup (limg_hip_kernels.hip)
  constexpr int kWaves = 4;
  constexpr int kBlocksPerWave = 8; // kStripBlocks / kWaves: a wave's blocks in the E step's float stage and the F step
  constexpr uint64_t kDitherSeed = 0xCA7F00D15BADF00DULL; // reference: src/limg.cpp:1893

  // The dither chain partition (reference: src/limg.cpp:2114-2134) in block rows, stated once for the host and the kernels: chain c (< chainCount - 1) owns block
  // rows [c * chainRows, (c + 1) * chainRows), the last chain owns the rest; chainCount <= 1 or chainRows == 0 is one chain.
  __host__ __device__ inline uint32_t chain_of_row(uint32_t chainCount, uint32_t chainRows, uint32_t row)
  {
    if (chainCount <= 1 || chainRows == 0) return 0u;
    const uint32_t c = row / chainRows;
    return c < chainCount - 1 ? c : chainCount - 1;
  }
  // ... and the first block row of the chain that `row` belongs to (its strips' look-back ends there; the row above is no predecessor of its blocks)
  __host__ __device__ inline uint32_t chain_head_row(uint32_t chainCount, uint32_t chainRows, uint32_t row) { return chain_of_row(chainCount, chainRows, row) * chainRows; }

  // The caller's pointers of one image: input pixels and the 11 output planes.  A batched encode (limg_hip_encode3d_batch_device) holds one of these per image
  // in a device table; the kernels read them with scalar loads where they use them.
  struct ImageIO
  {
    const uint32_t *in;
    limg_hip_encode3d_info info;
  };

  // Everything one encode needs on the device.  Passed by value to the kernels.
  struct EncodeParams
  {
    ImageIO io;              // image 0 (the only one of a single-image encode)
    // batched encode: `batchCount` images of the same shape in ONE launch pair; image i = batch[i]; work strip ids, look-back descriptors and the per-block
    // scratch (records, shift words) run image after image (image i owns strips [i * imageStrips, (i + 1) * imageStrips) and block rows [i * blocksY, ...));
    // every image starts its own dither chain(s) (the reference's batch loop calls the encoder once per image: src/main.cpp:278-323)
    const ImageIO *batch;
    uint32_t batchCount, imageStrips;
    uint32_t sizeX, sizeY, blocksX, blocksY, stripsX;
    uint32_t maxPixel32;     // min(maxPixelBitCrushError, 2^32 - 1)
    uint64_t maxBlock;       // maxBlockBitCrushError
    uint32_t blockLimitFull; // min(ceil(maxBlock * 64 / 16), 2^32 - 1): what a full block's error sum is compared with (be * 16 < maxBlock * n)
    int32_t crushBits, fast; // reference: src/limg.cpp:2192-2197
    const uint32_t *accTable; // !fast: the accurate search's automaton, 8 dwords per state (limg_search_table_accurate.h expanded by the context)
    int32_t forced[3];       // -1 or forced shift
    int32_t recordLimit;     // |record value| above which a block takes the generic 32-bit trial (2700: the bound the packed trial's 16-bit terms are proven for; the test build lowers it to exercise the generic path)
    // chain partition (reference: src/limg.cpp:2114-2134), in block rows
    uint32_t chainCount, chainRows; // chain c (< chainCount-1) owns block rows [c*chainRows, (c+1)*chainRows); the last owns the rest
    // per-block scratch / compact outputs
    limg_hip_block_record *records;
    float *invN;           // per block 4 floats: 1 / |normal|^2 of factors A, B, C (src/limg_internal.h:426-452), 0; written by k_fit_tpb next to the record, read by the E step
    uint32_t *shifts;      // per block: sA | sB<<8 | sC<<16 | calls<<24
    uint32_t *stripCalls;  // per work strip: number of dither calls (blocksY * stripsX, raster order)
    uint32_t *stripBase;   // per work strip: index of its first dither call inside its chain (exclusive scan)
    uint32_t *stripWords;  // stream mode (or NULL): per work strip the payload words of its blocks in the compact stream -- what the packer's scan starts from
    // (split path: the pre-dither factor bytes live in the caller's factor planes between the two kernels)
    int32_t storePlanes;   // 0: _perf behaviour
    int32_t fullPlanes;    // 0: compact mode -- only the three factor planes (+ records / shift words) are written
    // dither noise: byte p of call k = low byte of the 16-bit lane the reference ANDs with ditherSize for pixel p
    const uint8_t *noise;
    uint32_t noiseLast;    // index of the table's last entry: call indices are clamped to it (a chain base handed in by the caller, limg_hip_encode3d_chain_device phase 2, cannot make the F step read past the table)
    // fused single-kernel path: per-strip look-back descriptors (status << 32 | value), work ticket, error word
    unsigned long long *desc;
    uint32_t *ticket;   // [0] = next strip id
    int32_t zeroLookback; // k_fit_tpb clears `ticket` (16 bytes) and the descriptors of the strips its waves cover (the persistent launch follows it on the stream)
    uint32_t *timeout;  // sticky: set when a look-back spin gave up; lives outside the per-launch words, cleared only by limg_hip_check_device_status
#ifdef LIMG_HIP_TEST_HOOKS // liblimg_hip_test.so only (include/limg_hip_test_hooks.h): the product's kernels carry none of this
    uint32_t lookbackSpins; // bound of one look-back wait, in polls (the product: kLookbackSpins)
    uint32_t testBaseErrStrip; // test hook: the strip with this id dithers from a chain position that is off by one call (~0: none); its published count stays right
    uint32_t testSkipStrip; // test hook: the strip with this id never publishes its dither-call count (~0: none) -- what a lost predecessor looks like to the look-back
#endif
    uint8_t *park;      // persistent kernel: per workgroup two 8 KiB slots holding a strip's parked results between its E and F steps
    int32_t compactOut; // persistent kernel: also write records / shift words to the raster-order arrays
    int32_t streamRaw;  // compact mode only: factors with shift 8 store their raw byte instead of 0 (input of the stream packer)
    int32_t fitOnly;    // split path: stop after the records (pass 1 of the merged-block encoder, src/limg.cpp:1088-1119)
    // cross-GPU single dither chain (split path only): the scan writes this image strip's dither-call total; the F step adds the strip's first call index
    unsigned long long *chainCallsOut;
    const unsigned long long *chainBase;
    int32_t fitPrio;    // k_fit_tpb: wave priority (s_setprio 0..3); raised when it runs next to a persistent kernel (batched encode as a pipeline)
    int32_t prefit;     // host dispatch only: p.records already hold the fit (k_fit_tpb ran first)
    int32_t floatFast;  // host dispatch only: FAST float stage (limg_hip_options.float_mode = 1)
    int32_t vecIn;      // rows of pIn may be read 16 bytes per lane (sizeX % 4 == 0 and pIn 16-byte aligned); otherwise dword loads
    int32_t vecPlanes;  // the seven block-uniform uint32 planes may be stored 16 bytes per lane (sizeX % 4 == 0 and all seven 16-byte aligned)
    int32_t vecFactors; // the three factor planes may be accessed 16 bytes per lane (sizeX % 16 == 0 and all three 16-byte aligned)
    int32_t vecFactors8; // ... 8 bytes per lane (sizeX % 8 == 0 and all three 8-byte aligned)
    int32_t vecDecoded; // pDecoded may be stored 16 bytes per lane (sizeX % 4 == 0 and 16-byte aligned)
  };

  // ---- a list whose images each carry their own error factor (limg_hip_encode_stream_batch_ef*, k_encode_list_rated) ----
  // Image i's bit-crush thresholds and flags (thresholds(), limg_hip_encode_rules.h) and the error factor its stream's header carries: an entry of a device table
  // next to the ImageIO table, read once per work strip with scalar loads.  The members carry EncodeParams' names: fit_search_strip takes its limits from `lim`,
  // which is the parameter block itself in every other kernel.
  struct RatedImage
  {
    uint32_t maxPixel32, blockLimitFull;
    uint64_t maxBlock;
    int32_t crushBits;
    uint32_t errorFactor;
    uint32_t pad[2];
  };
  static_assert(sizeof(RatedImage) == 32, "one entry of the threshold table");

  // k_encode_list_rated's arguments: the persistent kernel's loop over a list in compact stream mode (float stage by k_fit_tpb, default search), the thresholds per
  // image.  What the shared stages read carries EncodeParams' names; what that mode fixes is a constant here, and so are the look-back's test hooks: the kernarg
  // segment is the same in both builds (as RateProbeParams), and the test build's record_limit travels in recordLimit.
  struct RatedListParams
  {
    const ImageIO *batch;      // one entry per image of THIS launch (a sub-batch's slice of the list's table)
    const RatedImage *rated;   // ... and its thresholds, offset alike
    uint32_t batchCount, imageStrips;
    uint32_t sizeX, sizeY, blocksX, blocksY, stripsX;
    int32_t forced[3];
    int32_t recordLimit;
    uint32_t chainCount, chainRows;
    limg_hip_block_record *records;
    float *invN;
    uint32_t *shifts;
    uint32_t *stripWords;
    const uint8_t *noise;
    uint32_t noiseLast;
    int32_t vecIn, vecFactors, vecFactors8;
    unsigned long long *desc;
    uint32_t *ticket;
    uint32_t *timeout;
    uint8_t *park;
    // compact stream mode, whole blocks, one dither chain partition per image, nothing of the split path or of a chain shared between GPUs
    static constexpr int32_t storePlanes = 1, fullPlanes = 0, compactOut = 1, streamRaw = 1, fitOnly = 0, vecPlanes = 0, vecDecoded = 0;
    static constexpr uint32_t *stripCalls = nullptr, *stripBase = nullptr;
    static constexpr const unsigned long long *chainBase = nullptr;
    static constexpr const uint32_t *accTable = nullptr;
#ifdef LIMG_HIP_TEST_HOOKS // the three look-back hooks do not reach this kernel (include/limg_hip_test_hooks.h): the product's values
    static constexpr uint32_t lookbackSpins = 1u << 22, testBaseErrStrip = ~0u, testSkipStrip = ~0u;
#endif
  };

  // ---- a list whose images differ in SHAPE (limg_hip_encode_stream_list*; the layout: limg_hip_list_plan.h) ----
  // One chunk's images are concatenated: strip ids, look-back descriptors and payload words run through all of them, records / invN / shift words image after
  // image from each image's firstBlock.  Four device tables share the image index: ListImage (geometry and slice starts), ImageIO, RatedImage and -- the persistent
  // kernel's -- one RatedListParams per image, the VIEW its stages read in place of the kernel arguments: that image's geometry, flags and chain partition, and
  // records / invN / shifts already offset to its first block (so the stages' rowBase is 0); desc, stripWords, noise and timeout are the launch's own in every view.
  struct StreamImage;
  static_assert(sizeof(RatedListParams) == 160 && sizeof(ImageIO) == 96, "the per-image table entries include/limg_hip.h states");
  // k_fit_tpb_list's arguments: no hook member, the kernarg segment is the same in both builds.
  struct FitListParams
  {
    const ListImage *images;
    const ImageIO *batch;
    const uint32_t *firstUnit; // nImages: exclusive prefix of the images' float-stage units
    uint32_t nImages, nUnits;
    limg_hip_block_record *records;
    float *invN;
    unsigned long long *desc;  // the persistent launch's look-back descriptors and ticket, which this grid clears on its way (as EncodeParams::zeroLookback)
    uint32_t *ticket;
  };
  // k_encode_list_mixed's arguments
  struct MixedListParams
  {
    const RatedListParams *views; // per image
    const ImageIO *batch;
    const RatedImage *rated;
    const uint32_t *firstStrip;   // nImages: exclusive prefix of the images' work strips
    uint32_t nImages, nStrips;
    uint32_t *ticket;
    uint8_t *park;
  };
  // the list's scan + pack (limg_hip_stream.hip)
  struct StreamListParams
  {
    const ListImage *images;
    const StreamImage *streams;   // per image: its three factor planes and its stream
    const RatedImage *rated;      // ... and the error factor its header carries
    const uint32_t *firstStrip;
    uint32_t nImages, nStrips, nWaves, channels, flags;
    const limg_hip_block_record *records;
    const uint32_t *shifts;
    uint32_t *stripWords;
  };

  // stream pack (limg_hip_stream.hip): from the compact outputs of an encode (factor planes, records, shift words)
  struct StreamParams
  {
    uint32_t sizeX, sizeY, blocksX, blocksY, nBlocks, nTiles, channels, errorFactor, flags;
    const uint8_t *fac[3];
    const limg_hip_block_record *records;
    const uint32_t *shifts;
    uint8_t *stream;
    uint32_t *tileBase; // three-kernel form (widths that are not whole blocks): per tile of 256 blocks payload words, then (after the scan) the tile's first payload word
    // strip form (widths in whole blocks): the encode kernel leaves every work strip's payload words (EncodeParams::stripWords); k_stream_scan_strips turns them into
    // the strips' first payload words in place and writes the header; k_stream_pack_strips packs one strip (<= 32 consecutive blocks of one block row) per wave step
    uint32_t *stripWords;
    uint32_t stripsX, nStrips, nWaves;
  };

  // batched stream pack (limg_hip_stream.hip): a chunk of `nImages` images of one shape, all of whole blocks, behind ONE compact-mode batched encode.  Records, shift
  // words and the strips' payload words run image after image (image i owns strips [i * imageStrips, (i + 1) * imageStrips)); what differs per image -- its three
  // factor planes (slices of the context's streamFac) and its stream -- is an entry of a device table, read with scalar loads where a strip uses it.
  struct StreamImage
  {
    const uint8_t *fac[3];
    uint8_t *stream;
  };
  struct StreamBatchParams
  {
    uint32_t sizeX, sizeY, blocksX, blocksY, nBlocks /* of one image */, channels, errorFactor, flags;
    uint32_t stripsX, imageStrips, nImages, nStrips /* of all images */, nWaves;
    const StreamImage *images;
    const limg_hip_block_record *records;
    const uint32_t *shifts;
    uint32_t *stripWords;
    const RatedImage *rated; // NULL: every header carries errorFactor; else image i's carries rated[i].errorFactor (a list with one error factor per image)
  };

  struct DecodeParams
  {
    uint32_t sizeX, sizeY, blocksX, blocksY, nBlocks;
    const uint8_t *stream;
    unsigned long long streamBytes;
    uint32_t *out;
    uint32_t *status; // bit 0: header mismatch, bit 1: inconsistent payload offsets
    uint32_t *sink;   // 2 KiB nobody reads: where lanes whose block row is not (wholly) inside the image send their two 16-byte stores, so that EVERY lane of EVERY group issues
                      // exactly two stores and the wait for the next payload run can be counted (s_waitcnt vmcnt(2)) instead of draining the stores (vmcnt(0)); see k_stream_decode
  };

  const uint64_t *noise_checkpoints_host(size_t *pCount, size_t *pEvery);
  const uint64_t *noise_checkpoints_far_host(size_t *pCount, size_t *pEvery);
  void launch_noise_fill(uint8_t *noise, const uint64_t *dCheckpoints, size_t count, hipStream_t s);
  void launch_noise_expand(uint8_t *noise, const unsigned long long *dStates, const uint8_t *dPixels, size_t calls, bool pcg, hipStream_t s);
  void launch_noise_expand_calls(uint8_t *noise, const unsigned long long *dStates, const unsigned long long *dOffsets, const uint32_t *dPixels, size_t calls, bool pcg, hipStream_t s);
  void launch_set_batch_table(ImageIO *dTable, const ImageIO *hTable, size_t count, hipStream_t s);
  // f(std::bool_constant<flag>()...): run-time flags as the template arguments of a kernel, so that a launcher names its kernel once and every combination of
  // the flags is instantiated
  template <class F> void with_flags(F &&f) { f(); }
  template <class F, class... Flags> void with_flags(F &&f, bool flag, Flags... rest)
  {
    if (!flag) with_flags([&](auto... b) { f(std::false_type(), b...); }, rest...);
    else with_flags([&](auto... b) { f(std::true_type(), b...); }, rest...);
  }

  void launch_fit_tpb(const EncodeParams &p, int channels, hipStream_t s);
  void launch_fit_search(const EncodeParams &p, int channels, hipStream_t s);
  void launch_encode_persistent(const EncodeParams &p, int channels, int workgroups, hipStream_t s);
  void launch_encode_list_rated(const RatedListParams &p, int channels, bool floatFast, int workgroups, hipStream_t s);
  void launch_fit_tpb_list(const FitListParams &p, int channels, bool floatFast, bool direct, hipStream_t s);
  void launch_encode_list_mixed(const MixedListParams &p, int channels, bool floatFast, int workgroups, hipStream_t s);
  void launch_stream_pack_list(const StreamListParams &b, hipStream_t s);                  // one scan launch + one pack launch, whatever the shapes are
  void launch_set_words(void *dDst, const void *hSrc, size_t bytes, hipStream_t s);          // hSrc: HOST memory (may die when the call returns), through kernel arguments; bytes % 4 == 0
  void launch_set_rated_table(RatedImage *dTable, const uint32_t *hErrorFactors, size_t count, hipStream_t s); // hErrorFactors: HOST array (may die when the call returns), 64 per launch
  void launch_strip_scan(const EncodeParams &p, hipStream_t s);
  void launch_dither_store(const EncodeParams &p, int channels, hipStream_t s);
  void launch_shift_stats(const uint32_t *dShifts, uint32_t blocksX, uint32_t blocksY, uint32_t rows, uint32_t sizeX, uint32_t sizeY, unsigned long long *dOut30, hipStream_t s);
  void launch_chain_base(const unsigned long long *dCalls, int rank, int world, unsigned long long *dBase, uint32_t *dAborted, hipStream_t s);

  // ---- merged-block encoder (limg_hip_blocked.hip; reference: limg_blocked_encode3d_test, src/limg.cpp:1774-1885, :2329-2453) ----
  // (the similarity window kMatch* and the host stages: limg_hip_blocked_host.h)
  struct RegionDesc // one rectangle of 8x8 blocks, in creation (= block index = dither chain) order
  {
    uint32_t ox, oy, rx, ry; // blocks
    uint32_t keep;           // 1: single block that keeps its pass-1 fit (src/limg.cpp:1863-1881)
    uint32_t scratch;        // first element of this region in the scratch arrays (multiple of 4)
    uint32_t pad[2];
  };
  struct RegionOut
  {
    limg_hip_block_record rec;
    uint32_t shiftWord; // sA | sB << 8 | sC << 16 | ditherCalls << 24
    uint32_t pad[3];
  };
  struct BlockedParams
  {
    const uint32_t *in;
    uint32_t sizeX, sizeY, blocksX, blocksY, channels;
    uint32_t maxPixel32;
    uint64_t maxBlock;
    int32_t crushBits, fast, forced[3];
    const limg_hip_block_record *pass1;
    unsigned long long *matchBits; // [blocks][kMatchWords]
    uint32_t seedBase, seedCount;  // k_blocked_match: the seeds of this launch (a band of block rows)
    uint8_t *matchFlags;           // per seed: bit 0 = its 3x3 neighbourhood (right / down) matches entirely, bit 1 = its right or its lower neighbour matches
    float *matchBound;             // per block, 4 floats (k_blocked_bounds): the coefficients of an upper bound of the predicate's 27-colour average; nullptr = not used
    const RegionDesc *regions; // of this launch (a batch of consecutive rectangles)
    uint32_t nRegions;
    uint32_t regionBase;       // index of regions[0] in creation order (block index = regionBase + r + 1)
    RegionOut *out;
    int32_t vecStore;          // k_blocked_store: 4 pixels per lane, 16-byte plane stores (image of whole blocks, sizeX % 4 == 0, every plane suitably aligned)
    uint32_t *order;           // per launch (or NULL): the rectangle each workgroup takes -- large ones first (k_blocked_order)
    uint32_t *scratchPx; // gathered pixels, region-major (src/limg.cpp:1747-1748)
    uint8_t *scratchFac; // 3 planes of scratchCap bytes: pre-dither factor bytes
    uint32_t scratchCap;
    const uint8_t *noise;              // one byte per pixel per dither call, region after region in chain order
    const unsigned long long *noiseBase; // per region: offset of its first call's bytes
    limg_hip_blocked_encode3d_info info;
  };

  void launch_blocked_bounds(const BlockedParams &p, hipStream_t s);
  void launch_blocked_match(const BlockedParams &p, hipStream_t s);
  void launch_blocked_fit_search(const BlockedParams &p, hipStream_t s);
  void launch_blocked_store(const BlockedParams &p, hipStream_t s);
  void launch_blocked_order(const BlockedParams &p, hipStream_t s);

  // ---- version 2 stream: the merged-block encoder's rectangles (limg_hip_blocked_stream.hip; its decode, whole images included: the window decode below) ----
  // Pack: from what a compact-mode merged-block encode leaves in the context (see blocked_encode_device).  The work unit is a RUN: 64 consecutive pixels (rectangle
  // row-major order) of one rectangle, all three fields.
  struct BlockedStreamParams
  {
    uint32_t sizeX, sizeY, blocksX, blocksY, channels, errorFactor, flags;
    uint32_t nRegions, nTiles, scratchCap;
    const RegionDesc *regions;
    const RegionOut *out;
    const unsigned long long *noiseBase;
    const uint8_t *scratchFac, *noise;
    uint8_t *stream;
    uint32_t *units; // nRegions + 1: every rectangle's first run (exclusive prefix of ceil(n / 64)); [nRegions] = all runs
    uint32_t *tiles; // per tile of 256 rectangles { payload words, runs }: totals, then (k_stream_tile_scan<2>) their exclusive prefix
  };
  // (cus: the device's compute units, as the context knows them -- limg_hip_context::persistentWorkgroups / 5; the persistent launches size themselves by it)
  void launch_blocked_stream_pack(const BlockedStreamParams &p, int cus, hipStream_t s);

  // ---- window decode, both versions (limg_hip_stream_window.hip): a pixel rectangle of the image into a caller's stride ----
  struct WindowDecodeParams
  {
    uint32_t sizeX, sizeY, blocksX, blocksY, nBlocks; // the image (what the header is checked against)
    const uint8_t *stream;
    unsigned long long streamBytes;
    uint32_t x0, y0, width, height; // the window, pixels: inside the image, not empty
    uint32_t bx0, by0, wbx, wby;    // ... and its block range: blocks bx0 .. bx0 + wbx - 1 of block rows by0 .. by0 + wby - 1
    uint32_t *out;                  // pixel (x0 + c, y0 + r) at out[r * outStride + c]
    unsigned long long outStride;
    uint32_t vecOut;                // a block row piece that lies wholly inside the window may leave as two 16-byte stores (out 16-byte aligned, outStride % 4 == 0, x0 % 4 == 0)
    uint32_t log2Scale;             // the *_scaled entries (0 everywhere else; it lies in what was padding, so the struct's layout is what it was): level L.  x0 .. wby above then
                                    // describe the job's SOURCE FOOTPRINT, multiples of k = 1 << L; the output window is (x0 >> L, y0 >> L, width >> L, height >> L), whose pixel
                                    // (x0 >> L, y0 >> L) goes to out[0]; vecOut is stated on x0 >> L
    uint32_t *map;                  // version 2: per block of the window the rectangle that covers it (~0: none yet)
    uint32_t *status;               // the context's sticky stream status word, bits as in DecodeParams
    uint32_t *state;                // version 2: this call's words (zeroed in front of it): [0] window blocks claimed, [1] non-0 = the stream is refused
    // planar float output (the *_windows_tensor entries): `out` is then float / _Float16, element (c, r, col) at out[c * planeStride + r * outStride + col], and vecOut
    // says that a piece wholly inside the window may leave as 16-byte stores per plane (out 16-byte aligned; outStride, planeStride and x0 multiples of 16 / element size)
    unsigned long long planeStride;
  };
  void launch_stream_window_decode(const WindowDecodeParams &p, int cus, hipStream_t s);
  void launch_blocked_stream_window_decode(const WindowDecodeParams &p, int cus, hipStream_t s);

  // ---- batched window decode (limg_hip_stream_window.hip): many windows of many streams per launch ----
  // Jobs of one call that name the same stream (pointer, bytes, image size) form a GROUP: version 2 scans a group's rectangle table once and offers every
  // rectangle to every window of the group.
  struct WindowGroup
  {
    uint32_t sizeX, sizeY, blocksX, blocksY, nBlocks;
    uint32_t firstJob, nJobs; // its jobs: groupJobs[firstJob .. firstJob + nJobs - 1]
    uint32_t pad;
    const uint8_t *stream;
    unsigned long long streamBytes;
  };
  // The job table of one call, in device memory.  jobs[i]: what the single-window entry would have launched job i with, except that `map` is the job's slice of the
  // call's concatenated map, `state` the job's own [claimed, refused] pair and `status` the context's sticky word.
  struct WindowBatchParams
  {
    const WindowDecodeParams *jobs;
    const uint32_t *unitBase; // count + 1: exclusive prefix of the jobs' decode units (version 1: runs of up to 64 blocks; version 2: of 8); [count] = totalUnits
    uint32_t count, totalUnits;
    uint32_t *status;         // the context's sticky stream status word
    uint32_t *jobStatus;      // per job (may be NULL): 0 = decoded, else its status bits; zeroed in front of the launch
    // version 2
    const WindowGroup *groups;
    const uint32_t *groupJobs;   // job indices, group after group
    const uint32_t *groupItemBase; // nGroups + 1: exclusive prefix of ceil(nBlocks / 64), the map kernel's work items (64 rectangles each; R <= nBlocks)
    uint32_t nGroups, totalItems;
    // the error entries (NULL everywhere else): per job the sum of the per-pixel colour error over its window, device memory, zeroed in front of the launch; the jobs'
    // `out` / outStride / vecOut then describe the ORIGINAL the window is compared with, which is only read
    unsigned long long *errorSums;
  };
  // f: NULL for packed RGBA8, else the planar float format of the launch (the same job table with planeStride set and out / outStride / vecOut in elements of f's
  // type); scaled: the *_scaled entries' kernels, which honour every job's log2Scale -- a plain job table never goes to them
  void launch_stream_windows(const WindowBatchParams &b, bool scaled, const limg_hip_tensor_format *f, int cus, hipStream_t s);
  void launch_blocked_stream_windows(const WindowBatchParams &b, bool scaled, const limg_hip_tensor_format *f, int cus, hipStream_t s);
  void launch_stream_windows_error(const WindowBatchParams &b, int cus, hipStream_t s);
  void launch_blocked_stream_windows_error(const WindowBatchParams &b, int cus, hipStream_t s);
  static_assert(sizeof(WindowDecodeParams) == 128, "the job table's entry: log2Scale must not grow it");

  // ---- resized window decode (the *_resized entries): any source rectangle to any output size, bilinear on the level-L image (contract: include/limg_hip.h) ----
  // The work item is an output TILE of a job: one workgroup decodes the tile's level-L footprint into an LDS tile and resamples from it.  jobs[i] of the batch table
  // describes, as for a scaled job, the job's SOURCE FOOTPRINT at level L (the level pixels [lo, hi] of both axes times k, log2Scale = L; `out`, outStride and
  // planeStride are the output's); what does not fit into that entry is the job's ResizeJob in a second table of the same ring slot.
  constexpr uint32_t kResizeTilePixels = 4096; // capacity of the LDS tile in level-L pixels (16 KiB; DESIGN.md 4c says why)
  constexpr uint32_t kResizeTileEdge = 64;     // a tile is at most 64 output columns (one per lane of a wave) and 64 output rows
  struct ResizeJob
  {
    uint32_t outW, outH;         // the output's size
    uint32_t x0, y0, srcW, srcH; // the source rectangle, full-resolution pixels
    uint32_t flags;              // LIMG_HIP_RESIZE_FLIP_X
    uint32_t tileW, tileH;       // a tile's output size (the last tile of a row / column may be smaller); its level-L footprint holds at most kResizeTilePixels
    uint32_t tilesX;             // tiles per row of tiles
    uint32_t stepR, pad0;        // four output rows further the y axis' numerator is (srcH << 18) larger: that step's remainder and quotient by outH, so a lane
    unsigned long long stepQ;    // that walks down its rows divides once
    uint32_t pad[2];
  };
  static_assert(sizeof(ResizeJob) == 64, "the second per-job table's entry");
  struct WindowResizeParams
  {
    WindowBatchParams b;
    const ResizeJob *resize;  // count entries
    const uint32_t *tileBase; // count + 1: exclusive prefix of the jobs' tile counts; [count] = totalTiles
    uint32_t totalTiles;
  };
  // One axis of the contract's formula: output index X (already mirrored where the job flips) of `out` -> taps a, b (level-L pixels, clamped to [lo, hi]) and the
  // weight f = 0 .. 256 of b.  num / out is the only division; the kernel takes it once per lane and steps the quotient (resize_axis_q + resize_taps).
  struct ResizeTaps { uint32_t a, b, f; };
  __host__ __device__ inline ResizeTaps resize_taps(unsigned long long c16, uint32_t L, uint32_t lo, uint32_t hi)
  {
    const long long u16 = (long long)(c16 >> L) - 32768;
    const long long i0 = u16 >> 16, l = (long long)lo, h = (long long)hi;
    ResizeTaps t;
    t.f = (uint32_t)(((u16 & 0xFFFF) + 128) >> 8);
    t.a = (uint32_t)(i0 < l ? l : i0 > h ? h : i0);
    t.b = (uint32_t)(i0 + 1 < l ? l : i0 + 1 > h ? h : i0 + 1);
    return t;
  }
  __host__ __device__ inline ResizeTaps resize_axis(uint32_t X, uint32_t s0, uint32_t len, uint32_t out, uint32_t L, uint32_t lo, uint32_t hi)
  {
    return resize_taps(((unsigned long long)s0 << 16) + ((((unsigned long long)(2u * X + 1u) * len) << 15) / out), L, lo, hi);
  }
  // the level pixels an axis of a job may touch: lo = s0 >> L, hi = min((s0 + len - 1) >> L, R - 1) with R the level image's size (the caller has checked lo <= R - 1)
  __host__ __device__ inline uint32_t resize_hi(uint32_t s0, uint32_t len, uint32_t L, uint32_t size)
  {
    const uint32_t e = (s0 + len - 1u) >> L, r = (size >> L) - 1u;
    return e < r ? e : r;
  }
  // v1 / v2 launch: f NULL = packed RGBA8
  void launch_stream_windows_resized(const WindowResizeParams &r, const limg_hip_tensor_format *f, int cus, hipStream_t s);
  void launch_blocked_stream_windows_resized(const WindowResizeParams &r, const limg_hip_tensor_format *f, int cus, hipStream_t s);

  void launch_stream_pack(const StreamParams &p, hipStream_t s);
  void launch_stream_pack_batch(const StreamBatchParams &b, hipStream_t s);                                                  // one scan launch + one pack launch, whatever nImages is
  void launch_set_stream_table(StreamImage *dTable, const StreamImage *hTable, size_t count, hipStream_t s);                // as launch_set_batch_table: through kernel arguments
  void launch_stream_gather_bytes(const StreamImage *dTable, size_t count, unsigned long long *dBytes, hipStream_t s);      // dBytes[i] = totalBytes of image i's header
  void launch_stream_decode(const DecodeParams &p, int cus, hipStream_t s);
  // k_stream_tile_scan<1> alone: the exclusive prefix of `n` payload-word totals in place (any n: it loops beyond 1024), and the version 1 header of that geometry
  void launch_stream_scan(uint32_t *totals, uint32_t n, uint8_t *stream, uint32_t sizeX, uint32_t sizeY, uint32_t channels, uint32_t errorFactor, uint32_t flags, hipStream_t s);

  // ---- stream splice (limg_hip_stream_splice.hip): a version 1 stream from rectangles of blocks of version 1 streams, copied, never decoded ----
  struct SpliceRun; // limg_hip_splice_plan.h: one block row of one piece
  struct SpliceSource // a piece's stream and the geometry its header is checked against (the members stream_header_ok reads)
  {
    const uint8_t *stream;
    unsigned long long streamBytes;
    uint32_t sizeX, sizeY, blocksX, blocksY, nBlocks, reserved[3];
  };
  struct SpliceParams
  {
    const SpliceSource *sources;  // per piece
    const SpliceRun *runs;        // nRuns, in the output's raster order
    const uint32_t *itemBase;     // nRuns + 1: exclusive prefix of the runs' copy items (kSpliceItemBlocks blocks each)
    uint32_t *totals;             // nRuns + 1, zero: a run's payload words (k_splice_measure), then their exclusive prefix (the scan)
    uint32_t *fail;               // the call's own verdict word, zero: a source was refused and nothing is copied
    uint32_t *status;             // the context's sticky word (limg_hip_check_device_status)
    uint8_t *out;
    uint32_t nRuns, nItems;
    uint32_t sizeX, sizeY, blocksX, blocksY, nBlocks, channels, errorFactor, flags; // the output's header
  };
  void launch_stream_splice(const SpliceParams &p, int cus, hipStream_t s); // three launches whatever the pieces are: measure, scan + header, copy

  // ---- the stream's size probe (limg_hip_rate.hip) ----
  // What the probes of one call read on the device and the step kernel between them writes: the search (limg_hip_rate_step.h) or the position in a list of error
  // factors, and the thresholds of the error factor being measured.
  struct RateDevice
  {
    RateState search;
    uint32_t listNext;       // list form: the entry the next step kernel fills
    uint32_t maxPixel32, blockLimitFull, crushBits; // as EncodeParams
    uint64_t maxBlock;
  };
  // k_rate_probe's arguments: the same in both builds (no test-hook member; the test build's record_limit travels in recordLimit, as in EncodeParams).  The members the
  // E step's stages read carry EncodeParams' names.
  struct RateProbeParams
  {
    struct { const uint32_t *in; } io;
    uint32_t sizeX, sizeY, blocksX, blocksY, stripsX;
    int32_t vecIn;
    int32_t recordLimit;
    int32_t forced[3];
    const limg_hip_block_record *records; // k_fit_tpb's
    const float *invN;
    const RateDevice *state;
    unsigned long long *counter;          // the payload words of the error factor being measured, summed over the strips
  };
  void launch_rate_begin(RateDevice *dState, unsigned long long *dCounter, const RateState &first, uint32_t firstErrorFactor, hipStream_t s);
  // fixedBytes: header + table.  dList == nullptr: the search; else the list form (dListBytes[i] = the size at dList[i])
  void launch_rate_step(RateDevice *dState, unsigned long long *dCounter, uint64_t fixedBytes, const uint32_t *dList, unsigned long long *dListBytes, uint32_t listCount,
                        hipStream_t s);
  void launch_rate_probe(const RateProbeParams &p, int channels, bool floatFast, hipStream_t s);
  // The list form (limg_hip_encode_stream_budget_batch*): `nImages` images of one shape, each on a search of its own.  states[i] / counters[i] are image i's; the
  // records and invN of k_fit_tpb's batched grid run image after image (image i owns block rows [i * blocksY, (i + 1) * blocksY)); image i's pixels are batch[i].in,
  // an entry of the batched encode's device table.  The members the E step's stages read carry EncodeParams' names.
  struct RateProbeBatchParams
  {
    const ImageIO *batch;
    uint32_t nImages, imageStrips;
    uint32_t sizeX, sizeY, blocksX, blocksY, stripsX;
    int32_t vecIn;
    int32_t recordLimit;
    int32_t forced[3];
    const limg_hip_block_record *records;
    const float *invN;
    const RateDevice *states;
    unsigned long long *counters;
  };
  struct RateBudgetChunk { uint32_t n; unsigned long long maxBytes[64]; }; // k_rate_begin_batch's budgets, as kernel arguments
  // hMaxBytes: HOST array of `count` budgets (may die when the call returns); every search runs over [hLo, hHi].  dList: the call measures a list of error factors
  // (device memory; hMaxBytes may then be NULL): no search, the thresholds of dList[0]
  void launch_rate_begin_batch(RateDevice *dStates, unsigned long long *dCounters, const uint64_t *hMaxBytes, size_t count, uint32_t hLo, uint32_t hHi, hipStream_t s,
                               const uint32_t *dList = nullptr);
  // dImages: the ListImage table of a chunk of mixed shapes -- image i's fixed bytes are those of its own block count, fixedBytes is not read.  dList: the list form,
  // image i's size at dList[k] goes to dListBytes[i * listCount + k]
  void launch_rate_step_batch(RateDevice *dStates, unsigned long long *dCounters, uint32_t nImages, uint64_t fixedBytes, hipStream_t s, const ListImage *dImages = nullptr,
                              const uint32_t *dList = nullptr, unsigned long long *dListBytes = nullptr, uint32_t listCount = 0);
  void launch_rate_probe_batch(const RateProbeBatchParams &p, int channels, bool floatFast, hipStream_t s);
  // A chunk of images of MIXED shapes (limg_hip_encode_stream_budget_list*, limg_hip_stream_sizes_list*): the chunk's tables as encode_list_chunk puts them on the
  // device, records and invN of k_fit_tpb_list image after image from each image's firstBlock, states[i] / counters[i] image i's.  One workgroup per work strip of
  // the chunk.  No hook member: the kernarg segment is the same in both builds.
  struct RateProbeListParams
  {
    const ListImage *images;
    const ImageIO *batch;
    const uint32_t *firstStrip; // nImages: exclusive prefix of the images' work strips
    uint32_t nImages, nStrips;
    int32_t recordLimit;
    int32_t forced[3];
    const limg_hip_block_record *records;
    const float *invN;
    const RateDevice *states;
    unsigned long long *counters;
  };
  void launch_rate_probe_list(const RateProbeListParams &p, int channels, bool floatFast, hipStream_t s);

  void launch_synth_random_gradient(uint32_t *out, uint32_t w, uint32_t h, uint64_t seed, int opaque, uint32_t y0, hipStream_t s);
  void launch_synth_photo_noise(uint32_t *out, uint32_t w, uint32_t h, uint64_t seed, uint32_t y0, hipStream_t s);
  void launch_compare(const uint32_t *a, const uint32_t *b, uint64_t count, int channels, unsigned long long *dErrorSum, hipStream_t s);
}

#endif
