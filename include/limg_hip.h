/* limg_hip.h -- C ABI of liblimg_hip.so: the MI355X (gfx950) implementation of limg's encode hot path.
 *
 * Drop-in boundary for the reference's `limg_encode3d_test` / `limg_encode3d_test_perf` / `limg_compare` and (further down)
 * `limg_blocked_encode3d_test` (reference: src/limg.h:27-48; the reference has no FFI layer, its API is plain C++ functions), plus
 * the build-defined compact stream pair the task names `limg_encode` / `limg_decode`.  Every entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only; no C++ or torch types.  A header-only C++ shim with the *exact* reference
 * signatures is in include/limg_hip_shim.hpp.  There is no CPU fallback: without a HIP device limg_hip_init fails.
 *
 * Data layout (identical to the reference, src/limg.h:29-33 and SURVEY.md 8(b)):
 *   pIn            row-major uint32 RGBA8, byte 0 = R, sizeX*sizeY elements, row stride sizeX
 *   8 uint32 planes (pDecoded, pShiftABCX, pColAMin, pColAMax, pColBMin, pColBMax, pColCMin, pColCMax)
 *   3 uint8  planes (pFactorsA, pFactorsB, pFactorsC), each sizeX*sizeY elements, row stride sizeX
 * Ownership: the caller allocates and frees every image/plane buffer; the library never retains caller pointers.
 * The context owns device staging buffers, per-block scratch and the dither noise table.
 */
#ifndef LIMG_HIP_H
#define LIMG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* same numeric values as `enum limg_result` (src/limg.h:9-18) */
typedef enum limg_hip_result
{
  limg_hip_success = 0,
  limg_hip_error_Generic = 100, /* also: any HIP runtime failure */
  limg_hip_error_InvalidParameter,
  limg_hip_error_ArgumentNull,
  limg_hip_error_OutOfBounds,
  limg_hip_error_MemoryAllocationFailure
} limg_hip_result;

/* same member order and meaning as `struct limg_encode3d_info` (src/limg.h:29-33) */
typedef struct limg_hip_encode3d_info
{
  uint32_t *pDecoded, *pShiftABCX, *pColAMin, *pColAMax, *pColBMin, *pColBMax, *pColCMin, *pColCMax;
  uint8_t *pFactorsA, *pFactorsB, *pFactorsC;
} limg_hip_encode3d_info;

/* `limg_encode_3d_output<4>` (src/limg_internal.h:343-353): the per-block decomposition record, 64 bytes.
 * For 3-channel input lane 3 of every array is 0 (the reference's 48-byte <3> layout is this minus lane 3). */
typedef struct limg_hip_block_record
{
  float avg[4];
  int16_t dirA_min[4], dirA_max[4], dirB_offset[4], dirB_mag[4], dirC_offset[4], dirC_mag[4];
} limg_hip_block_record;

/* Optional per-block ("compact") outputs of the device entry point; any pointer may be NULL. Device pointers. */
typedef struct limg_hip_compact_out
{
  limg_hip_block_record *pRecords; /* blocksX*blocksY, raster order */
  uint32_t *pShifts;               /* blocksX*blocksY: shiftA | shiftB << 8 | shiftC << 16 | ditherCalls << 24 */
} limg_hip_compact_out;

/* Knobs that have no parameter in the reference signature (the reference has none of these: src/limg.h:27-48).  Fill with limg_hip_default_options, then set what
 * you need.  The struct is VERSIONED BY ITS SIZE: `struct_size` is sizeof(limg_hip_options) as the caller's compiler saw it (limg_hip_default_options below writes
 * it); the library reads and writes only that many bytes and gives every member beyond them its default, so members can be appended without breaking a caller
 * built against an earlier header.  Nothing here changes results except forced_shift, dither_pcg and float_mode; there are no fault-injection or test knobs in this
 * library (those live in liblimg_hip_test.so, include/limg_hip_test_hooks.h, which the test suite loads instead). */
typedef struct limg_hip_options
{
  uint32_t struct_size;    /* sizeof(limg_hip_options) in the caller's build; limg_hip_set_options rejects 0, anything not a multiple of 4 and anything too short for forced_shift */
  int32_t forced_shift[3]; /* all three in 0..8: bypass the shift search (a10-a12) with this triple; otherwise {-1,-1,-1} */
  int32_t force_split_kernels; /* non-0: use the three-launch path (fit+search, scan, dither+store) even where the persistent kernel applies */
  int32_t dither_pcg;          /* non-0: the reference's PCG dither (src/limg.cpp:799-822, what it runs on hosts without AES-NI) instead of the AES one */
  int32_t float_mode;          /* 0 (default) = EXACT: the float stage op for op as the reference's strict SSE build (DPPS order, x86 RSQRTPS table, correctly
                                  rounded divisions): every plane bit-identical to the reference.  1 = FAST: hardware v_rsq_f32 / v_rcp_f32 and fused multiply-adds;
                                  contract: the integer stage stays bit-exact given the same records, extrema within +-2 LSB on >= 99.9 % of blocks, perceptual PSNR
                                  within 0.10 dB of EXACT; the 8x8 path only (the merged-block encoder always runs EXACT) */
  int32_t legacy_float_stage;  /* non-0: run the float stage inside the E step with lane == pixel (round-1 mapping; what images with partial edge blocks always use)
                                  instead of the one-lane-per-block kernel k_fit_tpb.  Same bits either way; A/B switch for tests and the bench */
  int32_t collect_stats;       /* non-0: every encode (8x8 path and merged-block encoder) also leaves the reference's bit statistics for limg_hip_last_stats */
  int32_t host_noise_table;    /* non-0: build the context's dither noise table on the host (one serial AES walk + upload, ~100 ms per new size class: what rounds 1-2 did)
                                  instead of filling it on the GPU from the embedded chain checkpoints.  Same bytes; A/B switch for tests */
  int32_t batch_sub_images;    /* limg_hip_encode3d_batch_device runs a long list as a PIPELINE of sub-batches: the float-stage kernel of sub-batch k + 1 on a stream of
                                  the context's own next to the persistent kernel of sub-batch k (which leaves it a residency slot: 5 workgroups per CU instead of 6).
                                  0 = automatic (sub-batches of 8 for lists of 32 images and more, of 4 from 16 images, none below); > 0 = sub-batches of this many
                                  images; < 0 = never: one launch pair for the whole list.  Same planes in every case */
  int32_t ragged_bands;        /* images with a partial last block COLUMN and one dither chain (poolThreads == 0): the host's chain walk -- the floor of this class -- is
                                  pipelined with the GPU in this many bands of block rows (E step band by band, the walk under it, every band's F step under the next band's
                                  walk).  0 = automatic (16 bands from 64 block rows x 32 block columns on), N > 0 = N bands, < 0 = off (one E launch, walk, one F launch) */
  int32_t ragged_walk_threads; /* ... with several chains (poolThreads > 0) the chains are independent, as on the reference's thread pool (src/limg.cpp:2114-2134): they are
                                  walked on this many host threads (0 = one per chain, at most 16 and the host's hardware threads; 1 = serial) */
} limg_hip_options;

typedef struct limg_hip_context limg_hip_context;

/* Thread safety.  The reference is re-entrant (stack scratch only, src/limg.cpp:1890-1891).  Here a context owns device scratch, so:
 *   - the blocking HOST-pointer entries (limg_hip_encode3d, _encode3d_perf, _compare, _blocked_encode3d, _encode_stream, _decode_stream, _blocked_encode_stream,
 *     _blocked_decode_stream) take a mutex inside the
 *     context: any number of threads may call them on one shared context at once (this is what the C++ shim's limg_encode3d_test & co. rely on); the calls run
 *     one after the other;
 *   - the asynchronous *_device entries enqueue kernels that use the context's scratch after the call has returned: use one context per HIP stream / thread
 *     for those (contexts are independent and cheap next to an image: tests/test_gpu_parity.py::test_two_contexts_on_two_threads);
 *   - limg_hip_init / limg_hip_shutdown / limg_hip_set_options of one context must not race with calls on that context. */

/* Create / destroy a context bound to HIP device `device` (-1 = current device).  No reference analogue
 * (the reference keeps no state besides CPUID flags, src/limg_simd.cpp:57-60). */
limg_hip_result limg_hip_init(int device, limg_hip_context **ppCtx);
void limg_hip_shutdown(limg_hip_context **ppCtx);
/* Defaults into the first `structSize` bytes of *pOptions (struct_size = structSize).  Call it through limg_hip_default_options, which passes the size of the struct
 * as the CALLER was compiled. */
void limg_hip_default_options_sized(limg_hip_options *pOptions, size_t structSize);
static inline void limg_hip_default_options(limg_hip_options *pOptions) { limg_hip_default_options_sized(pOptions, sizeof(limg_hip_options)); }
/* Takes pOptions->struct_size bytes; members beyond them get their defaults. */
limg_hip_result limg_hip_set_options(limg_hip_context *pCtx, const limg_hip_options *pOptions);
/* pOptions->struct_size must be set on entry (= the room the caller has); that many bytes are written.  Read, change one member, set: nothing else is reset. */
limg_hip_result limg_hip_get_options(const limg_hip_context *pCtx, limg_hip_options *pOptions);

/* Replaces `limg_encode3d_test` (src/limg.h:35, src/limg.cpp:2175-2265).  HOST pointers; blocking.
 * poolThreads: 0 == `pThreadPool = nullptr` (one dither chain over the image); T > 0 == a pool of T threads, i.e. T*4
 * row strips each restarting the dither chain (src/limg.cpp:2114-2134).  bool parameters are ints (0 / non-0). */
limg_hip_result limg_hip_encode3d(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_encode3d_info *pInfo,
                                  uint32_t errorFactor, int poolThreads, int fastBitCrushing);

/* Replaces `limg_encode3d_test_perf` (src/limg.h:37, src/limg.cpp:2267-2327): same work, nothing stored. HOST pointer. */
limg_hip_result limg_hip_encode3d_perf(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint32_t errorFactor,
                                       int poolThreads, int fastBitCrushing);

/* Device-resident variant of `limg_encode3d_test`: every pointer (pIn, the 11 planes inside *pInfo, pCompact members)
 * is a DEVICE pointer; pInfo / pCompact themselves are host structs.  Asynchronous on `stream` (a hipStream_t passed
 * as void*; NULL = default stream).  pInfo == NULL gives the `_perf` behaviour (fit + search only).
 * Compact mode (SURVEY.md 8(d), 8.05 B/px): pInfo with the eight uint32 plane pointers all NULL and the three factor planes set
 * writes only the crushed factor bytes; together with pCompact (records + shift words) that is everything a decoder needs.
 * Alignment: any (4-byte aligned pIn / uint32 planes) is accepted.  The kernels use 16-byte accesses on pIn when it is 16-byte aligned and
 * sizeX % 4 == 0, and on the factor planes when all three are 16-byte aligned and sizeX % 16 == 0; other pointers (sliced, offset) take
 * dword / byte paths with identical results (hipMalloc and torch allocations are 256-byte aligned). */
limg_hip_result limg_hip_encode3d_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                         const limg_hip_encode3d_info *pInfo, const limg_hip_compact_out *pCompact, uint32_t errorFactor, int poolThreads,
                                         int fastBitCrushing, void *stream);

/* A list of images of ONE shape, each with its own 11 planes: replaces the reference's per-file loop `for (file) limg_encode3d_test(...)` (src/main.cpp:278-323, what
 * its `--count` benchmark and BASELINE configs 2 / 4 run).  ppIn[i] / pInfos[i] are the DEVICE pointers of image i (the arrays themselves are host memory and may be
 * freed when the call returns).  Every image gets the planes a single limg_hip_encode3d_device call would give it (own dither chain(s), same poolThreads rule), but
 * the whole list goes through one launch pair -- one float-stage grid over the blocks of all images, one persistent launch over the strips of all images -- so a
 * small image's ramp-up and drain are paid once per list, not once per image.  Images with partial edge blocks, compact mode (planes NULL) and the A/B options
 * fall back to one encode per image, same results.  Asynchronous on `stream`. */
limg_hip_result limg_hip_encode3d_batch_device(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                               const limg_hip_encode3d_info *pInfos, uint32_t errorFactor, int poolThreads, int fastBitCrushing, void *stream);

/* Replaces `limg_compare` (src/limg.h:48, src/limg.cpp:2455-2491): perceptual PSNR; HOST pointers. */
double limg_hip_compare(limg_hip_context *pCtx, const uint32_t *pImageA, const uint32_t *pImageB, size_t sizeX, size_t sizeY, int hasAlpha,
                        double *pMeanSquaredError, double *pMaxPossibleSquaredError);
/* same on DEVICE pointers (blocking on `stream`) */
double limg_hip_compare_device(limg_hip_context *pCtx, const uint32_t *pImageA, const uint32_t *pImageB, size_t sizeX, size_t sizeY, int hasAlpha,
                               double *pMeanSquaredError, double *pMaxPossibleSquaredError, void *stream);

/* Synthetic inputs of SURVEY.md 8(d), generated directly in HBM (DEVICE pointer, async on stream).
 * (y0, fullWidth) let a rank generate only its row strip of a larger image. */
limg_hip_result limg_hip_synth_random_gradient_device(uint32_t *pOut, size_t width, size_t height, uint64_t seed, int opaque, size_t y0, void *stream);
limg_hip_result limg_hip_synth_photo_noise_device(uint32_t *pOut, size_t width, size_t height, uint64_t seed, size_t y0, void *stream);

/* Waits for the device and returns limg_hip_error_Generic if the persistent kernel's bounded look-back wait ever timed out (protocol safety net; the host-pointer
 * entry points call it themselves and return the error).  Such a timeout is never silent: the strip that gave up and every later strip of its dither chain store
 * NOTHING that depends on the chain position -- their pDecoded / pFactorsA/B/C pixels keep what the caller's buffers held, the block-uniform planes may be partly
 * written -- so a caller of the asynchronous *_device entries that skips this check cannot end up with wrongly dithered planes that look complete.
 * Progress does not depend on what else runs on the GPU: every work strip id is drawn from an atomic ticket by a workgroup that is already resident, so any number
 * of contexts may have persistent kernels in flight on their own streams at once (tests/test_gpu_concurrency.py). */
limg_hip_result limg_hip_check_device_status(limg_hip_context *pCtx);

/* The statistics the reference's limg_encode3d_test / limg_blocked_encode3d_test print themselves (src/limg.cpp:2232-2248; counters :1971-1999, :1561-1590):
 * pCounters30[f] (f = 0..2: factor A, B, C) = bits kept, summed over the pixels ((8 - shift) per pixel); pCounters30[3 + 9 f + s] = pixels whose block crushed factor
 * f by s bits.  "Average Block Bits" = (c[0] + c[1] + c[2]) / pixels; the histogram line of factor f = c[3 + 9 f + s] * 100 / pixels for s = 0..8 ("8 bit" .. "0 bit").
 * Of the context's last encode made with limg_hip_options.collect_stats set (a batched encode: all its images together); waits for that encode.
 * The library itself prints nothing (SURVEY 8(b) "Side effects"); include/limg_hip_shim.hpp's limg_print_stats and tools/limg_hip_cli.cpp print upstream's lines. */
limg_hip_result limg_hip_last_stats(limg_hip_context *pCtx, uint64_t *pCounters30, uint64_t *pPixels);
/* limg_hip_encode3d / limg_hip_blocked_encode3d that ALSO return the counters of that very encode (upstream keeps them on the stack of the call, src/limg.cpp:1975-1976,
 * so its printout is per call whatever other threads do): encode and fetch happen under the context's mutex, collect_stats is on for the call only.  What the C++
 * shim's limg_encode3d_test / limg_blocked_encode3d_test call when limg_hip_shim::print_stats(true) is set -- safe from any number of threads on one context. */
limg_hip_result limg_hip_encode3d_stats(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_encode3d_info *pInfo,
                                        uint32_t errorFactor, int poolThreads, int fastBitCrushing, uint64_t *pCounters30, uint64_t *pPixels);

/* Per-kernel timing for the bench (HIP events recorded on the stream each profiled encode is launched on).
 * limg_hip_profile_end writes 3 floats per profiled encode: k_fit_search, k_strip_scan (or the host chain walk of ragged
 * images), k_dither_store, in milliseconds; returns the number of encodes written or -1. */
limg_hip_result limg_hip_profile_begin(limg_hip_context *pCtx);
int limg_hip_profile_end(limg_hip_context *pCtx, float *pMs, int maxEncodes);

/* Host-only helpers (no GPU touched): the data-independent dither noise stream and the strip partition rule.
 *  limg_hip_host_noise_table : `calls` x 64 noise bytes of a chain of full 8x8 blocks starting at the reference's seed
 *                              (src/limg.cpp:1893); byte p of call k is what the AES dither ANDs with ditherSize for pixel p.
 *  limg_hip_host_chain_call  : one dither call's state walk over `pixelCount` pixels (64 for an 8x8 block, any count for a rectangle of the
 *                              merged-block encoder): returns the next chain value (src/limg.cpp:824-879), optionally writing the noise
 *                              bytes (buffer of max(64, pixelCount) bytes).
 *                              forceSoftwareAes bit 0: do not use AES-NI; bit 1: PCG dither instead of AES.
 *  limg_hip_host_partition   : src/limg.cpp:2114-2134 in block rows: chain c < count-1 owns rows [c*rows, (c+1)*rows), the last the rest. */
limg_hip_result limg_hip_host_noise_table(uint8_t *pOut, size_t calls);
/*  limg_hip_noise_table_device: the same stream written by the GPU (what a context does for itself on the first encode of a size class): `calls` x 64 bytes into a
 *                              DEVICE buffer (16-byte aligned), asynchronous on `stream`; at most 2^27 calls (the reach of the embedded checkpoints: dense ones -- every
 *                              1024 calls -- through 16 Mi calls, far ones -- every 65536 -- beyond, which the context makes dense on host threads when an image of
 *                              more than 5.59 M blocks needs them). */
limg_hip_result limg_hip_noise_table_device(limg_hip_context *pCtx, uint8_t *pOutDevice, size_t calls, void *stream);
uint64_t limg_hip_host_chain_call(uint64_t chainValue, size_t pixelCount, uint8_t *pNoise64, int forceSoftwareAes);
limg_hip_result limg_hip_host_partition(size_t sizeY, int poolThreads, uint32_t *pChainCount, uint32_t *pChainBlockRows);
/*  limg_hip_host_chain_checkpoints: walks `calls` full-block dither calls from the reference's seed (src/limg.cpp:1893) and writes the chain value that call
 *                              i * every starts from to pOut[i] (may be NULL); returns the value after the last call.  The library's embedded checkpoint
 *                              table (one value every 1024 calls, from which the GPU fills the noise table in parallel) is generated and checked with it. */
uint64_t limg_hip_host_chain_checkpoints(size_t calls, size_t every, uint64_t *pOut, int pcg);
/*  limg_hip_host_dense_checkpoints: the chain values that calls number (first + k) * 1024, k < count, start from -- what the GPU's noise-table fill is given -- from the
 *                              embedded tables alone: the dense one where it reaches, the far one + 65536 calls on foot per far value (host threads) beyond;
 *                              limg_hip_error_OutOfBounds beyond 2^27 calls.  Equal to limg_hip_host_chain_checkpoints' serial walk (tests/test_host.py). */
limg_hip_result limg_hip_host_dense_checkpoints(size_t first, size_t count, uint64_t *pOut);
/*  limg_hip_host_accurate_table: the accurate shift search's automaton in the expanded form a context uploads on its first accurate encode -- the same routine fills
 *                              both: 8 dwords per state = { a | phase2 << 5 | final << 31, byte offset of the next entry on pass, on fail, b, c, mul(a), mul(b),
 *                              mul(c) }, bits 24..26 of either offset = which factors (A, B, C) the successor's triple changes against this state's.  `dwords` must be
 *                              the table's size, 8 x its state count (18878 states: 151024), else limg_hip_error_InvalidParameter. */
limg_hip_result limg_hip_host_accurate_table(uint32_t *pOut, size_t dwords);

/* ---- merged-block encoder ----------------------------------------------------------------------------------------------------------
 * Replaces `limg_blocked_encode3d_test` (src/limg.h:46, src/limg.cpp:2329-2453), what the reference's CLI runs on a single file
 * (src/main.cpp:255): per-8x8 fit, greedy merge of similar neighbouring blocks into rectangles, re-fit + bit crush + dither + decode
 * per rectangle.  Struct = `limg_blocked_encode3d_info` (src/limg.h:39-44), same member order.  pBlockError is never written (it is not
 * upstream either) and may be NULL.  The pool argument of the reference only splits its first pass and has no effect on the result, so it
 * has no counterpart here.  Division of labour: fits, the block-similarity predicate, the per-rectangle work and all plane
 * stores run on the GPU; the greedy raster scan over precomputed similarity bits and the (inherently serial) dither chain walk run on the host. */
typedef struct limg_hip_blocked_encode3d_info
{
  uint32_t *pDecoded;
  uint8_t *pFactorsA, *pFactorsB, *pFactorsC, *pBlockError, *pBitsPerPixel;
  uint32_t *pShiftABCX, *pColAMin, *pColAMax, *pColBMin, *pColBMax, *pColCMin, *pColCMax, *pBlockIndex;
} limg_hip_blocked_encode3d_info;

typedef struct limg_hip_region { uint32_t ox, oy, rx, ry; } limg_hip_region; /* in 8x8 blocks, creation (= block index) order */

/* HOST pointers, blocking. */
limg_hip_result limg_hip_blocked_encode3d(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_blocked_encode3d_info *pInfo,
                                          uint32_t errorFactor, int fastBitCrushing);
limg_hip_result limg_hip_blocked_encode3d_stats(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_blocked_encode3d_info *pInfo,
                                                uint32_t errorFactor, int fastBitCrushing, uint64_t *pCounters30, uint64_t *pPixels);
/* DEVICE pointers (pIn and the planes inside *pInfo); returns when everything has been enqueued on `stream` -- the call itself waits for
 * the intermediate device results its host stages need. */
limg_hip_result limg_hip_blocked_encode3d_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                 const limg_hip_blocked_encode3d_info *pInfo, uint32_t errorFactor, int fastBitCrushing, void *stream);
/* The rectangles of the context's last merged-block encode (copies up to `capacity`, always reports the count). */
limg_hip_result limg_hip_blocked_regions(limg_hip_context *pCtx, limg_hip_region *pRegions, size_t capacity, size_t *pCount);
/* Milliseconds of the last merged-block encode: [0] pass 1 + similarity bits (GPU, incl. their copy to the host), [1] greedy merge (host, this thread), and --
 * overlapped with [1] on a worker thread, summed over its batches -- [2] per-rectangle fit + search (GPU, incl. copies), [3] dither chain walk (host),
 * [4] noise upload + dither/decode/store launch; [5] wall-clock total. */
limg_hip_result limg_hip_blocked_timing(limg_hip_context *pCtx, double *pMs6);
/* The similarity bits of the context's last merged-block encode (limg_hip_host_blocked_match_words() words per block, the layout of limg_hip_host_blocked_match_bits):
 * copies up to `capacityWords`, always reports the count.  For tests: the GPU kernel's bits against the host evaluation of the same records. */
limg_hip_result limg_hip_blocked_match_bits(limg_hip_context *pCtx, uint64_t *pBits, size_t capacityWords, size_t *pWords);
/* GPU time of the last merged-block encode's launches, from HIP events on the streams they run on: [0] pass 1 (the 8x8 path's float stage), [1] the similarity
 * kernels (16 bands, back to back), and summed over the worker's batches [2] the per-rectangle fit + search kernel, [3] chain-value upload + noise expansion +
 * dither/decode/store kernel -- after limg_hip_blocked_encode_stream*, which stores no plane: noise expansion + the stream's scan and pack kernels.  (What the GPU side costs with no host in the way: bench.py's kernel-only rate of the merged-block encoder.) */
limg_hip_result limg_hip_blocked_kernel_timing(limg_hip_context *pCtx, double *pMs4);
/* Host-only (no GPU touched): the block-similarity predicate `limg_encode_3d_matches` (src/limg.cpp:1137-1268) as the host merge evaluates it
 * for candidates outside the precomputed window; records in `limg_hip_block_record` layout. */
int limg_hip_host_blocked_matches(int channels, const limg_hip_block_record *pSeed, const limg_hip_block_record *pCandidate);
/* Host-only: the greedy raster merge (src/limg.cpp:1386-1496, :1813-1881) over per-block fits; pMatchBits = the similarity bits in the layout the
 * GPU kernel produces (limg_hip_host_blocked_match_words() 64-bit words per block) or NULL (every pair is evaluated on the host).  Writes up to
 * `capacity` rectangles in creation order, always reports the count. */
limg_hip_result limg_hip_host_blocked_merge(const limg_hip_block_record *pFits, const uint64_t *pMatchBits, size_t blocksX, size_t blocksY, int channels,
                                            limg_hip_region *pRegions, size_t capacity, size_t *pCount);
/* Host-only: the similarity bits of every block against its neighbourhood, computed on the host (tests, benchmarks of the merge). */
size_t limg_hip_host_blocked_match_words(void);
limg_hip_result limg_hip_host_blocked_match_bits(const limg_hip_block_record *pFits, size_t blocksX, size_t blocksY, int channels, uint64_t *pMatchBits);

/* ---- compact stream ("LMG3") -----------------------------------------------------------------------------------------------
 * The north-star names `limg_encode()` / `limg_decode()` and a bitstream; upstream has neither (src/limg.h:27-48 is the whole API,
 * SURVEY.md 0.1 / 8(f) #2).  These entry points are the build-defined pair over a container that holds exactly what the reference's
 * decoder (`limg_decode_block_from_factors_3d`, src/limg_decode.h:36-236, called at src/limg.cpp:2093) consumes, so that
 * decode(encode(image)) equals the reference's pDecoded plane bit for bit.  Layout, little endian, sections 8-byte aligned:
 *   limg_hip_stream_header | limg_hip_stream_block[blocksX * blocksY] (raster order) | payload (8-byte words)
 * Block payload at `payloadWord`: factor A field, B field, C field; a field of b = 8 - shift bits per pixel is b words, pixel
 * (row r, column x) of the 8x8 grid at bit (8 r + x) b (pixels outside the image are 0).  shift 8 => no field, except the
 * raw-byte escape (bit 24 + k of `shift`): 4-channel blocks whose factor-k alpha normal is non-zero keep the raw 8-bit factor,
 * because the reference multiplies it into the alpha lane even at shift 8. */
#define LIMG_HIP_STREAM_MAGIC 0x33474D4Cu /* "LMG3" */
#define LIMG_HIP_STREAM_VERSION 1u

typedef struct limg_hip_stream_header
{
  uint32_t magic, version;
  uint32_t sizeX, sizeY;
  uint32_t channels;    /* 3 or 4 (hasAlpha) */
  uint32_t errorFactor; /* informational */
  uint32_t blocksX, blocksY;
  uint64_t payloadWords; /* 8-byte words after the block table */
  uint64_t totalBytes;   /* header + table + payload */
  uint32_t flags;        /* bit 0: fast bit crushing, bit 1: PCG dither (informational); version 2: bit 2 = merged-block stream */
  uint32_t reserved[3];  /* 0; version 2: [0] = rectangle count */
} limg_hip_stream_header; /* 64 bytes */

typedef struct limg_hip_stream_block
{
  int16_t dirA_min[4], dirA_max[4], dirB_offset[4], dirB_mag[4], dirC_offset[4], dirC_mag[4]; /* `limg_encode_3d_output` minus avg */
  uint32_t shift;       /* shiftA | shiftB << 8 | shiftC << 16 | rawEscapeMask << 24 */
  uint32_t payloadWord; /* first payload word of this block */
} limg_hip_stream_block; /* 56 bytes */

/* Worst-case stream size for an image (what `capacity` must be at least); 0 if the image is too large for 32-bit payload offsets. */
size_t limg_hip_stream_bound(size_t sizeX, size_t sizeY);

/* "limg_encode": the encode hot path (same parameters as limg_hip_encode3d_device) followed by the stream packer.  DEVICE pointers,
 * asynchronous on `stream`; the stream's size lands in its header (`totalBytes`).  pBytes (host, may be NULL) receives it too,
 * which makes the call wait for the stream. */
limg_hip_result limg_hip_encode_stream_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream,
                                              size_t capacity, size_t *pBytes, uint32_t errorFactor, int poolThreads, int fastBitCrushing, void *stream);
/* "limg_decode" (a16 for every block): DEVICE pointers, asynchronous.  sizeX / sizeY must match the header (the kernel checks and
 * reports a mismatch or inconsistent offsets through limg_hip_check_device_status as limg_hip_error_InvalidParameter). */
limg_hip_result limg_hip_decode_stream_device(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t sizeX, size_t sizeY,
                                              void *stream);
/* HOST-pointer variants (blocking). */
limg_hip_result limg_hip_encode_stream(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                       size_t *pBytes, uint32_t errorFactor, int poolThreads, int fastBitCrushing);
limg_hip_result limg_hip_decode_stream(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t outPixels);
/* Host-only: validates a header (first 64 bytes suffice) and reports the image shape. */
limg_hip_result limg_hip_stream_info(const uint8_t *pStream, size_t streamBytes, size_t *pSizeX, size_t *pSizeY, int *pHasAlpha, size_t *pTotalBytes);

/* ---- batched stream encode: a list of images to version 1 streams in one call ---------------------------------------------------
 * limg_hip_encode3d_batch_device puts a list of same-shape images through one float-stage grid and one persistent launch, so that ramp-up and drain are paid once per
 * list; these entries do the same for the compact stream, which is what a caller who encodes a set of images keeps.
 * Result: stream i is byte for byte what limg_hip_encode_stream_device writes for image i with the same arguments and options; every image starts its own dither chain
 * (or chains: poolThreads means what it means there).  Nothing beyond `totalBytes` of a stream has a specified value.  All images have the shape sizeX x sizeY.
 * Errors, in this order and before anything touches the device: NULL context, array or array element: limg_hip_error_ArgumentNull;
 * limg_hip_stream_bound(sizeX, sizeY) == 0: limg_hip_error_InvalidParameter; capacityEach < that bound: limg_hip_error_OutOfBounds; (device form) any ppStreams[i] not
 * 16-byte aligned: limg_hip_error_InvalidParameter, whichever i it is.  Then count == 0: limg_hip_success with nothing done, as limg_hip_encode3d_batch_device.  A
 * refused call writes nothing.  Output buffers that overlap are not checked.
 * pBytes (device form: host array of `count` entries, or NULL): when given, the call waits for the streams and fills all `count` sizes from ONE download of the headers'
 * totalBytes, gathered on the device -- not one blocking copy per image.
 * Options: forced_shift, dither_pcg, float_mode, collect_stats (limg_hip_last_stats: all images of the list together) and batch_sub_images are honoured exactly as by
 * limg_hip_encode3d_batch_device.
 * Cost: a list that fits one launch pair is that batch's launches (image table, float stage, persistent kernel -- or its pipeline of sub-batches) plus ONE scan launch
 * (one workgroup per image: the strips' first payload words and the image's header) and ONE pack launch (min(strips of the list, 16 x CUs) persistent one-wave
 * workgroups striding over the strips of all images), whatever `count` is; the streams' pointers travel to the device as kernel arguments of a small launch.
 * One encode per image instead -- the same bytes -- for images with partial edge blocks, under force_split_kernels or legacy_float_stage, and for count == 1.
 * Longer lists go in chunks by the rule of limg_hip_encode3d_batch_device (1 GiB of block records, 32-bit strip ids); a chunk of one image takes the single call.
 * Context memory: per image OF A CHUNK 3 bytes per pixel of factor planes (limg_hip_context::streamFac, where the single call holds one image's), 4 bytes per work strip
 * and the per-block scratch of the plane batch; 32 bytes per image of the list (the table) and, with pBytes, 8 more.  limg_hip_context_device_bytes reports all of it.
 * Ordering: calls on one context and stream execute in order and may be issued back to back; ppIn / ppStreams may be freed when the call returns. */
/* DEVICE pointers, asynchronous on `stream`.  ppIn / ppStreams are HOST arrays of `count` device pointers and may be freed when the call returns. */
limg_hip_result limg_hip_encode_stream_batch_device(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                    uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes /* host, count entries, or NULL */,
                                                    uint32_t errorFactor, int poolThreads, int fastBitCrushing, void *stream);
/* HOST pointers, blocking, under the context's mutex.  pBytes required.  Uploads the images, runs the device form into context staging (per image 4 bytes per pixel and
 * the stream bound), checks the device status and downloads totalBytes of each stream -- not capacityEach. */
limg_hip_result limg_hip_encode_stream_batch(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                             uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes,
                                             uint32_t errorFactor, int poolThreads, int fastBitCrushing);

/* ---- ... each image at its own error factor ---------------------------------------------------------------------------------------------
 * "This list, each image at its own quality": the batched stream encode above with pErrorFactors[i] (HOST array of `count` entries in both forms; may be freed when the
 * call returns) in the place of errorFactor.
 * Result: stream i is byte for byte what limg_hip_encode_stream_device writes for image i at errorFactor = pErrorFactors[i] with the same arguments and options.  Any
 * value is allowed, 0 and odd ones included; stream i's header carries pErrorFactors[i] as given, as the single call's does.
 * Errors: those of limg_hip_encode_stream_batch_device, in its order, pErrorFactors counted among the pointers; then count == 0: limg_hip_success with nothing done.  A
 * refused call writes nothing.  pBytes, options (forced_shift, dither_pcg, float_mode, collect_stats, batch_sub_images), chunks and ordering: as that entry.
 * Cost: the shared-factor call's launches -- one float-stage grid, the persistent launch (k_encode_list_rated in the place of k_encode_persistent: the same loop, which
 * fetches its image's bit-crush thresholds from a device table once per work strip, with scalar loads, where the other reads kernel arguments) or its pipeline of
 * sub-batches, one scan, one pack -- plus one small launch per 64 images of a chunk that writes the threshold table from the factors, which travel as its kernel
 * arguments.  That is one launch pair per chunk however many distinct factors the list holds, where the calls above need one encode per distinct factor.
 * Fallback, the same bytes: images with partial edge blocks, force_split_kernels, legacy_float_stage, fastBitCrushing == 0 (the accurate search has no such kernel) and
 * count == 1 go through the entries above, the images grouped by error factor -- one limg_hip_encode_stream_batch_device per factor that two or more images share, one
 * limg_hip_encode_stream_device per factor of one image; a last chunk of one image takes the single call.
 * Context memory: what limg_hip_encode_stream_batch_device holds, and 32 bytes per image of the longest chunk for the threshold table. */
/* DEVICE pointers, asynchronous on `stream`.  ppIn / ppStreams / pErrorFactors are HOST arrays of `count` entries and may be freed when the call returns. */
limg_hip_result limg_hip_encode_stream_batch_ef_device(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                       uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes /* host, count entries, or NULL */,
                                                       const uint32_t *pErrorFactors /* host, count */, int poolThreads, int fastBitCrushing, void *stream);
/* HOST pointers, blocking, under the context's mutex.  pBytes required.  As limg_hip_encode_stream_batch. */
limg_hip_result limg_hip_encode_stream_batch_ef(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, const uint32_t *pErrorFactors, int poolThreads,
                                                int fastBitCrushing);

/* ---- stream encode to a byte budget: size probe and error-factor search (version 1 streams) -----------------------------------------
 * errorFactor is the stream's only rate knob.  A stream is 64 + 56 blocks + 8 x (payload words) bytes, and the payload words follow from the blocks' records -- which do
 * not depend on errorFactor -- and their shift triples, which depend on it through errorFactor / 2 only.  So the size at an error factor is the float stage once and,
 * per error factor, the per-pixel factors and the shift search of every block with the field widths summed (k_rate_probe): no dither, no decode, no plane, no packer.
 *
 * limg_hip_stream_sizes*: pBytes[i] = the totalBytes limg_hip_encode_stream* reports for the same image, arguments and options at errorFactor pErrorFactors[i]; any
 * value is allowed (0, odd ones).  The records are computed once; there is one probe launch per entry and ONE download.  pErrorFactors and pBytes are HOST arrays of
 * `count` entries in both forms.  Errors, in this order and before anything touches the device: NULL context, image or array: limg_hip_error_ArgumentNull;
 * limg_hip_stream_bound(sizeX, sizeY) == 0: limg_hip_error_InvalidParameter.  Then count == 0: limg_hip_success with nothing done.
 *
 * limg_hip_encode_stream_budget*: the stream of limg_hip_encode_stream* at an error factor chosen for maxBytes.  The search runs over h = errorFactor / 2 between
 * minErrorFactor / 2 and maxErrorFactor / 2 (0 means 2 and 1024) and is this algorithm, with size(h) the stream's length at errorFactor 2 h:
 *     if size(hHi) > maxBytes:          errorFactor = maxErrorFactor, withinBudget = 0       (the call still succeeds and writes that stream)
 *     elif size(hLo) <= maxBytes:       errorFactor = minErrorFactor, withinBudget = 1
 *     else bisect with size(lo) > maxBytes >= size(hi) until hi - lo == 1:  errorFactor = 2 hi, withinBudget = 1
 * With withinBudget = 1 the stream is never longer than maxBytes (only measured values are returned).  The size is NOT monotone in errorFactor (the shift search is
 * greedy), so errorFactor is the smallest that fits only where it happens to be; a budget may even be refused that some error factor below maxErrorFactor would meet.
 * probes: sizes measured, at most 2 + ceil(log2(hHi - hLo)).  The stream written is byte for byte limg_hip_encode_stream_device's at pResult->errorFactor, and
 * pResult->bytes its totalBytes.  pResult (host): set struct_size to sizeof(limg_hip_budget_result) before the call.
 * Errors: those of limg_hip_encode_stream_device in its order, pResult counted among the pointers; then an odd bound, a bound below 2, minErrorFactor >
 * maxErrorFactor, maxBytes == 0 or a struct_size below the struct's: limg_hip_error_InvalidParameter.  All before anything touches the device; a refused call writes
 * nothing.
 * The device forms enqueue all probes at once -- the thresholds of the next probe are written on the device (k_rate_step, the search of limg_hip_rate_step.h) -- wait
 * ONCE for the 48-byte state, and then encode.  They SYNCHRONISE `stream`, so they cannot be captured into a graph.
 * Fallback: images with partial edge blocks, force_split_kernels, legacy_float_stage and fastBitCrushing == 0 have no probe kernel; each size is then one ordinary
 * stream encode (budget: into the caller's buffer; sizes: into context staging of the stream bound) whose totalBytes is read back, driven by the same search function:
 * the same results, one wait per size.
 * Options: forced_shift (a flat size curve), dither_pcg and float_mode are honoured as by limg_hip_encode_stream_device.
 * Context memory: 48 + 24 + 8 bytes of state and counter, and 12 bytes per entry of a sizes list, besides what a stream encode of the image holds. */
typedef struct limg_hip_budget_result
{
  uint32_t struct_size;  /* in: sizeof(limg_hip_budget_result) */
  uint32_t errorFactor;  /* the error factor the stream was encoded with */
  uint32_t probes;       /* sizes the search measured */
  uint32_t withinBudget; /* 1: bytes <= maxBytes */
  uint64_t bytes;        /* the stream's totalBytes */
} limg_hip_budget_result; /* 24 bytes */

/* DEVICE image, asynchronous probes, ONE wait for the sizes. */
limg_hip_result limg_hip_stream_sizes_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const uint32_t *pErrorFactors,
                                             size_t count, size_t *pBytes, int poolThreads, int fastBitCrushing, void *stream);
/* HOST image, blocking, under the context's mutex. */
limg_hip_result limg_hip_stream_sizes(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const uint32_t *pErrorFactors, size_t count,
                                      size_t *pBytes, int poolThreads, int fastBitCrushing);
/* DEVICE pointers (pIn, pStream: 16-byte aligned, capacity >= limg_hip_stream_bound); waits for `stream`. */
limg_hip_result limg_hip_encode_stream_budget_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream,
                                                     size_t capacity, size_t maxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads,
                                                     int fastBitCrushing, limg_hip_budget_result *pResult, void *stream);
/* HOST pointers, blocking, under the context's mutex.  capacity may be below the bound: pResult is filled, and limg_hip_error_OutOfBounds returned with nothing written
 * to pStream, where pResult->bytes > capacity. */
limg_hip_result limg_hip_encode_stream_budget(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                              size_t maxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                              limg_hip_budget_result *pResult);

/* ---- budgeted stream encode of a list: one search per image, the probes of all images in the same launches ------------------------
 * "Compress these `count` same-shape images to at most pMaxBytes[i] bytes each": the product of the batched stream encode and the budget entries above.
 * Result, for every i: pResults[i] holds exactly what limg_hip_encode_stream_budget_device puts in *pResult for image i with maxBytes = pMaxBytes[i] and the same
 * bounds, arguments and options; ppStreams[i] is byte for byte limg_hip_encode_stream_device's stream at pResults[i].errorFactor.
 * Independence: every image runs its own search (rate_begin / rate_step of the algorithm above); one image's outcome -- refused, met at the lower bound, bisected --
 * never touches another's.  minErrorFactor / maxErrorFactor are shared by the list; the budgets are per image.  pMaxBytes and pResults are HOST arrays of `count`
 * entries in both forms; set struct_size in EVERY pResults[i] before the call.
 * Errors, all before anything touches the device -- a refused call writes nothing to any stream or result -- in this order: (1) those of
 * limg_hip_encode_stream_batch_device in its order, pMaxBytes and pResults counted among the pointers; (2) the bound rules above (odd, below 2, min > max):
 * limg_hip_error_InvalidParameter; (3) any pMaxBytes[i] == 0 or any struct_size below the struct's: limg_hip_error_InvalidParameter, whichever i it is; (4) count == 0:
 * limg_hip_success with nothing done.
 * Cost: lists go chunk by chunk by the rule of limg_hip_encode3d_batch_device (1 GiB of block records, 32-bit strip ids).  Per chunk: the image table and ONE k_fit_tpb
 * grid over all its images (records in the context's float mode), one k_rate_begin_batch per 64 images, then 2 + ceil(log2(hHi - hLo)) pairs of k_rate_probe_batch
 * (one workgroup per image and work strip; the workgroups of an image whose search is over return at their first load) and k_rate_step_batch, ONE copy of the chunk's
 * states and ONE wait -- whatever the chunk's length: for 64 images over the default bounds 2 table launches, the float stage, one begin and 22 probe / step launches
 * with one wait, where 64 single calls are 64 x 24 launches and 64 waits.  Then the chunk is encoded ONCE, every image at the error factor its search chose: one
 * limg_hip_encode_stream_batch_ef_device -- a threshold-table launch, one launch pair, scan and pack, whatever the searches chose -- or, where all chose the same value,
 * one limg_hip_encode_stream_batch_device.  pResults[i].bytes is the size the probe measured at the result, which is the stream's totalBytes: no wait follows the
 * encodes.  A chunk of one image takes the single call.
 * Synchronisation: the device form SYNCHRONISES `stream` once per chunk, for that chunk's search states; it cannot be captured into a graph.  The streams themselves
 * are complete in stream order behind the call.
 * Fallback: where the single call has no probe kernel (partial edge blocks, force_split_kernels, legacy_float_stage, fastBitCrushing == 0) and for count == 1 the call
 * is the loop of single budget calls: the same results by construction.
 * Options: as the single call.  limg_hip_last_stats after these entries is that of the last encode issued: the last chunk, all its images together.
 * Context memory, besides what limg_hip_encode_stream_batch_device holds for the longest chunk: 72 bytes of state (sizeof RateDevice: the 48-byte search state, the list
 * position and the thresholds) + 8 bytes of counter = 80 bytes per image of the longest chunk (streamRateState, streamRateCounter); the probes read the images through
 * the batched encode's own table (96 bytes per image of a chunk, no second table), and the final encode's threshold table (32 bytes per image) lies in the chunk's
 * search states, which are on the host by then: no memory of its own.  limg_hip_context_device_bytes reports all of it.
 * Out of scope: version 2 streams; the accurate search with per-image error factors in one launch (it takes
 * the grouped fallback of limg_hip_encode_stream_batch_ef_device); the CLI, which encodes one file. */
/* DEVICE pointers; ppIn / ppStreams are HOST arrays of `count` device pointers (streams 16-byte aligned, capacityEach >= limg_hip_stream_bound) and, as pMaxBytes, may
 * be freed when the call returns.  Waits for `stream`. */
limg_hip_result limg_hip_encode_stream_budget_batch_device(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                           uint8_t *const *ppStreams, size_t capacityEach, const size_t *pMaxBytes /* host, count */,
                                                           uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                           limg_hip_budget_result *pResults /* host, count, struct_size set in each */, void *stream);
/* HOST images and HOST stream buffers, blocking, under the context's mutex.  Uploads the list, runs the device form into context staging (as
 * limg_hip_encode_stream_batch) and downloads pResults[i].bytes of each stream.  capacityEach may be below the bound: where it is below some pResults[i].bytes, all
 * results are filled, NO stream is written and limg_hip_error_OutOfBounds is returned -- the single host call's rule. */
limg_hip_result limg_hip_encode_stream_budget_batch(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                    uint8_t *const *ppStreams, size_t capacityEach, const size_t *pMaxBytes /* host, count */,
                                                    uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                    limg_hip_budget_result *pResults /* host, count, struct_size set in each */);

/* ---- stream encode to a quality target: error-factor search on the stream's measured error (version 1 streams) ----------------------
 * The budget entries answer "at most N bytes"; these answer "at least this good": the stream of limg_hip_encode_stream* at the COARSEST error factor the search finds whose
 * error sum against its own image -- limg_hip_decode_stream_windows_error over the whole image, mse * pixels of limg_hip_compare(image, decode(stream)) -- is at most
 * maxErrorSum.  For a PSNR target pass limg_hip_error_sum_for_psnr(sizeX, sizeY, hasAlpha, dB): "PSNR >= dB" is then the exact integer comparison errorSum <= limit.
 * The search runs over h = errorFactor / 2 between minErrorFactor / 2 and maxErrorFactor / 2 (even bounds; 0 means 2 and 1024) and is this algorithm, with E(h) the error
 * sum of the stream at errorFactor 2 h (limg_hip_quality_step.h: the budget search on the mirrored axis hLo + hHi - h, with E in the size's place):
 *     if E(hLo) > maxErrorSum:          errorFactor = minErrorFactor, withinTarget = 0       (not even the finest allowed value reaches the target; the call still
 *                                                                                             succeeds and writes that stream)
 *     elif E(hHi) <= maxErrorSum:       errorFactor = maxErrorFactor, withinTarget = 1
 *     else bisect with E(lo) <= maxErrorSum < E(hi), mid = hi - (hi - lo) / 2, until hi - lo == 1:  errorFactor = 2 lo, withinTarget = 1
 * Every value is asked for once (hLo == hHi asks once); probes is at most 2 + ceil(log2(hHi - hLo)).  With withinTarget = 1 the result is a value whose error was MEASURED
 * and found to meet the limit.  E is NOT monotone in errorFactor (the shift search is greedy and the dither differs between error factors), so errorFactor is the largest
 * that meets the limit only on curves that happen to rise monotonically: the search may return a finer stream than the coarsest that would do.
 * The stream written is byte for byte limg_hip_encode_stream_device's at pResult->errorFactor, pResult->bytes its totalBytes and pResult->errorSum its E.  maxErrorSum == 0
 * is allowed: it asks for a lossless image.  pResult (host): set struct_size to sizeof(limg_hip_quality_result) before the call; the budget result's rule.
 * Each probe is ONE ordinary stream encode into the caller's buffer -- so every shape, option and search the stream encode accepts works here, there is no fallback
 * class --, ONE error launch over the whole image and ONE 8-byte download.  The device form therefore WAITS for `stream` once per probe (and once more for the size) and
 * cannot be captured into a graph.  Where the last probe was not the result, the result's stream is encoded once more.
 * Errors: those of limg_hip_encode_stream[_device] in its order, pResult counted among the pointers; then an odd bound, a bound below 2, minErrorFactor > maxErrorFactor or
 * a struct_size below the struct's: limg_hip_error_InvalidParameter.  All before anything touches the device; a refused call writes nothing.
 * Context memory: 8 bytes per image of the call besides what the stream encode and one batched window call hold.
 * Follow-up, not here: a device-stepped search that enqueues all probes at once needs the encode's thresholds from a device table for a single image too (the list
 * encode has one); error at reduced levels; version 2 streams; other metrics.  (Lists of mixed shapes: limg_hip_encode_stream_quality_list below.) */
typedef struct limg_hip_quality_result
{
  uint32_t struct_size;  /* in: sizeof(limg_hip_quality_result) */
  uint32_t errorFactor;  /* the error factor the stream was encoded with */
  uint32_t probes;       /* error sums the search measured */
  uint32_t withinTarget; /* 1: errorSum <= maxErrorSum */
  uint64_t bytes;        /* the stream's totalBytes */
  uint64_t errorSum;     /* the stream's error sum against the image */
} limg_hip_quality_result; /* 32 bytes */

/* DEVICE pointers (pIn, pStream: 16-byte aligned, capacity >= limg_hip_stream_bound); waits for `stream`. */
limg_hip_result limg_hip_encode_stream_quality_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream,
                                                      size_t capacity, uint64_t maxErrorSum, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads,
                                                      int fastBitCrushing, limg_hip_quality_result *pResult, void *stream);
/* HOST pointers, blocking, under the context's mutex.  capacity may be below the bound: pResult is filled, and limg_hip_error_OutOfBounds returned with nothing written
 * to pStream, where pResult->bytes > capacity. */
limg_hip_result limg_hip_encode_stream_quality(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                               uint64_t maxErrorSum, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                               limg_hip_quality_result *pResult);
/* A list of `count` same-shape images: pResults[i] and ppStreams[i] are exactly the single call's for image i with maxErrorSum = pMaxErrorSums[i] and the same bounds,
 * arguments and options; one image's outcome never touches another's.  Per round the images whose search is not over are encoded at their own next value by ONE
 * limg_hip_encode_stream_batch_ef_device call, measured by ONE error launch and stepped behind ONE download: a list costs at most 2 + ceil(log2(hHi - hLo)) rounds, plus
 * at most one final list encode for the images whose buffer does not hold their result's stream, and one download of the sizes -- whatever its length.  A list of one is
 * the single call.  pMaxErrorSums and pResults are HOST arrays of `count` entries in both forms; set struct_size in EVERY pResults[i].
 * Errors, all before anything touches the device -- a refused call writes nothing to any stream or result -- in this order: (1) those of
 * limg_hip_encode_stream_batch_device in its order, pMaxErrorSums and pResults counted among the pointers; (2) the bound rules above: limg_hip_error_InvalidParameter;
 * (3) any struct_size below the struct's: limg_hip_error_InvalidParameter; (4) count == 0: limg_hip_success with nothing done.
 * DEVICE pointers; ppIn / ppStreams are HOST arrays of `count` device pointers (streams 16-byte aligned, capacityEach >= limg_hip_stream_bound).  Waits for `stream` once
 * per round. */
limg_hip_result limg_hip_encode_stream_quality_batch_device(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                            uint8_t *const *ppStreams, size_t capacityEach, const uint64_t *pMaxErrorSums /* host, count */,
                                                            uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                            limg_hip_quality_result *pResults /* host, count, struct_size set in each */, void *stream);
/* HOST images and HOST stream buffers, blocking, under the context's mutex.  capacityEach may be below the bound: where it is below some pResults[i].bytes, all results are
 * filled, NO stream is written and limg_hip_error_OutOfBounds is returned -- the single host call's rule. */
limg_hip_result limg_hip_encode_stream_quality_batch(limg_hip_context *pCtx, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                     uint8_t *const *ppStreams, size_t capacityEach, const uint64_t *pMaxErrorSums /* host, count */,
                                                     uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                     limg_hip_quality_result *pResults /* host, count, struct_size set in each */);

/* ---- stream encode of a list of MIXED shapes in one launch pair -----------------------------------------------------------------------
 * The list entries above take one sizeX x sizeY for the whole list.  These take one item per image -- its pixels, its stream buffer, its own size and its own
 * error factor -- and put the images that can share launches through ONE float-stage grid, ONE persistent launch, ONE scan and ONE pack per chunk, whatever the
 * number of distinct shapes (the decode side's counterpart: limg_hip_decode_stream_windows*, which takes any mix of streams).
 * Result: stream i is byte for byte what limg_hip_encode_stream_device writes for (pIn, sizeX, sizeY, hasAlpha, errorFactor) of item i under the same options, and
 * pBytes[i] is its totalBytes.  The result for an item does not depend on its position in the list or on what else is in the list.  Every image starts its own
 * dither chain(s); poolThreads means for each image what it means for the single call.
 * pItems is a HOST array of `count` items in both forms and may be freed or overwritten when the call returns.  itemSize = sizeof(limg_hip_stream_list_item) versions
 * the struct as struct_size does elsewhere.
 * Errors, all before anything touches the device -- a refused call writes nothing -- in this order: (1) NULL context or pItems (host form: or pBytes):
 * limg_hip_error_ArgumentNull; (2) itemSize below the struct's: limg_hip_error_InvalidParameter; (3) per item, the FIRST offending item in list order decides, and
 * within an item: NULL pIn or pStream: limg_hip_error_ArgumentNull; sizeX or sizeY 0, or limg_hip_stream_bound(sizeX, sizeY) == 0 (the single call's size bound):
 * limg_hip_error_InvalidParameter; (device form) pStream not 16-byte aligned: limg_hip_error_InvalidParameter; (device form) capacity below that bound:
 * limg_hip_error_OutOfBounds; reserved != 0: limg_hip_error_InvalidParameter; (4) count == 0: limg_hip_success with nothing done.
 * Options: forced_shift, dither_pcg, float_mode and collect_stats (limg_hip_last_stats: all images of the list together) are honoured as by
 * limg_hip_encode_stream_batch_ef_device.  batch_sub_images does NOT apply to the mixed route -- a chunk is one launch pair -- and the bytes do not depend on it.
 * Routing: an item is ELIGIBLE for the shared launches when both its sizes are multiples of 8, fastBitCrushing != 0, and force_split_kernels and legacy_float_stage
 * are off (what k_encode_list_rated asks).  Ineligible items take limg_hip_encode_stream_device, inside the same call and on the same stream: the same bytes.  Where
 * all eligible items share one shape they go to limg_hip_encode_stream_batch_ef_device's route as it is (a list of one item included).  Otherwise they go chunk by
 * chunk -- the plane batch's rule (1 GiB of block records, 32-bit strip ids) counted in blocks and strips SUMMED over the images; a chunk that holds one item takes
 * the single call -- and per chunk the call issues: the tables (kernel arguments of small launches, 3 KiB each), k_fit_tpb_list, k_encode_list_mixed,
 * k_stream_scan_strips_list, k_stream_pack_strips_list; with pBytes one gather launch and ONE download per call.
 * Context memory: what limg_hip_encode_stream_batch_ef_device holds for a chunk of the same blocks, strips and pixels (every image's factor planes are 3 slices of
 * sizeX x sizeY bytes, each rounded up to 256), and per image of the longest chunk 64 + 96 + 32 + 32 bytes of tables, 160 for its view (the persistent kernel's parameters as that image's own launch would have them) and
 * 8 for the two prefixes.  limg_hip_context_device_bytes reports all of it.
 * Ordering: calls on one context and stream execute in order and may be issued back to back without a wait.
 * Out of scope: a mixed-shape plane batch; the accurate search in the shared launch; version 2 streams; the CLI. */
typedef struct limg_hip_stream_list_item
{
  const uint32_t *pIn;      /* image i */
  uint8_t        *pStream;  /* its stream buffer */
  uint64_t        capacity; /* of pStream */
  uint32_t        sizeX, sizeY;
  uint32_t        errorFactor;
  uint32_t        reserved; /* 0 */
} limg_hip_stream_list_item;  /* 40 bytes */

/* DEVICE pointers in the items (pStream 16-byte aligned, capacity >= limg_hip_stream_bound(sizeX, sizeY)), asynchronous on `stream`; with pBytes it waits. */
limg_hip_result limg_hip_encode_stream_list_device(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems /* host */, size_t itemSize, int hasAlpha,
                                                   size_t *pBytes /* host, count entries, or NULL */, int poolThreads, int fastBitCrushing, void *stream);
/* HOST pointers in the items, blocking, under the context's mutex.  pBytes required.  A capacity may be below the bound: where some item's capacity is below that
 * stream's totalBytes, all `count` sizes are reported, NO stream is written and limg_hip_error_OutOfBounds is returned. */
limg_hip_result limg_hip_encode_stream_list(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha, size_t *pBytes,
                                            int poolThreads, int fastBitCrushing);
/* ... to a quality target: the same items (each item's errorFactor is ignored), pResults[i] and stream i exactly limg_hip_encode_stream_quality_device's for item i
 * with maxErrorSum = pMaxErrorSums[i].  The rounds of limg_hip_encode_stream_quality_batch_device, each round's encode one limg_hip_encode_stream_list_device call; the
 * error launch takes jobs of any shape as it is.  Errors: (1) - (3) above, pMaxErrorSums and pResults counted among the pointers; then the bound rules and struct_size
 * of limg_hip_encode_stream_quality_batch_device; then count == 0.  The device form waits for `stream` once per round. */
limg_hip_result limg_hip_encode_stream_quality_list_device(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems /* host */, size_t itemSize,
                                                           int hasAlpha, const uint64_t *pMaxErrorSums /* host, count */, uint32_t minErrorFactor, uint32_t maxErrorFactor,
                                                           int poolThreads, int fastBitCrushing, limg_hip_quality_result *pResults /* host, count */, void *stream);
/* HOST pointers in the items, blocking; the capacity rule of limg_hip_encode_stream_list with pResults[i].bytes. */
limg_hip_result limg_hip_encode_stream_quality_list(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                                    const uint64_t *pMaxErrorSums, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                    limg_hip_quality_result *pResults);

/* ---- byte budget and size probe for a list of MIXED shapes --------------------------------------------------------------------------
 * limg_hip_encode_stream_budget_list*: pResults[i] and stream i are exactly limg_hip_encode_stream_budget_device's for item i with maxBytes = pMaxBytes[i] and the same
 * bounds, arguments and options; each item's errorFactor is ignored.  Every image runs its own search; the result for an item does not depend on its position in the
 * list or on what else is in the list.  pMaxBytes and pResults are HOST arrays of `count` entries in both forms; set struct_size in EVERY pResults[i].
 * Errors, all before anything touches the device -- a refused call writes nothing to any stream or result -- in this order: rules (1) to (3) of
 * limg_hip_encode_stream_list_device, pMaxBytes and pResults counted among the pointers; then the bound rules (odd, below 2, min > max), any pMaxBytes[i] == 0 and any
 * struct_size below the struct's, as limg_hip_encode_stream_budget_batch_device states them: limg_hip_error_InvalidParameter; then count == 0: limg_hip_success with
 * nothing done.
 * limg_hip_stream_sizes_list*: pBytes[i * factorCount + k] = the totalBytes limg_hip_encode_stream* reports for item i at pErrorFactors[k], without encoding; any factor
 * value is allowed.  Of an item only pIn, sizeX, sizeY and reserved (0) are read: pStream may be NULL, capacity and errorFactor are ignored.  pErrorFactors (factorCount
 * entries) and pBytes (count * factorCount) are HOST arrays in both forms.  Errors: the item rules above without those on pStream and capacity, pErrorFactors and pBytes
 * counted among the pointers; then factorCount == 0 or count == 0: limg_hip_success with nothing done.
 * Routing: eligibility is limg_hip_encode_stream_list's, the chunks are its chunks.  Per chunk of more than one eligible item the call issues the chunk's tables and ONE
 * k_fit_tpb_list grid (records in the context's float mode, image after image; no noise table, no park slots), one k_rate_begin_batch per 64 images, and then
 *   budget: 2 + ceil(log2(hHi - hLo)) pairs of k_rate_probe_list -- one workgroup per work strip of the chunk, the strip's image by the binary search of
 *           k_encode_list_mixed, its geometry from its table entry; the workgroups of an image whose search is over return at their first load -- and k_rate_step_batch
 *           with the chunk's image table (image i's fixed bytes are 64 + 56 x its own blocks), ONE copy of the chunk's states and ONE wait; then the chunk goes through
 *           limg_hip_encode_stream_list_device's route with each item's errorFactor replaced by the one its search chose.  pResults[i].bytes is the size the probe
 *           measured at the result, which is the stream's totalBytes.
 *   sizes:  factorCount pairs of k_rate_probe_list and the step's list form, ONE download of the chunk's count x factorCount sizes and ONE wait.
 * An ineligible item, and a chunk that holds one item, takes limg_hip_encode_stream_budget_device (sizes: limg_hip_stream_sizes_device, which has its own fallback) inside
 * the same call and on the same stream.  Eligible items that all share one shape take limg_hip_encode_stream_budget_batch_device's route with the smallest capacity as
 * capacityEach: the same results.
 * Ordering: as limg_hip_encode_stream_list_device.  The device forms SYNCHRONISE `stream` once per chunk (and once per single call) and cannot be captured into a graph.
 * Options: as the single calls.  limg_hip_last_stats after the budget entries is that of the last encode issued.
 * Context memory, on top of what the mixed-list encode of the same chunk holds: sizeof(RateDevice) + 8 = 80 bytes per image of the longest chunk (state and counter);
 * for the sizes list, which holds the probe's share of that encode only (tables, records, invN, look-back words), 8 x factorCount bytes per image of the longest chunk
 * plus 4 x factorCount.  limg_hip_context_device_bytes reports all of it.
 * Note: the chunk's final encode runs its own float stage, as the same-shape budgeted list's does; reusing the probe's records there is a follow-up.  Out of scope as
 * well: the CLI; version 2 streams; the accurate search in the shared launches; a mixed-shape plane batch. */
/* DEVICE pointers in the items (pStream 16-byte aligned, capacity >= limg_hip_stream_bound(sizeX, sizeY)); waits for `stream`. */
limg_hip_result limg_hip_encode_stream_budget_list_device(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems /* host */, size_t itemSize,
                                                          int hasAlpha, const size_t *pMaxBytes /* host, count */, uint32_t minErrorFactor, uint32_t maxErrorFactor,
                                                          int poolThreads, int fastBitCrushing, limg_hip_budget_result *pResults /* host, count */, void *stream);
/* HOST pointers in the items, blocking; the capacity rule of limg_hip_encode_stream_list with pResults[i].bytes. */
limg_hip_result limg_hip_encode_stream_budget_list(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                                   const size_t *pMaxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                   limg_hip_budget_result *pResults);
/* DEVICE images; waits for `stream`. */
limg_hip_result limg_hip_stream_sizes_list_device(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems /* host */, size_t itemSize, int hasAlpha,
                                                  const uint32_t *pErrorFactors /* host, factorCount */, size_t factorCount, size_t *pBytes /* host, count * factorCount */,
                                                  int poolThreads, int fastBitCrushing, void *stream);
/* HOST images, blocking, under the context's mutex. */
limg_hip_result limg_hip_stream_sizes_list(limg_hip_context *pCtx, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                           const uint32_t *pErrorFactors, size_t factorCount, size_t *pBytes, int poolThreads, int fastBitCrushing);

/* ---- compact stream, version 2: the merged-block encoder's rectangles --------------------------------------------------------
 * What limg_hip_blocked_encode3d computes -- the rectangles of merged 8x8 blocks, each with ONE record, ONE shift triple and its crushed factor values -- in the same
 * "LMG3" container, so that decode(blocked_encode_stream(image)) equals the pDecoded plane of `limg_blocked_encode3d_test` bit for bit.  Version 1 streams and their
 * entry points are unchanged; each decoder refuses the other version.  Layout, little endian, sections 8-byte aligned:
 *   limg_hip_stream_header, version = 2 | limg_hip_stream_rect[R], creation order | payload (8-byte words)
 * Header: the struct above with version = LIMG_HIP_STREAM_VERSION_BLOCKED, R in reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES], bit 2 of `flags`
 * (LIMG_HIP_STREAM_FLAG_MERGED) set, blocksX / blocksY as in version 1, totalBytes = 64 + 64 R + 8 payloadWords.
 * Table: one 64-byte entry per rectangle in creation order (= block-index order = dither-chain order = the order of limg_hip_blocked_regions).  The six vectors are
 * the rectangle's record (`limg_encode_3d_output` minus avg): the pass-1 fit of a single block that kept it, the re-fit over all its pixels otherwise.  `shift` as in
 * version 1, escape rule included: factor k of a 4-channel rectangle at shift 8 whose alpha normal (lane 3 of max/mag minus min/offset) is non-zero keeps its raw
 * 8-bit factor byte and sets bit 24 + k.  ox, oy, rx, ry in 8x8 blocks; every block of the image belongs to exactly one rectangle.
 * Payload of rectangle r, at `payloadWord`: field A, then B, then C.  The rectangle covers n = wpx * hpx image pixels, wpx = 8 rx and hpx = 8 ry CLIPPED to the image
 * (a rectangle that holds the last block column of an image with sizeX % 8 != 0 has wpx = 8 rx - 8 + sizeX % 8; likewise hpx).  A field of b = 8 - shift bits per
 * pixel (b = 8 when escaped; no field at shift 8 without escape) takes ceil(n b / 64) words; pixel (yy, xx) of the rectangle, i = yy * wpx + xx, sits at bit i * b
 * of the field (bit 0 = least significant bit of the first word's first byte) -- the index the reference's decoder uses (src/limg_decode.h).  Unused high bits of a
 * field's last word are 0.  A value is the dithered factor >> shift (what pFactorsK holds, >> shift), or the un-dithered factor byte where escaped.
 * On images of whole blocks n is a multiple of 64: a field is exactly n b / 64 words and every row piece of 8 pixels a run of b bytes. */
#define LIMG_HIP_STREAM_VERSION_BLOCKED 2u
#define LIMG_HIP_STREAM_RESERVED_RECTANGLES 0 /* index into limg_hip_stream_header::reserved: the rectangle count R of a version 2 stream */
#define LIMG_HIP_STREAM_FLAG_MERGED 4u        /* limg_hip_stream_header::flags bit 2: merged-block stream */

typedef struct limg_hip_stream_rect
{
  int16_t dirA_min[4], dirA_max[4], dirB_offset[4], dirB_mag[4], dirC_offset[4], dirC_mag[4];
  uint32_t shift;       /* shiftA | shiftB << 8 | shiftC << 16 | rawEscapeMask << 24 */
  uint32_t payloadWord; /* first payload word of this rectangle */
  uint16_t ox, oy, rx, ry; /* origin and size in 8x8 blocks */
} limg_hip_stream_rect; /* 64 bytes */

/* Worst case (every block its own rectangle): 64 + blocks * 64 + blocks * 192 bytes; 0 where limg_hip_stream_bound is 0 or a dimension exceeds 65535 blocks. */
size_t limg_hip_blocked_stream_bound(size_t sizeX, size_t sizeY);
/* The merged-block encoder (same pipeline as limg_hip_blocked_encode3d_device up to its store step, float_mode always EXACT; forced_shift, dither_pcg and
 * collect_stats are honoured) in a compact mode that stores no plane, followed by a device-side scan over the rectangles' field sizes (payloadWord, header, totalBytes)
 * and the bit packer.  Argument and alignment rules of limg_hip_encode_stream_device: DEVICE pointers, pStream 16-byte aligned, capacity >= the bound; pBytes (host,
 * may be NULL) makes the call wait for the stream.  limg_hip_blocked_regions / _timing / _kernel_timing describe this encode afterwards; the scan + pack kernels count
 * into slot [3] of limg_hip_blocked_kernel_timing.  Context memory beyond that of limg_hip_blocked_encode3d_device: 4 bytes per block. */
limg_hip_result limg_hip_blocked_encode_stream_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream,
                                                      size_t capacity, size_t *pBytes, uint32_t errorFactor, int fastBitCrushing, void *stream);
/* DEVICE pointers (16-byte aligned), asynchronous.  Two launches: the rectangle table is validated and scattered into a block -> rectangle map (every rectangle inside
 * the block grid, every block covered exactly once, R <= blocks, every payload offset inside the payload), then a raster decode.  A stream that fails any of it is
 * refused as a whole -- pOut is not written -- and limg_hip_check_device_status reports limg_hip_error_InvalidParameter, once.  sizeX / sizeY must match the header. */
limg_hip_result limg_hip_blocked_decode_stream_device(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t sizeX, size_t sizeY,
                                                      void *stream);
/* HOST-pointer variants (blocking, under the context's mutex; *pBytes / limg_hip_error_OutOfBounds as limg_hip_encode_stream). */
limg_hip_result limg_hip_blocked_encode_stream(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                               size_t *pBytes, uint32_t errorFactor, int fastBitCrushing);
limg_hip_result limg_hip_blocked_decode_stream(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, uint32_t *pOut, size_t outPixels);
/* The version 2 stream of the context's LAST merged-block encode -- limg_hip_blocked_encode3d* (the planes) or limg_hip_blocked_encode_stream* -- without encoding
 * again: that encode's rectangles, records, shift words, factor and noise bytes stay in the context until its next merged-block encode, and this call runs the scan and the
 * packer over them (what tools/limg_hip_cli.cpp --blocked-stream writes next to the planes).  HOST pointer, blocking, under the context's mutex; the caller keeps other
 * threads from encoding on the context in between.  limg_hip_error_InvalidParameter if there is no such encode; *pBytes / limg_hip_error_OutOfBounds as above. */
limg_hip_result limg_hip_blocked_last_stream(limg_hip_context *pCtx, uint8_t *pStream, size_t capacity, size_t *pBytes);
/* Host-only: validates a version 2 header (first 64 bytes suffice) and reports the image shape and the rectangle count.  limg_hip_stream_info refuses version 2. */
limg_hip_result limg_hip_blocked_stream_info(const uint8_t *pStream, size_t streamBytes, size_t *pSizeX, size_t *pSizeY, int *pHasAlpha, size_t *pTotalBytes,
                                             size_t *pRectangles);

/* ---- window decode: any pixel rectangle of a stream, either version -----------------------------------------------------------
 * The table gives every block (version 1) or rectangle (version 2) its own payloadWord, so a region of the image decodes without the rest.
 * Result: pOut[r * outStridePixels + c] = pixel (x0 + c, y0 + r) of what the version's full decoder writes, for 0 <= r < height, 0 <= c < width, bit for bit.
 * NOTHING ELSE IS WRITTEN: not the outStridePixels - width pixels behind each row, not anything beyond the last row -- pOut may be a slice of a larger buffer
 * (a tile atlas, a batch tensor).
 * Window: any pixel rectangle inside the image; x0, y0, width, height need not be multiples of 8, and the window may cover the partial edge blocks of an image
 * whose size is not in whole blocks.
 * Errors, in this order: NULL context or pointer: limg_hip_error_ArgumentNull (before anything touches the device); width == 0, height == 0 or
 * outStridePixels < width: limg_hip_error_InvalidParameter; a window that is not inside sizeX x sizeY: limg_hip_error_OutOfBounds.
 * Alignment: pStream 16 bytes, as for the full decoders; pOut 4 bytes only.  A block row piece of 8 pixels leaves as two 16-byte stores where pOut is 16-byte aligned
 * and outStridePixels and x0 are multiples of 4, otherwise as dword stores -- identical results.
 * Validation: the header against the call's geometry and streamBytes, exactly as the full decoders.
 *   Version 1: every table entry the window reads is checked as the full decoder checks its groups of 8 blocks: offsets in 64 bits, inside the payload, a
 *   group's run no longer than 8 x 24 words.  A group that fails stores nothing (the other groups do), as in the full decoder.
 *   Version 2: the WHOLE rectangle table is scanned (64 bytes per rectangle): every rectangle's geometry, shifts and payload extent are checked as by the full decoder,
 *   and every block of the window must be claimed by exactly one rectangle.  Overlaps that lie wholly outside the window are NOT detected.  A stream that fails
 *   is refused as a whole: nothing is written.
 *   Either way limg_hip_check_device_status reports limg_hip_error_InvalidParameter, once.
 * Cost: table entries and payload read, pixels stored and context memory are functions of the window's block range bx0 = x0 / 8 .. (x0 + width - 1) / 8 (likewise
 * in y), not of the image -- with the one exception of version 2's table scan.  Version 2's block -> rectangle map covers the window's blocks only (4 bytes each).
 * Thread safety as for the family: the _device forms are asynchronous on `stream` and want one context per HIP stream; the host forms block and take the context's mutex. */
/* DEVICE pointers, asynchronous on `stream`.  sizeX / sizeY must match the header. */
limg_hip_result limg_hip_decode_stream_window_device(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0, size_t y0,
                                                     size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, void *stream);
limg_hip_result limg_hip_blocked_decode_stream_window_device(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0,
                                                             size_t y0, size_t width, size_t height, uint32_t *pOut, size_t outStridePixels, void *stream);
/* HOST pointers, blocking, under the context's mutex.  The image size comes from the header (limg_hip_stream_info / limg_hip_blocked_stream_info).  The whole stream
 * is uploaded, the window is decoded into context staging (4 bytes per window pixel), the status is checked, and only then are the window's rows copied into the caller's
 * stride: a refused stream leaves pOut untouched, in both versions. */
limg_hip_result limg_hip_decode_stream_window(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height,
                                              uint32_t *pOut, size_t outStridePixels);
limg_hip_result limg_hip_blocked_decode_stream_window(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height,
                                                      uint32_t *pOut, size_t outStridePixels);

/* ---- batched window decode: many windows of many streams per call ---------------------------------------------------------------
 * One window is a few workgroups: a 256 x 256 window fills a few percent of the device, and version 2 scans the whole rectangle table for it.  Callers that cut
 * many tiles out of a stream, or one crop out of each of many streams, hand all of them to one call.
 * Result: job i writes exactly what the single-window _device entry of that version writes for the same arguments, bit for bit, and nothing else: the rules above
 * for the stride slack, the rows beyond the window, unaligned pOut and partial edge blocks hold per job, and so does the choice between 16-byte and dword stores.
 * Jobs are independent: they may name different streams, image sizes and channel counts, and several may name the same stream.  Each entry takes ONE stream version;
 * a job whose stream is the other version is a header mismatch for that job.  Output rectangles of different jobs that overlap are not checked: which job's pixels
 * land there is unspecified.
 * Errors, before anything touches the device: NULL context or pJobs / pWindows: limg_hip_error_ArgumentNull; count == 0: limg_hip_error_InvalidParameter; then the jobs
 * in index order, each by the single-window entry's rules in its order.  The first failing job's error is returned and NOTHING IS ENQUEUED: no job writes anything, not
 * even those before it.  A list whose summed window blocks or work units do not fit in 32 bits: limg_hip_error_InvalidParameter.
 * Validation on the device: every job exactly as the single-window kernels validate it, and a refused job never changes what another job writes.
 *   Version 1: a group of 8 blocks that fails stores nothing; the job's other groups are stored.
 *   Version 2: a job whose stream's table fails anywhere, or whose window is not claimed exactly once, writes nothing.  Overlaps wholly outside a job's window do not
 *   concern that job.
 *   pJobStatus: DEVICE pointer to `count` words, or NULL.  Every call overwrites it for every job: 0 = decoded, otherwise the job's status bits (bit 0 header
 *   mismatch, bit 1 table or payload inconsistent).  The context's sticky status is raised as well: limg_hip_check_device_status reports
 *   limg_hip_error_InvalidParameter, once.
 * Cost: version 1 is ONE kernel launch per call, version 2 TWO, whatever `count` is.  Table entries and payload read and pixels stored are the sums over the jobs'
 * block ranges.  Version 2 scans each distinct stream's rectangle table ONCE per call: jobs with the same pStream, streamBytes, sizeX and sizeY form a group, a
 * rectangle is checked once per group and offered to every window of the group.  Context memory: the job table (about 128 bytes per job), version 2's map (4 bytes
 * per window block, summed over the jobs) and a few words of state per job -- per call in flight, four at most.
 * Ordering: calls on one context and stream execute in order.  A call's job table lives in context-owned memory of its own until the call has run, so further calls
 * may be issued before it has; the fifth call in flight waits on the host for the first.  These entries must not be used while `stream` is being captured into a graph. */
typedef struct limg_hip_window /* one window and where it goes */
{
  size_t x0, y0, width, height; /* pixels, inside the image, not empty */
  uint32_t *pOut;               /* pixel (x0 + c, y0 + r) at pOut[r * outStridePixels + c] */
  size_t outStridePixels;
} limg_hip_window;

typedef struct limg_hip_window_job /* one window of one stream */
{
  const uint8_t *pStream; /* DEVICE, 16-byte aligned */
  size_t streamBytes;
  size_t sizeX, sizeY;    /* must match the stream's header */
  limg_hip_window window; /* pOut: DEVICE, 4-byte aligned */
} limg_hip_window_job;

/* DEVICE pointers inside the jobs; pJobs itself is HOST memory and may be reused or freed when the call returns.  Asynchronous on `stream`. */
limg_hip_result limg_hip_decode_stream_windows_device(limg_hip_context *pCtx, const limg_hip_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream);
limg_hip_result limg_hip_blocked_decode_stream_windows_device(limg_hip_context *pCtx, const limg_hip_window_job *pJobs, size_t count, uint32_t *pJobStatus, void *stream);
/* HOST pointers, blocking, under the context's mutex: `count` windows of ONE stream.  The image size comes from the header; the stream is uploaded ONCE; all windows
 * decode in one batched call into context staging (4 bytes per window pixel, summed); the status is checked, and only then is each window copied into its stride: a
 * stream refused for any window leaves EVERY pOut untouched, in both versions. */
limg_hip_result limg_hip_decode_stream_windows(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_window *pWindows, size_t count);
limg_hip_result limg_hip_blocked_decode_stream_windows(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_window *pWindows, size_t count);

/* ---- stream error inside the decode: a window of a stream against an original, without the decoded image ------------------------
 * "How good is this stream?" -- the reference's answer is limg_compare, the perceptual RGB(A) PSNR of its tool -- used to take a full decode (4 bytes per pixel stored)
 * and limg_hip_compare_device (8 bytes per pixel read).  These entries are the batched window decode with a sink instead of a store: the decoded pixels never leave the
 * registers, the original's pixels are read where the decoded ones would have been written, and one integer per job is all that is written.
 * Result: let P(x, y) be the pixel the version's full decoder writes and O(x, y) = pOriginal[(y - y0) * originalStridePixels + (x - x0)].  pErrorSums[i] is the sum over
 * the window's pixels of the reference's colour error between P and O, exactly what limg_hip_compare_device adds per pixel: with the byte differences r, g, b, a
 *     r^2 * (r^2 < 0x4000 ? 2 : 3) + g^2 * 4 + b^2 * (r^2 < 0x4000 ? 3 : 2) + (a^2 * 3 where the STREAM's header says 4 channels)
 * It is an exact integer sum, so it does not depend on the order the device adds in; over the window (0, 0, sizeX, sizeY) it is mse * sizeX * sizeY of
 * limg_hip_compare(original, decode(stream)) with hasAlpha = (channels == 4), and "PSNR >= target" is pErrorSums[i] <= limg_hip_error_sum_for_psnr(...).
 * The call zeroes the `count` sums on `stream` in front of its launch.  NOTHING ELSE IS WRITTEN: no decoded pixel, no scratch image; the originals are only read, and
 * only at the window's pixels (never in the stride slack).  Load width: a block row piece of 8 pixels that lies wholly inside the window is read as two 16-byte loads
 * where pOriginal is 16-byte aligned and originalStridePixels and x0 are multiples of 4, else pixel by pixel -- the store rule of the batched window decode.
 * Full scale only: there is no level and no resize.
 * Jobs, checks and refusals are the batched window decode's: jobs are independent and may name different streams; every job is checked on the host, in index order and by
 * the single-window entry's rules in its order, with pOriginal in pOut's place (NULL: limg_hip_error_ArgumentNull; not 4-byte aligned or originalStridePixels < width:
 * limg_hip_error_InvalidParameter; a window outside the image: limg_hip_error_OutOfBounds), NULL pErrorSums counting as a NULL pointer of the call and count == 0 as
 * limg_hip_error_InvalidParameter; a refused call enqueues nothing and leaves the sums untouched.  Each entry takes ONE stream version.
 * Validation on the device is the window decode's.  A job that is refused there (bit 0 header mismatch, bit 1 table entry or payload extent inconsistent) raises
 * pJobStatus[i] and the context's sticky status; what it contributes to its own sum is then unspecified (version 1 leaves out the groups of 8 blocks that failed,
 * version 2 the whole job) and pErrorSums[i] is MEANINGLESS.  No other job's sum changes.
 * Cost: version 1 is ONE kernel launch per call, version 2 TWO (k_bstream_windows_map as it is), and one memset.  A wave adds its lanes' sums up once per work unit
 * and issues one 64-bit atomic per run of units of the same job; the runs its loop ends in leave with those of its workgroup's other waves, one atomic per job.  Memory read: the windows' table entries and payload and 4 bytes per window pixel of the originals.
 * Ordering and context memory: the batched window decode's (the job table in the ring of four slots); these entries must not be used while `stream` is being captured. */
typedef struct limg_hip_error_window /* one window and the original it is compared with */
{
  size_t x0, y0, width, height; /* pixels, inside the image, not empty */
  const uint32_t *pOriginal;    /* the original's pixel for image pixel (x0 + c, y0 + r) at pOriginal[r * originalStridePixels + c]; read only */
  size_t originalStridePixels;  /* >= width */
} limg_hip_error_window;

typedef struct limg_hip_error_window_job /* one window of one stream */
{
  const uint8_t *pStream; /* DEVICE, 16-byte aligned */
  size_t streamBytes;
  size_t sizeX, sizeY;    /* must match the stream's header */
  limg_hip_error_window window; /* pOriginal: DEVICE, 4-byte aligned */
} limg_hip_error_window_job;

/* DEVICE pointers inside the jobs and for pErrorSums (count x uint64_t) and pJobStatus (count words, or NULL); pJobs itself is HOST memory and may be reused or freed when
 * the call returns.  Asynchronous on `stream`. */
limg_hip_result limg_hip_decode_stream_windows_error_device(limg_hip_context *pCtx, const limg_hip_error_window_job *pJobs, size_t count, uint64_t *pErrorSums,
                                                            uint32_t *pJobStatus, void *stream);
limg_hip_result limg_hip_blocked_decode_stream_windows_error_device(limg_hip_context *pCtx, const limg_hip_error_window_job *pJobs, size_t count, uint64_t *pErrorSums,
                                                                    uint32_t *pJobStatus, void *stream);
/* HOST pointers, blocking, under the context's mutex: `count` windows of ONE stream.  The image size comes from the header; the stream is uploaded ONCE; every window's
 * original is staged densely (4 bytes per window pixel, summed); the status is checked before any sum is handed back: a stream refused for any window leaves pErrorSums
 * (host, count) untouched, in both versions. */
limg_hip_result limg_hip_decode_stream_windows_error(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_error_window *pWindows, size_t count,
                                                     uint64_t *pErrorSums);
limg_hip_result limg_hip_blocked_decode_stream_windows_error(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_error_window *pWindows,
                                                             size_t count, uint64_t *pErrorSums);
/* The whole image: HOST pointers, blocking; takes either stream version by its header.  Returns the value, *pMse and *pMax (either may be NULL) of
 * limg_hip_compare(pOriginal, decode(pStream), sizeX, sizeY, channels == 4) with the size and channel count of the header; `pixels` must be sizeX * sizeY.  NaN on any
 * refusal (a NULL pointer, a header that is not a stream's, pixels that do not match, a stream refused on the device). */
double limg_hip_stream_compare(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const uint32_t *pOriginal, size_t pixels, double *pMse, double *pMax);
/* Host only, no context: floor(255^2 * (hasAlpha ? 12 : 9) * sizeX * sizeY / 10^(psnr / 10)), the largest error sum whose PSNR by limg_hip_compare_device's constants is
 * at least `psnr` dB.  0 for a NaN or an empty size; saturates at UINT64_MAX (psnr = -inf). */
uint64_t limg_hip_error_sum_for_psnr(size_t sizeX, size_t sizeY, int hasAlpha, double psnr);

/* ---- batched window decode into planar float tensors ---------------------------------------------------------------------------
 * The crop + normalise + layout step of an image loader, fused into the decode: every job's window leaves as `planes` planes of float32 or float16 instead of packed
 * RGBA8, so a batch tensor N x C x h x w is filled by one call, without the RGBA intermediate and the pass over it.  One format per call, many jobs per call.
 * Result: let P(x, y) be the pixel the version's full decoder writes.  Element (c, r, col) of job i, for c < planes, r < height, col < width, is
 *     v = (float)((P(x0 + col, y0 + r) >> 8c) & 0xFF) * scale[c] + bias[c]
 * evaluated in float32 as one multiply, then one add, each rounded on its own (no fused multiply-add); stored as is for LIMG_HIP_TENSOR_F32, converted with
 * round-to-nearest-even for LIMG_HIP_TENSOR_F16.  numpy gives the same bits: (b.astype(float32) * float32(scale)) + float32(bias), then .astype(float16).
 * NOTHING ELSE IS WRITTEN: not the rowStride - width elements behind a row, not the gap between planes, no plane at or beyond `planes`, nothing beyond the last row.
 * Store width: a block row piece of 8 pixels that lies wholly inside the window leaves as 16-byte stores per plane -- two for F32 where pOut is 16-byte aligned and
 * rowStride, planeStride and x0 are multiples of 4; one for F16 where pOut is 16-byte aligned and the three are multiples of 8 -- otherwise element by element, with
 * identical results.
 * Errors, before anything is enqueued, in this order: NULL context, pJobs / pWindows or pFormat: limg_hip_error_ArgumentNull; count == 0: limg_hip_error_InvalidParameter;
 * an unknown `type`, or `planes` not 3 or 4: limg_hip_error_InvalidParameter; then the jobs in index order, each by the single-window entry's rules in its order, where
 * rowStride < width or planeStride < (height - 1) * rowStride + width takes the place of outStridePixels < width, and pOut must be aligned to the element size
 * (4 / 2 bytes).  The first failing job's error is returned and nothing is enqueued for any job.
 * Everything else is the batched window decode's, unchanged: validation on the device and what a refused job or group stores, per version; pJobStatus and the sticky
 * status; ONE launch for version 1 and TWO for version 2 whatever `count` is; version 2 scans each distinct stream's table once per call; ordering, the four calls
 * in flight, and not during graph capture. */
#define LIMG_HIP_TENSOR_F32 0u
#define LIMG_HIP_TENSOR_F16 1u

typedef struct limg_hip_tensor_format
{
  uint32_t type;   /* LIMG_HIP_TENSOR_F32 / LIMG_HIP_TENSOR_F16 */
  uint32_t planes; /* 3 or 4: plane c holds byte c of the decoded pixel (R, G, B[, byte 3]) */
  float scale[4], bias[4];
} limg_hip_tensor_format;

typedef struct limg_hip_tensor_window /* one window and where it goes */
{
  size_t x0, y0, width, height;  /* pixels, inside the image, not empty */
  void *pOut;                    /* element (c, r, col) at pOut[c * planeStride + r * rowStride + col], in elements of the format's type */
  size_t rowStride, planeStride; /* in elements */
} limg_hip_tensor_window;

typedef struct limg_hip_tensor_window_job /* one window of one stream */
{
  const uint8_t *pStream; /* DEVICE, 16-byte aligned */
  size_t streamBytes;
  size_t sizeX, sizeY;    /* must match the stream's header */
  limg_hip_tensor_window window; /* pOut: DEVICE, aligned to the element size */
} limg_hip_tensor_window_job;

/* DEVICE pointers inside the jobs; pJobs and pFormat are HOST memory and may be reused or freed when the call returns.  Asynchronous on `stream`. */
limg_hip_result limg_hip_decode_stream_windows_tensor_device(limg_hip_context *pCtx, const limg_hip_tensor_window_job *pJobs, size_t count,
                                                             const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream);
limg_hip_result limg_hip_blocked_decode_stream_windows_tensor_device(limg_hip_context *pCtx, const limg_hip_tensor_window_job *pJobs, size_t count,
                                                                     const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream);
/* HOST pointers, blocking, under the context's mutex: `count` windows of ONE stream, as limg_hip_decode_stream_windows.  Context staging takes planes x element size
 * per window pixel, summed; a stream refused for any window leaves EVERY pOut untouched, in both versions. */
limg_hip_result limg_hip_decode_stream_windows_tensor(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_tensor_window *pWindows,
                                                      size_t count, const limg_hip_tensor_format *pFormat);
limg_hip_result limg_hip_blocked_decode_stream_windows_tensor(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_tensor_window *pWindows,
                                                              size_t count, const limg_hip_tensor_format *pFormat);

/* ---- reduced-scale window decode: 1/2, 1/4, 1/8 windows, RGBA8 or planar float tensors -----------------------------------------
 * What libjpeg's scale_num / 8 is to a JPEG: a loader that wants a 224 x 224 sample out of a 1792 x 1792 crop, or a viewer that wants level 3 of a pyramid, gets it
 * from the decode itself, without the full-resolution intermediate and the pass that shrinks it.  Every job carries its own level log2Scale = L in {0, 1, 2, 3},
 * k = 1 << L; the format and the encoder do not change.
 * Reduced image: let P(x, y) be the pixel the version's full decoder writes for an image of sizeX x sizeY.  The level-L image has size RX = sizeX >> L, RY = sizeY >> L:
 * trailing source columns and rows that do not fill a box are dropped.
 * Reduced pixel: for each byte c = 0 .. 3 independently, with no alpha weighting,
 *     Q_L(X, Y).byte[c] = (sum over 0 <= i, j < k of byte c of P(k X + i, k Y + j) + (k k >> 1)) >> 2L
 * in integer arithmetic: the mean of the k x k box, round half up.  L = 0 is P itself.
 * Window: x0, y0, width, height are in level-L coordinates, inside RX x RY, not empty, and need not be aligned to anything.
 * RGBA form: pOut[r * outStridePixels + c] = Q_L(x0 + c, y0 + r).
 * Tensor form: element (c, r, col) = (float)Q_L(x0 + col, y0 + r).byte[c] * scale[c] + bias[c], evaluated and rounded exactly as the tensor entries above state it: the
 * result is their conversion applied to the RGBA form's result.
 * NOTHING ELSE IS WRITTEN: per job the rules above for the stride slack, the gap between planes, planes at or beyond `planes` and the rows beyond the window.
 * Store width: a reduced block row piece is 8 >> L pixels.  A piece of exactly 16 bytes -- level 1, RGBA8 or F32 -- that lies wholly inside the window leaves as one
 * 16-byte store where pOut is 16-byte aligned and the strides and x0 (level coordinates) are multiples of 4; every other piece (level 1 F16, levels 2 and 3, pieces
 * across the window's edge, other alignments) leaves element by element.  Level 0 jobs follow the rules of the entries above.  Identical results either way.
 * Errors: the list and the order of the batched entries above (the tensor entries' for the tensor forms), plus: log2Scale > 3 is limg_hip_error_InvalidParameter,
 * checked where the job's zero width or height is; a window that is not inside RX x RY is limg_hip_error_OutOfBounds -- any window when RX or RY is 0, that is on an
 * image smaller than k.  The first failing job's error is returned and nothing is enqueued.
 * Validation on the device, pJobStatus and the sticky status are the batched window decode's, stated on the job's source footprint (k x0, k y0, k width, k height):
 * version 1: a group of 8 blocks that fails stores none of its output pixels, the job's other groups are stored; version 2: a job refused by the map kernel writes
 * nothing.
 * Cost and call rules, unchanged: ONE launch for version 1 and TWO for version 2 whatever `count` and whatever mix of levels; version 2 scans each distinct stream's
 * table once per call; four calls in flight; not during graph capture.  Table entries and payload read are those of the footprint's block range; pixels stored are the
 * window's (1 / 64 of the footprint's at level 3). */
typedef struct limg_hip_scaled_window /* limg_hip_window and the level */
{
  size_t x0, y0, width, height; /* level-L pixels, inside (sizeX >> L) x (sizeY >> L), not empty */
  uint32_t *pOut;               /* Q_L(x0 + c, y0 + r) at pOut[r * outStridePixels + c] */
  size_t outStridePixels;
  uint32_t log2Scale;           /* L: 0 .. 3 */
} limg_hip_scaled_window;

typedef struct limg_hip_scaled_window_job /* one window of one stream */
{
  const uint8_t *pStream; /* DEVICE, 16-byte aligned */
  size_t streamBytes;
  size_t sizeX, sizeY;    /* must match the stream's header */
  limg_hip_scaled_window window; /* pOut: DEVICE, 4-byte aligned */
} limg_hip_scaled_window_job;

typedef struct limg_hip_scaled_tensor_window /* limg_hip_tensor_window and the level */
{
  size_t x0, y0, width, height;  /* level-L pixels, inside (sizeX >> L) x (sizeY >> L), not empty */
  void *pOut;                    /* element (c, r, col) at pOut[c * planeStride + r * rowStride + col], in elements of the format's type */
  size_t rowStride, planeStride; /* in elements */
  uint32_t log2Scale;            /* L: 0 .. 3 */
} limg_hip_scaled_tensor_window;

typedef struct limg_hip_scaled_tensor_window_job /* one window of one stream */
{
  const uint8_t *pStream; /* DEVICE, 16-byte aligned */
  size_t streamBytes;
  size_t sizeX, sizeY;    /* must match the stream's header */
  limg_hip_scaled_tensor_window window; /* pOut: DEVICE, aligned to the element size */
} limg_hip_scaled_tensor_window_job;

/* DEVICE pointers inside the jobs; pJobs and pFormat are HOST memory and may be reused or freed when the call returns.  Asynchronous on `stream`. */
limg_hip_result limg_hip_decode_stream_windows_scaled_device(limg_hip_context *pCtx, const limg_hip_scaled_window_job *pJobs, size_t count, uint32_t *pJobStatus,
                                                             void *stream);
limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_device(limg_hip_context *pCtx, const limg_hip_scaled_window_job *pJobs, size_t count, uint32_t *pJobStatus,
                                                                     void *stream);
limg_hip_result limg_hip_decode_stream_windows_scaled_tensor_device(limg_hip_context *pCtx, const limg_hip_scaled_tensor_window_job *pJobs, size_t count,
                                                                    const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream);
limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_tensor_device(limg_hip_context *pCtx, const limg_hip_scaled_tensor_window_job *pJobs, size_t count,
                                                                            const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream);
/* HOST pointers, blocking, under the context's mutex: `count` windows of ONE stream, every window at its own level -- all levels of a pyramid, or all tiles of one
 * level, from one upload and one batched call.  Staging as in the host forms above, per reduced window pixel; a stream refused for any window leaves EVERY pOut untouched,
 * in both versions. */
limg_hip_result limg_hip_decode_stream_windows_scaled(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_window *pWindows,
                                                      size_t count);
limg_hip_result limg_hip_blocked_decode_stream_windows_scaled(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_scaled_window *pWindows,
                                                              size_t count);
limg_hip_result limg_hip_decode_stream_windows_scaled_tensor(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes,
                                                             const limg_hip_scaled_tensor_window *pWindows, size_t count, const limg_hip_tensor_format *pFormat);
limg_hip_result limg_hip_blocked_decode_stream_windows_scaled_tensor(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes,
                                                                     const limg_hip_scaled_tensor_window *pWindows, size_t count, const limg_hip_tensor_format *pFormat);

/* ---- resized window decode: any source rectangle to any output size, inside the decode ------------------------------------------
 * RandomResizedCrop plus horizontal flip of a training loader, a thumbnail or a viewer tile of a given pixel size: every job names a SOURCE rectangle in
 * full-resolution pixels (x0, y0, width, height: inside the image, not empty) and writes outWidth x outHeight pixels, smaller or larger than the rectangle and with
 * an aspect ratio of its own; flags bit 0 (LIMG_HIP_RESIZE_FLIP_X) mirrors the output horizontally, every other bit must be 0.
 * Level: log2Scale is L = 0 .. 3, or LIMG_HIP_RESIZE_AUTO: the largest L <= 3 with (width >> L) >= outWidth and (height >> L) >= outHeight, 0 if there is none -- the
 * deepest box level that still leaves at least one level pixel per output pixel on both axes.
 * Result: let Q_L be the level-L image of the reduced-scale entries above (byte-wise box mean of the full decode, round half up, RX = sizeX >> L, RY = sizeY >> L).
 * Per axis (x shown; y is the same with y0, height, outHeight, RY and no flip), for output column X, in integers -- the product in unsigned 64 bits, floor division,
 * arithmetic shifts on signed 64 bits afterwards:
 *     Xs  = flip ? outWidth - 1 - X : X
 *     c16 = (x0 << 16) + (((2 Xs + 1) * width) << 15) / outWidth      sample centre, full resolution, 16.16
 *     u16 = (c16 >> L) - 32768                                        in level-L pixel-centre coordinates
 *     i0  = u16 >> 16 ;  f = ((u16 & 0xFFFF) + 128) >> 8              f in 0 .. 256
 *     lo  = x0 >> L ;  hi = min((x0 + width - 1) >> L, RX - 1)
 *     a   = clamp(i0, lo, hi) ;  b = clamp(i0 + 1, lo, hi)
 * With (a, b, f) of the column and (ya, yb, g) of the row, per byte c:
 *     top = Q_L(a, ya)[c] * (256 - f) + Q_L(b, ya)[c] * f
 *     bot = Q_L(a, yb)[c] * (256 - f) + Q_L(b, yb)[c] * f
 *     R(X, Y)[c] = (top * (256 - g) + bot * g + 32768) >> 16
 * that is align_corners = false bilinear on the level-L image, clamped to the level pixels the rectangle touches, with no alpha weighting.  Consequences: with
 * outWidth == width, outHeight == height, L = 0 and no flip R is the window itself, bit for bit; with x0, y0, width, height multiples of k = 1 << L and
 * outWidth == width / k, outHeight == height / k it is that window of Q_L (and AUTO picks that L); the flip is exactly the column reversal.  Against exact bilinear
 * interpolation at level 0 the result deviates by less than 1.52 byte steps (weights rounded to 1 / 256: 1 / 512 plus two floors of 2^-16 per axis, 0.5 for the end).
 * RGBA form: pOut[Y * outStridePixels + X] = R(X, Y).  Tensor form: the tensor entries' conversion applied to R's bytes (one multiply, one add, no fused multiply-add,
 * round-to-nearest-even to F16).  NOTHING ELSE IS WRITTEN, by the rules of the entries above.  Stores are element by element; 64 consecutive elements of an output
 * row leave together.
 * Errors, before anything is enqueued: the list and the order of the reduced-scale entries; log2Scale > 3 and not LIMG_HIP_RESIZE_AUTO, a flag bit other than bit 0,
 * outWidth or outHeight of 0 or above 32768: limg_hip_error_InvalidParameter, checked where a zero width or height is; the stride rules are stated on outWidth and
 * outHeight; a source rectangle that is not inside the image: limg_hip_error_OutOfBounds; an explicit level with (x0 >> L) > RX - 1 or (y0 >> L) > RY - 1 -- a
 * rectangle that starts in the trailing columns or rows the level drops, or any rectangle when RX or RY is 0 -- limg_hip_error_OutOfBounds (AUTO cannot get there).
 * The first failing job's error is returned and nothing is enqueued.
 * Validation on the device, pJobStatus and the sticky status are the batched window decode's, stated on the job's footprint (the level pixels lo .. hi of both axes,
 * times k).  Version 2: a job refused by the map kernel writes nothing.  Version 1: a job whose header fails writes nothing; where a group of 8 blocks fails the
 * job's status gets bit 1 and the output pixels with a tap in that group are unspecified (they lie inside the job's output rectangle); every output pixel whose four
 * taps lie in sound groups is correct, and other jobs are unaffected.
 * Cost and call rules: ONE launch for version 1 and TWO for version 2 whatever the count, the mix of levels, the sizes and the flips; version 2 scans each distinct
 * stream's table once per call; four calls in flight; not during graph capture.  There is no full-resolution and no crop-sized intermediate in device memory: a
 * workgroup decodes an output tile's footprint into on-chip memory and resamples from there (blocks on a tile's border are decoded by both neighbours).  Context
 * memory per job: the batched entries' and 64 bytes more. */
#define LIMG_HIP_RESIZE_AUTO 0xFFFFFFFFu
#define LIMG_HIP_RESIZE_FLIP_X 1u

typedef struct limg_hip_resized_window
{
  size_t x0, y0, width, height; /* SOURCE rectangle, full-resolution pixels, inside the image, not empty */
  uint32_t *pOut;               /* R(X, Y) at pOut[Y * outStridePixels + X] */
  size_t outStridePixels;       /* >= outWidth */
  size_t outWidth, outHeight;   /* 1 .. 32768 */
  uint32_t log2Scale, flags;    /* L: 0 .. 3 or LIMG_HIP_RESIZE_AUTO; LIMG_HIP_RESIZE_FLIP_X */
} limg_hip_resized_window;

typedef struct limg_hip_resized_window_job /* one window of one stream */
{
  const uint8_t *pStream; /* DEVICE, 16-byte aligned */
  size_t streamBytes;
  size_t sizeX, sizeY;    /* must match the stream's header */
  limg_hip_resized_window window; /* pOut: DEVICE, 4-byte aligned */
} limg_hip_resized_window_job;

typedef struct limg_hip_resized_tensor_window
{
  size_t x0, y0, width, height;  /* SOURCE rectangle, full-resolution pixels, inside the image, not empty */
  void *pOut;                    /* element (c, Y, X) at pOut[c * planeStride + Y * rowStride + X], in elements of the format's type */
  size_t rowStride, planeStride; /* in elements: rowStride >= outWidth, planeStride >= (outHeight - 1) * rowStride + outWidth */
  size_t outWidth, outHeight;    /* 1 .. 32768 */
  uint32_t log2Scale, flags;     /* L: 0 .. 3 or LIMG_HIP_RESIZE_AUTO; LIMG_HIP_RESIZE_FLIP_X */
} limg_hip_resized_tensor_window;

typedef struct limg_hip_resized_tensor_window_job /* one window of one stream */
{
  const uint8_t *pStream; /* DEVICE, 16-byte aligned */
  size_t streamBytes;
  size_t sizeX, sizeY;    /* must match the stream's header */
  limg_hip_resized_tensor_window window; /* pOut: DEVICE, aligned to the element size */
} limg_hip_resized_tensor_window_job;

/* DEVICE pointers inside the jobs; pJobs and pFormat are HOST memory and may be reused or freed when the call returns.  Asynchronous on `stream`. */
limg_hip_result limg_hip_decode_stream_windows_resized_device(limg_hip_context *pCtx, const limg_hip_resized_window_job *pJobs, size_t count, uint32_t *pJobStatus,
                                                              void *stream);
limg_hip_result limg_hip_blocked_decode_stream_windows_resized_device(limg_hip_context *pCtx, const limg_hip_resized_window_job *pJobs, size_t count, uint32_t *pJobStatus,
                                                                      void *stream);
limg_hip_result limg_hip_decode_stream_windows_resized_tensor_device(limg_hip_context *pCtx, const limg_hip_resized_tensor_window_job *pJobs, size_t count,
                                                                     const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream);
limg_hip_result limg_hip_blocked_decode_stream_windows_resized_tensor_device(limg_hip_context *pCtx, const limg_hip_resized_tensor_window_job *pJobs, size_t count,
                                                                             const limg_hip_tensor_format *pFormat, uint32_t *pJobStatus, void *stream);
/* HOST pointers, blocking, under the context's mutex: `count` windows of ONE stream from one upload and one batched call.  Staging as in the host forms above, per
 * OUTPUT pixel (outWidth x outHeight); a stream refused for any window leaves EVERY pOut untouched, in both versions. */
limg_hip_result limg_hip_decode_stream_windows_resized(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_resized_window *pWindows,
                                                       size_t count);
limg_hip_result limg_hip_blocked_decode_stream_windows_resized(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, const limg_hip_resized_window *pWindows,
                                                               size_t count);
limg_hip_result limg_hip_decode_stream_windows_resized_tensor(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes,
                                                              const limg_hip_resized_tensor_window *pWindows, size_t count, const limg_hip_tensor_format *pFormat);
limg_hip_result limg_hip_blocked_decode_stream_windows_resized_tensor(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes,
                                                                      const limg_hip_resized_tensor_window *pWindows, size_t count, const limg_hip_tensor_format *pFormat);

/* ---- stream splice: a version 1 stream made from version 1 streams, on the GPU, without decoding -------------------------------------------
 * A version 1 block is self-contained: its entry holds record, shift word and payloadWord, its payload is whole 8-byte words, and no decoder needs a neighbour.
 * A rectangle of blocks of one stream can therefore be placed in the block grid of another stream by copying entries and payload and rebasing payloadWord: a
 * lossless crop (one piece), join (strips, tiles) or any mix.  decode(splice) equals the matching rectangles of decode(source) bit for bit; no factor bit changes,
 * no dither chain restarts.  Version 2 streams (rectangles that cross crop lines) are not handled.
 *
 * A PIECE is a rectangle of blocksW x blocksH blocks of a source stream from block (srcBx, srcBy), landing at block (dstBx, dstBy) of the output's grid.  Rules,
 * all decided on the host before anything is launched; a breach is limg_hip_error_InvalidParameter and nothing is written:
 *   exact cover    the pieces cover the output's blocksX x blocksY grid (of sizeX x sizeY) exactly once: no gap, no overlap; count >= 1, no piece is empty;
 *   inside         each piece lies inside its source's block grid (of srcSizeX x srcSizeY);
 *   edge rule      an output block the output size clips (last column when sizeX % 8 != 0, last row when sizeY % 8 != 0) comes from a source block clipped to
 *                  the same extent on that axis -- the source's own last column / row with the same size % 8; a whole output block comes from a whole source
 *                  block.  ("pixels outside the image are 0" then holds by copying alone; a whole block is never masked down to a partial one.)
 *   sizes          limg_hip_stream_bound(sizeX, sizeY) != 0 and the same for every source size; streamBytes holds at least the header and the source's table;
 *   device form    capacity >= limg_hip_stream_bound(sizeX, sizeY); pOut and every pStream 16-byte aligned; [pOut, pOut + capacity) overlaps no source;
 *   pieceSize      = sizeof(limg_hip_splice_piece) versions the struct, as itemSize does in the list calls: below the struct's is refused, a larger stride is walked.
 * NULL context, pPieces, pOut or a piece's pStream: limg_hip_error_ArgumentNull.  errorFactor and flags are the header's informational fields, written as given.
 *
 * The sources are untrusted, as in the decoders: the kernels check every source header (version 1, the channel count of hasAlpha, srcSizeX x srcSizeY) and that
 * every run of entries they copy is canonical -- each payloadWord the run's start plus the words of the blocks before it, the run's end inside the source's
 * payload, in 64-bit arithmetic.  A failure raises the context's status (limg_hip_check_device_status: limg_hip_error_InvalidParameter, once); nothing but the
 * 64 header bytes of pOut is written, the header comes back zeroed (totalBytes 0) and *pBytes is 0.
 *
 * The output is canonical: entries in raster order, payloadWord the exact exclusive prefix of the blocks' words, payloadWords / totalBytes set on the device;
 * every decode entry accepts it.  Three kernel launches whatever `count` is; context memory: 24 bytes per block row of a piece + 48 per piece. */
typedef struct limg_hip_splice_piece
{
  const uint8_t *pStream; /* the source stream: DEVICE pointer in the _device forms, host pointer otherwise */
  size_t streamBytes;
  uint32_t srcSizeX, srcSizeY; /* the source image's size; the kernel checks it against the header, as the decode calls do */
  uint32_t srcBx, srcBy;       /* first source block of the rectangle */
  uint32_t dstBx, dstBy;       /* where that block lands in the output's block grid */
  uint32_t blocksW, blocksH;   /* rectangle size in 8x8 blocks */
} limg_hip_splice_piece;

/* DEVICE pointers inside the pieces; pPieces is HOST memory and may be reused or freed when the call returns.  Asynchronous on `stream`; the size lands in the
 * header (`totalBytes`); pBytes (host, may be NULL) receives it too, which makes the call wait. */
limg_hip_result limg_hip_stream_splice_device(limg_hip_context *pCtx, const limg_hip_splice_piece *pPieces /* host */, size_t count, size_t pieceSize, size_t sizeX,
                                              size_t sizeY, int hasAlpha, uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes, void *stream);
/* HOST pointers, blocking, under the context's mutex.  Every source must pass limg_hip_stream_info (its error otherwise; limg_hip_error_OutOfBounds when the
 * stream is longer than streamBytes).  capacity may be below the bound: *pBytes is set, and limg_hip_error_OutOfBounds returned with nothing written, when the
 * finished stream is longer than `capacity`. */
limg_hip_result limg_hip_stream_splice(limg_hip_context *pCtx, const limg_hip_splice_piece *pPieces, size_t count, size_t pieceSize, size_t sizeX, size_t sizeY,
                                       int hasAlpha, uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes);
/* One piece from a pixel window: the stream of the width x height image at (x0, y0) of the source.  x0 and y0 must be multiples of 8; x0 + width a multiple of 8
 * or equal to sizeX, y0 + height a multiple of 8 or equal to sizeY; width, height >= 1 and the window inside the image: anything else is
 * limg_hip_error_InvalidParameter.  (An unaligned origin would need the blocks re-cut: not done.)  Otherwise the splice call's rules. */
limg_hip_result limg_hip_stream_crop_device(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, int hasAlpha, size_t x0, size_t y0,
                                            size_t width, size_t height, uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes, void *stream);
/* HOST pointers, blocking: size, channels, errorFactor and flags come from the source's header. */
limg_hip_result limg_hip_stream_crop(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height, uint8_t *pOut,
                                     size_t capacity, size_t *pBytes);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) ---------------------------------------------------------------------------------
 * The reference's only parallelism is row strips over a std::thread pool (src/limg.cpp:2105-2138); across GPUs the same strips
 * go one per rank.  Blocks are independent except for the dither chain, so the data path needs no collective in strip-restart mode (each strip
 * restarts its chain like the reference's pool strips: plain limg_hip_encode3d_device on the strip).  Two things do cross xGMI:
 *   * limg_hip_gather_stream              : reassembly of the compact streams on one rank (variable-size gather: an 8-byte all-gather of the sizes, then
 *                                           grouped ncclSend / ncclRecv of exactly the used bytes);
 *   * limg_hip_encode3d_single_chain_device: ONE dither chain through all strips in rank order, i.e. the result of the reference run with
 *                                           pThreadPool == nullptr (src/limg.cpp:1893, :2110): one 8-byte all-gather of the per-strip dither-call totals
 *                                           between the E step (fit + search) and the F step (dither + stores) of every rank.
 * RCCL is resolved at run time from the process (dlopen "librccl.so.1"): the library has no link-time dependency on it.  Failures map to
 * limg_hip_error_Generic.  The communicator belongs to the context; the caller only transports the 128-byte id from rank 0 to the others. */
#define LIMG_HIP_COMM_ID_BYTES 128
limg_hip_result limg_hip_comm_unique_id(uint8_t *pId128);                                                  /* rank 0: ncclGetUniqueId */
limg_hip_result limg_hip_comm_init(limg_hip_context *pCtx, const uint8_t *pId128, int rank, int worldSize); /* every rank: ncclCommInitRank on the context's device */
limg_hip_result limg_hip_comm_destroy(limg_hip_context *pCtx);
/* ncclCommUserRank / ncclCommCount of the context's communicator and ncclGetVersion (any pointer may be NULL): evidence for logs and bench lines. */
limg_hip_result limg_hip_comm_info(limg_hip_context *pCtx, int *pRank, int *pRanks, int *pRcclVersion);
/* pStream / pGathered are DEVICE pointers.  On `root`, piece r lands at pGathered + pOffsets[r] (16-byte aligned, ready for limg_hip_decode_stream_device);
 * pOffsets (host, worldSize + 1 entries) also receives the total.  Blocks until the sizes are known; the transfers are asynchronous on `stream`. */
limg_hip_result limg_hip_gather_stream(limg_hip_context *pCtx, const uint8_t *pStream, size_t streamBytes, int root, uint8_t *pGathered, size_t capacity,
                                       uint64_t *pOffsets, void *stream);
/* This rank's strip of `stripRows` rows (whole 8x8 blocks: sizeX, stripRows multiples of 8) of a taller image whose strips go to the ranks in order;
 * blocksBefore = number of 8x8 blocks in the strips of the ranks before this one (sizes the dither noise table).  DEVICE pointers, asynchronous. */
limg_hip_result limg_hip_encode3d_single_chain_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t stripRows, int hasAlpha,
                                                      const limg_hip_encode3d_info *pInfo, uint32_t errorFactor, int fastBitCrushing, size_t blocksBefore, void *stream);
/* Abort rule of the two collective entries (the reference's analogue, row strips on one thread pool, cannot half-fail: src/limg.cpp:2114-2136): a rank never leaves its
 * peers inside a collective.  limg_hip_gather_stream decides "fits / does not fit" from all-gathered numbers, so every rank returns limg_hip_error_OutOfBounds alike
 * before anything is posted.  limg_hip_encode3d_single_chain_device: a rank whose own E step failed (bad arguments, allocation, launch) still joins the 8-byte
 * all-gather, with the poison value ~0, and returns its error; on every other rank the call -- it is asynchronous -- returns limg_hip_success, the F step stores
 * NOTHING, and the next limg_hip_check_device_status of that context returns limg_hip_error_Generic ("a rank of the communicator aborted ..."), once. */
/* The two halves of the above without the exchange, for callers that move the counts themselves (and for single-GPU tests of the chain arithmetic):
 * phase 1 = E step + scan, writes this strip's dither-call total to *pCallsDevice; phase 2 = F step, its first dither call is *pChainBaseDevice.
 * Phase 2 must follow phase 1 of the same strip on the same context with nothing in between (the context holds the strip's intermediate results);
 * a phase 2 without that is refused with limg_hip_error_InvalidParameter. */
limg_hip_result limg_hip_encode3d_chain_device(limg_hip_context *pCtx, const uint32_t *pIn, size_t sizeX, size_t stripRows, int hasAlpha, const limg_hip_encode3d_info *pInfo,
                                               uint32_t errorFactor, int fastBitCrushing, int phase, uint64_t *pCallsDevice, const uint64_t *pChainBaseDevice,
                                               size_t blocksBefore, void *stream);
/* Host-only helpers (no GPU): the offset arithmetic of the gather (pOffsets: count + 1 entries) and the exclusive prefix of the call totals. */
limg_hip_result limg_hip_host_gather_offsets(const uint64_t *pSizes, int count, uint64_t *pOffsets);
limg_hip_result limg_hip_host_chain_bases(const uint64_t *pCalls, int count, uint64_t *pBases);

/* Introspection for the bench: names and launch count of the kernels one encode enqueues, bytes of context-owned HBM. */
size_t limg_hip_context_device_bytes(const limg_hip_context *pCtx);
const char *limg_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LIMG_HIP_H */
