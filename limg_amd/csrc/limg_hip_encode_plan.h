// limg_hip_encode_plan.h -- every decision of the 8x8 encode's host layer that needs no device, each written ONCE: the shape of an image in blocks and strips, the
// plane set of a limg_hip_encode3d_info, the 16-byte access flags, the advance of all eleven plane pointers, the dither-chain partition, "this list can go through
// one launch pair", and -- encode_plan -- which of the six launch paths a call of encode_device takes, or why it is refused, before anything is allocated or
// enqueued.  A host compiler builds it on its own (tests/helpers/encode_plan_check.cpp walks the rules' whole input space).  Plain C++: no HIP types, no library.
#ifndef LIMG_HIP_ENCODE_PLAN_H
#define LIMG_HIP_ENCODE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/limg_hip.h"

namespace limg_hip
{
  constexpr size_t kShapeBlock = 8, kShapeStripBlocks = 32; // kBlock, kStripBlocks (limg_hip_internal.h; limg_hip_context.h asserts that they agree)

  // ---- an image in 8x8 blocks and work strips (of one image) ----
  struct EncodeShape
  {
    size_t sizeX, sizeY, blocksX, blocksY, stripsX, blocks, strips;
    bool valid; // both sizes in 1 .. 2^31 - 8: every block and pixel coordinate fits 31 bits
    bool whole; // both sizes multiples of 8: no partial edge block
    EncodeShape(size_t x, size_t y)
      : sizeX(x), sizeY(y), blocksX((x + kShapeBlock - 1) / kShapeBlock), blocksY((y + kShapeBlock - 1) / kShapeBlock), stripsX((blocksX + kShapeStripBlocks - 1) / kShapeStripBlocks),
        blocks(blocksX * blocksY), strips(stripsX * blocksY), valid(x != 0 && y != 0 && x <= 0x7FFFFFF8ull && y <= 0x7FFFFFF8ull),
        whole(x % kShapeBlock == 0 && y % kShapeBlock == 0) {}
  };

  // ---- the planes of a limg_hip_encode3d_info: all eleven, or (compact mode) the three factor planes with the eight uint32 planes all NULL ----
  enum PlaneSet { kPlanesNone, kPlanesCompact, kPlanesFull, kPlanesInvalid };
  inline PlaneSet plane_set(const limg_hip_encode3d_info *info)
  {
    if (!info) return kPlanesNone;
    const void *const *pp = reinterpret_cast<const void *const *>(info); // pDecoded, pShiftABCX, pColAMin .. pColCMax, pFactorsA .. pFactorsC
    int n32 = 0;
    for (int i = 0; i < 8; i++) n32 += pp[i] != nullptr;
    for (int i = 8; i < 11; i++)
      if (!pp[i]) return kPlanesInvalid;
    return n32 == 8 ? kPlanesFull : (n32 == 0 ? kPlanesCompact : kPlanesInvalid);
  }

  // ---- 16-byte vector access straight on caller pointers only where the address is 16-byte aligned for every row: sliced or offset device pointers
  // take the dword paths.  One image; a list is the & over its images. ----
  struct VecAccess
  {
    bool in, planes, factors8, decoded, factors; // EncodeParams::vecIn, vecPlanes, vecFactors8 (8-byte), vecDecoded, vecFactors
    VecAccess &operator&=(const VecAccess &o) { in = in && o.in; planes = planes && o.planes; factors8 = factors8 && o.factors8; decoded = decoded && o.decoded; factors = factors && o.factors; return *this; }
  };
  inline VecAccess vec_access(const uint32_t *in, const limg_hip_encode3d_info *info, size_t sizeX, bool fullPlanes)
  {
    VecAccess v = { (sizeX % 4 == 0) && (((uintptr_t)in) & 15u) == 0, false, false, false, false };
    if (!info) return v;
    const uintptr_t factorBits = ((uintptr_t)info->pFactorsA) | ((uintptr_t)info->pFactorsB) | ((uintptr_t)info->pFactorsC);
    v.factors8 = (sizeX % 8 == 0) && (factorBits & 7u) == 0;
    v.factors = (sizeX % 16 == 0) && (factorBits & 15u) == 0;
    if (!fullPlanes || sizeX % 4 != 0) return v;
    uintptr_t bits = 0;
    const void *const *pp = reinterpret_cast<const void *const *>(info);
    for (int i = 1; i < 8; i++) bits |= (uintptr_t)pp[i]; // pShiftABCX .. pColCMax
    v.planes = (bits & 15u) == 0;
    v.decoded = (((uintptr_t)info->pDecoded) & 15u) == 0;
    return v;
  }

  // all eleven plane pointers `pixels` further (a sub-image that starts some rows down); NULL stays NULL
  inline void advance_planes(limg_hip_encode3d_info &info, size_t pixels)
  {
    uint32_t **words[] = { &info.pDecoded, &info.pShiftABCX, &info.pColAMin, &info.pColAMax, &info.pColBMin, &info.pColBMax, &info.pColCMin, &info.pColCMax };
    uint8_t **bytes[] = { &info.pFactorsA, &info.pFactorsB, &info.pFactorsC };
    for (uint32_t **p : words) if (*p) *p += pixels;
    for (uint8_t **p : bytes) if (*p) *p += pixels;
  }

  // ---- the dither chains of an image: src/limg.cpp:2114-2134 in block rows ----
  struct Partition { uint32_t chainCount, chainRows; };
  inline Partition partition(size_t sizeY, int poolThreads)
  {
    Partition pt = { 1, 0 };
    if (poolThreads <= 0) return pt;
    size_t thread_count = (size_t)poolThreads * 4;
    size_t y_range = ((sizeY / kShapeBlock) / thread_count) * kShapeBlock;
    if (y_range == 0)
    {
      thread_count = (size_t)poolThreads;
      y_range = ((sizeY / kShapeBlock) / thread_count) * kShapeBlock;
    }
    if (y_range == 0) return pt; // every strip but the last is empty
    pt.chainCount = (uint32_t)thread_count;
    pt.chainRows = (uint32_t)(y_range / kShapeBlock);
    return pt;
  }

  // A list of images of this shape can go through ONE launch pair (k_fit_tpb's grid over all images + one persistent launch): whole blocks, the persistent path,
  // the float stage as its own launch.  Otherwise a list is one encode per image.  (limg_hip_encode3d_batch_device adds: all eleven planes of every image.)
  inline bool list_in_one_pair(const EncodeShape &sh, const limg_hip_options &o) { return sh.whole && o.force_split_kernels == 0 && o.legacy_float_stage == 0; }

  // ---- what the choice of a launch path depends on, and nothing else ----
  struct EncodeFacts
  {
    bool nullArgument;                                // no context or no input
    size_t sizeX, sizeY;
    PlaneSet planes;
    bool callerRecords, callerShifts, recordsAligned; // compact outputs of the caller's; the address the records go to is 16-byte aligned (the context's own always is)
    int poolThreads;
    bool fast;
    Partition part;                                   // the dither chains: of this image, or of the larger one it is a part of (EncodeExtra::part)
    // EncodeExtra
    int chainPhase;
    size_t batchCount;
    bool inner, innerLast, fitOnly, fitFloatMode, streamRaw, stripWords, errorFactors, ratedTable, dPrevDesc;
    // limg_hip_options, the test hook (0 in the product) and limg_hip::checkpoint_reach()
    int32_t force_split_kernels, legacy_float_stage, dither_pcg, float_mode, collect_stats, batch_sub_images, ragged_bands, whole_image_ragged;
    size_t checkpoint_reach;
  };

  enum EncodePath
  {
    kPathHeightRagged, // whole width, partial last block row: the rows above as an image of whole blocks, the last row through the ragged path, chains joined
    kPathSubBatches,   // a list as a pipeline of launch pairs
    kPathFused,        // [k_fit_tpb +] the persistent kernel
    kPathChainPhase2,  // k_dither_store behind a chain encode's phase 1
    kPathSplit,        // [k_fit_tpb +] k_fit_search, scan, k_dither_store; also records only, nothing stored, chain phase 1
    kPathRagged        // partial edge blocks: k_fit_search, the host's chain walk, k_dither_store -- in `bands` bands of `bandRows` block rows
  };
  // how far a call gets, in the order the rules apply
  enum EncodeVerdict { kRefusedNull, kRefusedSize, kRefusedPlanes, kRefusedChain, kRefusedList, kRefusedErrorFactors, kAccepted };

  struct EncodePlan
  {
    limg_hip_result code;
    EncodeVerdict verdict;
    EncodePath path;
    size_t subImages;         // kPathSubBatches: images per launch pair
    uint32_t bands, bandRows; // kPathRagged
    bool prefit;              // the float stage as its own launch, one lane per block (k_fit_tpb): the E step starts from the records
    bool fused, floatFast, wantStats, fullPlanes, storePlanes, streamRaw, fitOnly;
    // profiling events this call records (Timeline, limg_hip_context.h): 4 a whole encode, 2 each phase of a chain encode; of a height-ragged image 3 the upper
    // rows, 0 the last row and 1 the call that runs both
    int marks;
  };

  inline EncodePlan encode_refused(EncodeVerdict v, limg_hip_result code)
  {
    EncodePlan p = {};
    p.code = code; p.verdict = v;
    return p;
  }

  inline EncodePlan encode_plan(const EncodeFacts &f)
  {
    if (f.nullArgument) return encode_refused(kRefusedNull, limg_hip_error_ArgumentNull);
    const EncodeShape sh(f.sizeX, f.sizeY);
    if (!sh.valid) return encode_refused(kRefusedSize, limg_hip_error_InvalidParameter);
    if (f.planes == kPlanesInvalid) return encode_refused(kRefusedPlanes, limg_hip_error_ArgumentNull);
    const bool stored = f.planes != kPlanesNone, ragged = !sh.whole;
    EncodePlan p = {};
    p.code = limg_hip_success; p.verdict = kAccepted;
    // An image whose WIDTH is whole blocks but whose last block row is partial (BASELINE config 1's shape class: 1024 x 618): every block row but the last
    // is on the fast path (its dither chain is the seed's orbit, the noise table applies); only the last row needs the host to walk its chain.
    if (ragged && f.sizeX % kShapeBlock == 0 && f.sizeY > kShapeBlock && stored && f.chainPhase == 0 && f.batchCount == 1 && !f.inner && !f.fitOnly &&
        f.force_split_kernels == 0 && f.legacy_float_stage == 0 && f.dither_pcg == 0 && f.whole_image_ragged == 0 && sh.blocks * 3 <= f.checkpoint_reach)
    {
      p.path = kPathHeightRagged; p.marks = 1; p.wantStats = f.collect_stats != 0; // (the two parts are calls of their own, with plans of their own)
      return p;
    }
    if (f.chainPhase != 0 && (ragged || !stored || f.poolThreads != 0)) return encode_refused(kRefusedChain, limg_hip_error_InvalidParameter); // a chain shared between GPUs: whole 8x8 blocks, one chain
    p.fullPlanes = f.planes != kPlanesCompact;
    p.storePlanes = stored;
    p.streamRaw = f.streamRaw && !p.fullPlanes;
    p.fitOnly = f.fitOnly && !stored;
    p.floatFast = f.float_mode == 1 && (!f.fitOnly || f.fitFloatMode);
    p.prefit = !ragged && f.legacy_float_stage == 0 && (!f.callerRecords || f.recordsAligned); // k_fit_tpb stores records 16 bytes at a time
    p.fused = stored && !ragged && (f.force_split_kernels == 0 || f.batchCount > 1) && f.chainPhase == 0;
    p.wantStats = f.collect_stats != 0 && stored && f.chainPhase == 0;
    p.marks = f.chainPhase != 0 ? 2 : (!f.inner ? 4 : (f.innerLast ? 0 : 3));
    // a list in compact mode only as the batched stream encode hands it over: raw-escaped factor bytes, the strips' payload words, records and shift words all in
    // raster arrays that run image after image (what its scan and packer read)
    const bool compactList = !p.fullPlanes && f.streamRaw && f.stripWords && f.callerRecords && f.callerShifts;
    // ... or for its records alone (the size probes of a budgeted list): k_fit_tpb's batched grid and nothing else
    const bool fitList = p.fitOnly && p.prefit && !ragged && f.chainPhase == 0;
    if (f.batchCount > 1 && !fitList && (!p.fused || !p.prefit || (!p.fullPlanes && !compactList)))
      return encode_refused(kRefusedList, limg_hip_error_InvalidParameter); // (limg_hip_encode3d_batch_device sends such lists through one encode per image instead)
    // ... each at its own error factor: that compact list, and the one kernel there is for it (k_encode_list_rated)
    if (f.errorFactors && (!f.ratedTable || f.batchCount <= 1 || !compactList || !p.fused || !p.prefit || !f.fast || f.chainPhase != 0))
      return encode_refused(kRefusedErrorFactors, limg_hip_error_InvalidParameter);
    // sub-batches (limg_hip_options.batch_sub_images): the option if positive; 0: 8 from 32 images on, 4 from 16 on; negative: none
    if (p.fused && p.prefit && f.batchCount > 1)
    {
      if (f.batch_sub_images > 0) p.subImages = (size_t)f.batch_sub_images;
      else if (f.batch_sub_images == 0) p.subImages = f.batchCount >= 32 ? 8 : (f.batchCount >= 16 ? 4 : 0);
      if (p.subImages >= f.batchCount) p.subImages = 0;
    }
    if (p.subImages > 0) p.path = kPathSubBatches;
    else if (p.fused) p.path = kPathFused;
    else if (f.chainPhase == 2) p.path = kPathChainPhase2;
    else if (!ragged) p.path = kPathSplit;
    else
    {
      // The walk is the floor of this class -- ~26 ms for 8190 x 8192, one dependent AESDEC chain -- so everything else is taken off its path: the E step runs in
      // BANDS of block rows whose shift words come back band by band (the walk starts when the first band is down and runs under the rest of the E step), and the F
      // step of a band is launched as soon as its chain values are up (it runs under the walk of the next band).  Only for one chain: independent chains are walked
      // in parallel instead.
      // (an explicit band count is honoured from 2 x 2 blocks on -- tests and the fuzz tool; a band must not be one block wide: the corner block of fewer than four
      //  pixels sums its LEFT neighbour's pixels, which for a one-block-wide image would be the row above, in another band)
      p.path = kPathRagged;
      const uint32_t blocksX = (uint32_t)sh.blocksX, blocksY = (uint32_t)sh.blocksY;
      uint32_t nBands = 1;
      if (stored && !f.dPrevDesc && f.part.chainCount <= 1 && f.ragged_bands >= 0 && blocksX >= 2 && blocksY >= 2 && (f.ragged_bands > 0 || (blocksX >= 32 && blocksY >= 64)))
        nBands = f.ragged_bands > 0 ? (uint32_t)f.ragged_bands : 16u;
      if (nBands > blocksY / 2) nBands = blocksY / 2 ? blocksY / 2 : 1;
      if (nBands > 64) nBands = 64;
      p.bandRows = (blocksY + nBands - 1) / nBands;
      p.bands = (blocksY + p.bandRows - 1) / p.bandRows;
    }
    return p;
  }
}

#endif
