// encode_plan_check.cpp -- limg_amd/csrc/limg_hip_encode_plan.h built by a host compiler on its own: the header's answers, one line per question.
// stdin, one question per line (every value an integer):
//   p <facts>            ->  code verdict path subImages bands bandRows prefit fused floatFast wantStats fullPlanes storePlanes streamRaw fitOnly marks
//   P <facts>            ->  the same question answered by the conditions of encode_device, encode_params, sub_batch_images and band_count as they stood before the
//                            header existed, lifted into parent_plan() below: code path subImages bands bandRows prefit fused floatFast wantStats fullPlanes storePlanes
//                            streamRaw fitOnly marks (no verdict: the old code had no such word)
//     <facts> = nullArgument sizeX sizeY planes callerRecords callerShifts recordsAligned poolThreads fast chainPhase batchCount inner innerLast fitOnly fitFloatMode
//               streamRaw stripWords errorFactors ratedTable dPrevDesc force_split_kernels legacy_float_stage dither_pcg float_mode collect_stats batch_sub_images
//               ragged_bands whole_image_ragged checkpoint_reach            (the partition is the image's own: partition(sizeY, poolThreads))
//   e sizeX sizeY        ->  blocksX blocksY stripsX blocks strips valid whole
//   s mask               ->  plane_set of an info whose pointer i (order of the struct) is there iff bit i of mask
//   v sizeX full info o0 .. o11  ->  in planes factors8 decoded factors: pointers at a 4096-aligned base + o_k bytes (o0: the image, o1 .. o11: the info's in order)
//   a mask pixels        ->  per pointer of the info the bytes it moved, -1 where it was NULL and stayed NULL, -2 where NULL did not stay NULL
//   n sizeY poolThreads  ->  chainCount chainRows
//   l sizeX sizeY force_split_kernels legacy_float_stage  ->  list_in_one_pair
#include "../../limg_amd/csrc/limg_hip_encode_plan.h"

#include <stdio.h>
#include <string.h>

using namespace limg_hip;

namespace
{
  bool read_facts(EncodeFacts &f)
  {
    long long v[29];
    for (long long &k : v)
      if (scanf("%lld", &k) != 1) return false;
    int i = 0;
    memset(&f, 0, sizeof(f));
    f.nullArgument = v[i++] != 0; f.sizeX = (size_t)v[i++]; f.sizeY = (size_t)v[i++]; f.planes = (PlaneSet)v[i++];
    f.callerRecords = v[i++] != 0; f.callerShifts = v[i++] != 0; f.recordsAligned = v[i++] != 0; f.poolThreads = (int)v[i++]; f.fast = v[i++] != 0;
    f.chainPhase = (int)v[i++]; f.batchCount = (size_t)v[i++];
    f.inner = v[i++] != 0; f.innerLast = v[i++] != 0; f.fitOnly = v[i++] != 0; f.fitFloatMode = v[i++] != 0; f.streamRaw = v[i++] != 0; f.stripWords = v[i++] != 0;
    f.errorFactors = v[i++] != 0; f.ratedTable = v[i++] != 0; f.dPrevDesc = v[i++] != 0;
    f.force_split_kernels = (int32_t)v[i++]; f.legacy_float_stage = (int32_t)v[i++]; f.dither_pcg = (int32_t)v[i++]; f.float_mode = (int32_t)v[i++];
    f.collect_stats = (int32_t)v[i++]; f.batch_sub_images = (int32_t)v[i++]; f.ragged_bands = (int32_t)v[i++]; f.whole_image_ragged = (int32_t)v[i++];
    f.checkpoint_reach = (size_t)v[i++];
    f.part = partition(f.sizeY, f.poolThreads);
    return f.planes >= kPlanesNone && f.planes <= kPlanesInvalid;
  }

  // ---- the parent's conditions.  The names are the parent's (c->opt, x, e, p = e.p, dInfo, compact as what was tested of them), so that the lines below are its lines;
  // what it did between them (allocation, launches) is left out, and its early returns are in its order. ----
  struct ParentAnswer { limg_hip_result code; int path; size_t subImages; uint32_t bands, bandRows; int prefit, fused, floatFast, wantStats, fullPlanes, storePlanes, streamRaw, fitOnly, marks; };
  ParentAnswer parent_plan(const EncodeFacts &f)
  {
    const int kBlock = 8, kStripBlocks = 32;
    struct { limg_hip_options opt; } ctx, *c = &ctx;
    memset(&ctx, 0, sizeof(ctx));
    c->opt.force_split_kernels = f.force_split_kernels; c->opt.legacy_float_stage = f.legacy_float_stage; c->opt.dither_pcg = f.dither_pcg; c->opt.float_mode = f.float_mode;
    c->opt.collect_stats = f.collect_stats; c->opt.batch_sub_images = f.batch_sub_images; c->opt.ragged_bands = f.ragged_bands;
    const int topt_whole_image_ragged = f.whole_image_ragged;
    struct { int chainPhase; size_t batchCount; bool inner, fitOnly, fitFloatMode, streamRaw, stripWords, errorFactors, ratedTable, dPrevDesc; int marks; } x =
      { f.chainPhase, f.batchCount, f.inner, f.fitOnly, f.fitFloatMode, f.streamRaw, f.stripWords, f.errorFactors, f.ratedTable, f.dPrevDesc, f.inner ? (f.innerLast ? 0 : 1) : 2 };
    const size_t sizeX = f.sizeX, sizeY = f.sizeY;
    const int poolThreads = f.poolThreads, fast = f.fast;
    const bool dInfo = f.planes != kPlanesNone;
    struct { bool pRecords, pShifts; } compactOut = { f.callerRecords, f.callerShifts }, *compact = (f.callerRecords || f.callerShifts) ? &compactOut : nullptr;
    ParentAnswer a;
    memset(&a, 0, sizeof(a));
    a.path = -1;
    auto refuse = [&](limg_hip_result r) { memset(&a, 0, sizeof(a)); a.code = r; a.path = -1; return a; };

    // encode_device
    const int chainPhase = x.chainPhase;
    const size_t batchCount = x.batchCount;
    if (f.nullArgument) return refuse(limg_hip_error_ArgumentNull); // if (!c || !dIn)
    if (sizeX == 0 || sizeY == 0 || sizeX > 0x7FFFFFF8ull || sizeY > 0x7FFFFFF8ull) return refuse(limg_hip_error_InvalidParameter);
    bool fullPlanes = true;
    if (dInfo)
    {
      if (f.planes == kPlanesInvalid) return refuse(limg_hip_error_ArgumentNull); // the n32 count: see the `s` question
      fullPlanes = f.planes == kPlanesFull;
    }
    const bool ragged = (sizeX % kBlock) != 0 || (sizeY % kBlock) != 0;
    if (ragged && sizeX % kBlock == 0 && sizeY > (size_t)kBlock && dInfo && chainPhase == 0 && batchCount == 1 && !x.inner && !x.fitOnly && c->opt.force_split_kernels == 0 &&
        c->opt.legacy_float_stage == 0 && c->opt.dither_pcg == 0 && topt_whole_image_ragged == 0)
    {
      if (((sizeX / kBlock) * ((sizeY + kBlock - 1) / kBlock)) * 3 <= f.checkpoint_reach)
      { // encode_height_ragged: its two parts record 3 and 0 events, it records one; statistics if (c->opt.collect_stats != 0)
        a.path = kPathHeightRagged; a.marks = 1; a.wantStats = c->opt.collect_stats != 0;
        return a;
      }
    }
    // encode_params
    struct { uint32_t blocksX, blocksY, stripsX; int floatFast, prefit; bool storePlanes, fullPlanes, streamRaw, fitOnly; } p;
    p.blocksX = (uint32_t)((sizeX + kBlock - 1) / kBlock);
    p.blocksY = (uint32_t)((sizeY + kBlock - 1) / kBlock);
    p.stripsX = (p.blocksX + kStripBlocks - 1) / kStripBlocks;
    p.floatFast = (c->opt.float_mode == 1 && (!x.fitOnly || x.fitFloatMode)) ? 1 : 0;
    const Partition pt = partition(sizeY, poolThreads);
    const bool recordsAligned = (compact && compact->pRecords) ? f.recordsAligned : true; // p.records: the caller's, or the context's own buffer
    p.storePlanes = dInfo;
    p.fullPlanes = fullPlanes;
    p.streamRaw = x.streamRaw && !fullPlanes;
    p.fitOnly = x.fitOnly && !dInfo;
    const bool rated = batchCount > 1 && x.errorFactors && x.ratedTable; // e.rated
    if (chainPhase != 0 && (ragged || !dInfo || poolThreads != 0)) return refuse(limg_hip_error_InvalidParameter);
    p.prefit = (!ragged && c->opt.legacy_float_stage == 0 && recordsAligned) ? 1 : 0;
    const bool fused = dInfo && !ragged && (c->opt.force_split_kernels == 0 || batchCount > 1) && chainPhase == 0;
    const bool wantStats = c->opt.collect_stats != 0 && dInfo && chainPhase == 0;
    // encode_device again
    const bool compactList = !fullPlanes && x.streamRaw && x.stripWords && compact && compact->pRecords && compact->pShifts;
    const bool fitList = p.fitOnly && p.prefit && !ragged && chainPhase == 0;
    if (batchCount > 1 && !fitList && (!fused || !p.prefit || (!fullPlanes && !compactList))) return refuse(limg_hip_error_InvalidParameter);
    if (x.errorFactors && (!rated || batchCount <= 1 || !compactList || !fused || !p.prefit || !fast || chainPhase != 0)) return refuse(limg_hip_error_InvalidParameter);
    a.prefit = p.prefit; a.fused = fused; a.floatFast = p.floatFast; a.wantStats = wantStats; a.fullPlanes = p.fullPlanes; a.storePlanes = p.storePlanes; a.streamRaw = p.streamRaw;
    a.fitOnly = p.fitOnly;
    a.marks = chainPhase != 0 ? 2 : (x.marks == 2 ? 4 : (x.marks == 1 ? 3 : 0)); // a chain phase: plain mark() twice; else mark_if: levels 1 (three events) and 2 (the fourth)
    // sub_batch_images
    size_t subImages = 0;
    {
      const limg_hip_options &o = c->opt;
      if (!fused || x.batchCount <= 1 || !p.prefit) subImages = 0;
      else if (o.batch_sub_images > 0) subImages = (size_t)o.batch_sub_images;
      else if (o.batch_sub_images == 0) subImages = x.batchCount >= 32 ? 8 : (x.batchCount >= 16 ? 4 : 0);
      else subImages = 0;
    }
    if (subImages > 0 && subImages < batchCount) { a.path = kPathSubBatches; a.subImages = subImages; return a; }
    if (fused) { a.path = kPathFused; return a; }
    if (chainPhase == 2) { a.path = kPathChainPhase2; return a; }
    if (!ragged) { a.path = kPathSplit; return a; }
    a.path = kPathRagged;
    // band_count, encode_ragged
    {
      const limg_hip_options &o = c->opt;
      uint32_t nBands = 1;
      if (dInfo && !x.dPrevDesc && pt.chainCount <= 1 && o.ragged_bands >= 0 && p.blocksX >= 2 && p.blocksY >= 2 && (o.ragged_bands > 0 || (p.blocksX >= 32 && p.blocksY >= 64)))
        nBands = o.ragged_bands > 0 ? (uint32_t)o.ragged_bands : 16u;
      if (nBands > p.blocksY / 2) nBands = p.blocksY / 2 ? p.blocksY / 2 : 1;
      if (nBands > 64) nBands = 64;
      const uint32_t bandRows = (p.blocksY + nBands - 1) / nBands;
      nBands = (p.blocksY + bandRows - 1) / bandRows;
      a.bands = nBands; a.bandRows = bandRows;
    }
    return a;
  }
}

int main()
{
  char what;
  while (scanf(" %c", &what) == 1)
  {
    if (what == 'p' || what == 'P')
    {
      EncodeFacts f;
      if (!read_facts(f)) return 2;
      if (what == 'p')
      {
        const EncodePlan p = encode_plan(f);
        printf("%d %d %d %llu %u %u %d %d %d %d %d %d %d %d %d\n", (int)p.code, (int)p.verdict, p.code == limg_hip_success ? (int)p.path : -1, (unsigned long long)p.subImages, p.bands,
               p.bandRows, (int)p.prefit, (int)p.fused, (int)p.floatFast, (int)p.wantStats, (int)p.fullPlanes, (int)p.storePlanes, (int)p.streamRaw, (int)p.fitOnly, p.marks);
      }
      else
      {
        const ParentAnswer a = parent_plan(f);
        printf("%d %d %llu %u %u %d %d %d %d %d %d %d %d %d\n", (int)a.code, a.path, (unsigned long long)a.subImages, a.bands, a.bandRows, a.prefit, a.fused, a.floatFast, a.wantStats,
               a.fullPlanes, a.storePlanes, a.streamRaw, a.fitOnly, a.marks);
      }
    }
    else if (what == 'e')
    {
      unsigned long long x, y;
      if (scanf("%llu %llu", &x, &y) != 2) return 2;
      const EncodeShape sh((size_t)x, (size_t)y);
      printf("%llu %llu %llu %llu %llu %d %d\n", (unsigned long long)sh.blocksX, (unsigned long long)sh.blocksY, (unsigned long long)sh.stripsX, (unsigned long long)sh.blocks,
             (unsigned long long)sh.strips, (int)sh.valid, (int)sh.whole);
    }
    else if (what == 's' || what == 'a')
    {
      static uint32_t words[8][64];
      static uint8_t bytes[3][64];
      unsigned mask;
      unsigned long long pixels = 0;
      if (scanf("%u", &mask) != 1 || mask >= (1u << 11) || (what == 'a' && (scanf("%llu", &pixels) != 1 || pixels > 64))) return 2;
      limg_hip_encode3d_info info;
      memset(&info, 0, sizeof(info));
      uint32_t **w[] = { &info.pDecoded, &info.pShiftABCX, &info.pColAMin, &info.pColAMax, &info.pColBMin, &info.pColBMax, &info.pColCMin, &info.pColCMax };
      uint8_t **b[] = { &info.pFactorsA, &info.pFactorsB, &info.pFactorsC };
      for (int i = 0; i < 8; i++) if (mask & (1u << i)) *w[i] = words[i];
      for (int i = 0; i < 3; i++) if (mask & (1u << (8 + i))) *b[i] = bytes[i];
      if (what == 's') { printf("%d\n", (int)plane_set(&info)); continue; }
      advance_planes(info, (size_t)pixels);
      for (int i = 0; i < 11; i++)
      {
        const uint8_t *now = i < 8 ? (const uint8_t *)*w[i] : *b[i - 8], *was = i < 8 ? (const uint8_t *)words[i] : bytes[i - 8];
        const long long moved = !(mask & (1u << i)) ? (now ? -2 : -1) : (long long)(now - was);
        printf(i < 10 ? "%lld " : "%lld\n", moved);
      }
    }
    else if (what == 'v')
    {
      alignas(4096) static uint8_t base[12][4096];
      unsigned long long sizeX, o[12];
      int full, hasInfo;
      if (scanf("%llu %d %d", &sizeX, &full, &hasInfo) != 3) return 2;
      for (unsigned long long &k : o)
        if (scanf("%llu", &k) != 1 || k >= 2048 || k % 4 != 0) return 2;
      limg_hip_encode3d_info info;
      void **pp = reinterpret_cast<void **>(&info);
      for (int i = 0; i < 11; i++) pp[i] = base[1 + i] + o[1 + i];
      const VecAccess v = vec_access((const uint32_t *)(base[0] + o[0]), hasInfo ? &info : nullptr, (size_t)sizeX, full != 0);
      printf("%d %d %d %d %d\n", (int)v.in, (int)v.planes, (int)v.factors8, (int)v.decoded, (int)v.factors);
    }
    else if (what == 'n')
    {
      unsigned long long y;
      int pool;
      if (scanf("%llu %d", &y, &pool) != 2) return 2;
      const Partition pt = partition((size_t)y, pool);
      printf("%u %u\n", pt.chainCount, pt.chainRows);
    }
    else if (what == 'l')
    {
      unsigned long long x, y;
      int fs, lf;
      if (scanf("%llu %llu %d %d", &x, &y, &fs, &lf) != 4) return 2;
      limg_hip_options o;
      memset(&o, 0, sizeof(o));
      o.force_split_kernels = fs; o.legacy_float_stage = lf;
      printf("%d\n", (int)list_in_one_pair(EncodeShape((size_t)x, (size_t)y), o));
    }
    else return 2;
  }
  return 0;
}
