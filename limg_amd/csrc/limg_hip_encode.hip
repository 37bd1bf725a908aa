// limg_hip_encode.hip -- the 8x8 encode: its parameters, the launch paths of an image of whole blocks (fused, sub-batch pipeline, chain phases, split) and the
// dispatcher that runs the one the plan names (encode_device; the decisions: limg_hip_encode_plan.h); the *_device, batch, chain and stats entries of the C ABI.
// Images with partial edge blocks: limg_hip_encode_ragged.hip.  Mirrors the reference's driver (src/limg.cpp:2175-2265 threshold/flag setup).
#include "limg_hip_context.h"
#include "limg_search_table_accurate.h"

using namespace limg_hip;

namespace
{
  // the reference's "Average Block Bits" counters (src/limg.cpp:1971-1999) of this encode, left on the device for limg_hip_last_stats
  // `rows` block rows of shift words of images of shape sh, `pixels` in all; add: on top of what the counters hold
  limg_hip_result shift_stats(limg_hip_context *c, const uint32_t *shifts, const EncodeShape &sh, size_t rows, uint64_t pixels, bool add, hipStream_t stream)
  {
    limg_hip_result rs;
    if ((rs = c->stats.counters.ensure(30 * 8)) != limg_hip_success) return rs;
    if (!add) HIP_TRY(hipMemsetAsync(c->stats.counters.p, 0, 30 * 8, stream));
    launch_shift_stats(shifts, (uint32_t)sh.blocksX, (uint32_t)sh.blocksY, (uint32_t)rows, (uint32_t)sh.sizeX, (uint32_t)sh.sizeY, (unsigned long long *)c->stats.counters.p, stream);
    c->stats.stream = stream; c->stats.state = 1;
    c->stats.pixels = (add ? c->stats.pixels : 0) + pixels;
    return limg_hip_success;
  }
  limg_hip_result encode_stats(const EncodeJob &e, const limg_hip_compact_out *compact)
  {
    limg_hip_context *const c = e.c;
    if (!e.plan.wantStats || e.x.inner) return limg_hip_success;
    const EncodeShape sh(e.sizeX, e.sizeY);
    const bool add = c->stats.accumulate && e.plan.path != kPathHeightRagged; // (an image of that path restarts the counters of a list)
    const uint32_t *shifts = (compact && compact->pShifts) ? compact->pShifts : (const uint32_t *)c->enc.shifts.p;
    return shift_stats(c, shifts, sh, sh.blocksY * e.x.batchCount, (uint64_t)e.sizeX * e.sizeY * e.x.batchCount, add, e.stream);
  }

  // The accurate search's automaton (tools/make_search_table.py, src/limg_bit_crush.h:668-830) in the form the kernel's scalar loads want: 8 dwords per state,
  // every field in a dword of its own = { a | phase2 << 5 | final << 31, byte offset on pass, byte offset on fail, b, c, mul(a), mul(b), mul(c) }.  Bits 24..26 of the two
  // offsets say which factors' shifts the SUCCESSOR's triple changes against this state's (A, B, C): a state of this DAG has several predecessors, so the change mask is a
  // property of the edge -- with it the kernel needs no record of the shifts its cached terms were built for and no three compares per trial.
  // The one expansion: what the context uploads and what limg_hip_host_accurate_table hands out (tests/test_search_tables.py checks every entry and edge of it).
  constexpr size_t kAccTableDwords = (size_t)LIMG_SEARCH_ACC_STATES * 8;
  void expand_accurate_table(uint32_t *wide /* kAccTableDwords */)
  {
    static const uint32_t compact[LIMG_SEARCH_ACC_STATES][2] = LIMG_SEARCH_ACC_TABLE_INIT;
    static const uint32_t mul[9] = { 1, 2, 4, 8, 17, 36, 85, 255, 256 }; // (1 << s) + decode_bias(s), src/limg_bit_crush_simd.h:611-619
    memset(wide, 0, kAccTableDwords * 4);
    for (size_t i = 0; i < (size_t)LIMG_SEARCH_ACC_STATES; i++)
    {
      const uint32_t w0 = compact[i][0], w1 = compact[i][1];
      uint32_t *e = &wide[i * 8];
      if (w0 >> 31) { e[0] = 1u << 31; continue; }
      const uint32_t a = w0 & 15u, b = (w0 >> 4) & 15u, cc = (w0 >> 8) & 15u;
      e[0] = a | ((w0 & 0x1000u) ? 0x20u : 0u);
      e[1] = (w1 & 0xFFFFu) * 32u; e[2] = (w1 >> 16) * 32u;
      e[3] = b; e[4] = cc;
      e[5] = mul[a]; e[6] = mul[b]; e[7] = mul[cc];
    }
    static_assert((size_t)LIMG_SEARCH_ACC_STATES * 32u < (1u << 24), "offsets leave bits 24..26 free");
    for (size_t i = 0; i < (size_t)LIMG_SEARCH_ACC_STATES; i++)
    {
      uint32_t *e = &wide[i * 8];
      if (e[0] >> 31) continue;
      for (int k = 1; k <= 2; k++)
      {
        const uint32_t *n = &wide[(e[k] / 32u) * 8];
        uint32_t mask = 0;
        if (!(n[0] >> 31)) mask = ((n[0] & 31u) != (e[0] & 31u) ? 1u : 0u) | (n[3] != e[3] ? 2u : 0u) | (n[4] != e[4] ? 4u : 0u);
        e[k] |= mask << 24;
      }
    }
  }

  limg_hip_result ensure_accurate_table(limg_hip_context *c)
  {
    if (c->enc.accTable.p) return limg_hip_success;
    std::vector<uint32_t> wide(kAccTableDwords);
    expand_accurate_table(wide.data());
    limg_hip_result r = c->enc.accTable.ensure(wide.size() * 4);
    if (r != limg_hip_success) return r;
    if (hipMemcpy(c->enc.accTable.p, wide.data(), wide.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { c->enc.accTable.release(); return limg_hip_error_Generic; }
    return limg_hip_success;
  }

  // The whole 8x8 encode's EncodeParams: geometry, thresholds and flags as the plan has them, the per-block / per-strip scratch, the vector-access flags, the batch
  // table, the noise table and the chain-phase arguments.  It fills and allocates; it decides nothing.
  limg_hip_result encode_params(EncodeJob &e, const uint32_t *dIn, const limg_hip_compact_out *compact, uint32_t errorFactor, int fast)
  {
    limg_hip_context *const c = e.c;
    const EncodeExtra &x = e.x;
    const EncodePlan &plan = e.plan;
    const limg_hip_encode3d_info *const dInfo = e.dInfo;
    const size_t sizeX = e.sizeX, batchCount = x.batchCount;
    const ImageIO *const batch = x.batch;
    const EncodeShape sh(sizeX, e.sizeY);
    EncodeParams &p = e.p;
    memset(&p, 0, sizeof(p));
    p.io.in = dIn;
    p.sizeX = (uint32_t)sizeX; p.sizeY = (uint32_t)e.sizeY;
    p.blocksX = (uint32_t)sh.blocksX; p.blocksY = (uint32_t)sh.blocksY; p.stripsX = (uint32_t)sh.stripsX;
    // thresholds and flags (limg_hip_encode_rules.h)
    const Thresholds t = thresholds(errorFactor);
    p.maxPixel32 = t.maxPixel32; p.maxBlock = t.maxBlock; p.blockLimitFull = t.blockLimitFull; p.crushBits = (int32_t)t.crushBits;
    p.fast = fast != 0;
    p.accTable = nullptr;
    if (!p.fast && p.crushBits)
    {
      limg_hip_result ra = ensure_accurate_table(c);
      if (ra != limg_hip_success) return ra;
      p.accTable = (const uint32_t *)c->enc.accTable.p;
    }
    forced_shifts(c->opt.forced_shift, p.forced);
    p.floatFast = plan.floatFast ? 1 : 0;
    p.recordLimit = record_limit(c);
    const Partition pt = e.pt;
    p.chainCount = pt.chainCount; p.chainRows = pt.chainRows;

    p.batchCount = (uint32_t)batchCount;
    p.imageStrips = (uint32_t)sh.strips;
    e.blocks = sh.blocks * batchCount; e.strips = sh.strips * batchCount;
    // the per-block / per-strip scratch: sized for the larger encode this call may be a part of, addressed from this part's first block row
    const size_t scratchRows = x.scratchRows > (size_t)p.blocksY * batchCount ? x.scratchRows : (size_t)p.blocksY * batchCount;
    const size_t scratchBlocks = scratchRows * p.blocksX, scratchStrips = scratchRows * p.stripsX;
    const size_t blockOff = x.scratchRow0 * p.blocksX, stripOff = x.scratchRow0 * p.stripsX;
    limg_hip_result r;
    if (compact && compact->pRecords) p.records = compact->pRecords + blockOff;
    else { if ((r = c->enc.records.ensure(scratchBlocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r; p.records = (limg_hip_block_record *)c->enc.records.p + blockOff; }
    if (compact && compact->pShifts) p.shifts = compact->pShifts + blockOff;
    else { if ((r = c->enc.shifts.ensure(scratchBlocks * 4)) != limg_hip_success) return r; p.shifts = (uint32_t *)c->enc.shifts.p + blockOff; }
    if ((r = c->enc.invN.ensure(scratchBlocks * 16)) != limg_hip_success) return r;
    p.invN = (float *)c->enc.invN.p + blockOff * 4;
    if ((r = c->enc.stripCalls.ensure(scratchStrips * 4)) != limg_hip_success) return r;
    if ((r = c->enc.stripBase.ensure(scratchStrips * 4)) != limg_hip_success) return r;
    p.stripCalls = (uint32_t *)c->enc.stripCalls.p + stripOff; p.stripBase = (uint32_t *)c->enc.stripBase.p + stripOff;
    p.storePlanes = plan.storePlanes;
    p.fullPlanes = plan.fullPlanes;
    p.streamRaw = plan.streamRaw;
    p.stripWords = plan.streamRaw ? x.stripWords : nullptr;
    p.fitOnly = plan.fitOnly;
    p.prefit = plan.prefit ? 1 : 0;
    if (dInfo) p.io.info = *dInfo;
    VecAccess vec = vec_access(dIn, dInfo, sizeX, plan.fullPlanes);
    if (batchCount > 1)
    { // the 16-byte access paths only if every image of the batch allows them; the table goes to the device behind whatever the stream still holds
      for (size_t i = 1; i < batchCount; i++) vec &= vec_access(batch[i].in, dInfo ? &batch[i].info : nullptr, sizeX, plan.fullPlanes);
      if ((r = c->enc.batchTable.ensure(batchCount * sizeof(ImageIO))) != limg_hip_success) return r;
      launch_set_batch_table((ImageIO *)c->enc.batchTable.p, batch, batchCount, e.stream); // through kernel arguments: stream-ordered, and the host array may die right away
      p.batch = (const ImageIO *)c->enc.batchTable.p;
      if (x.errorFactors && x.ratedTable)
      { // one error factor per image: the thresholds go to the caller's table, by the same kind of launch as the image table
        launch_set_rated_table(x.ratedTable, x.errorFactors, batchCount, e.stream);
        e.rated = x.ratedTable;
      }
    }
    p.vecIn = vec.in; p.vecPlanes = vec.planes; p.vecFactors8 = vec.factors8; p.vecDecoded = vec.decoded; p.vecFactors = vec.factors;

    if (dInfo && sh.whole)
    {
      // longest chain, in blocks: every block makes at most 3 dither calls
      uint32_t maxRows = p.blocksY;
      if (pt.chainCount > 1 && (pt.chainCount - 1) * pt.chainRows < p.blocksY) maxRows = p.blocksY - (pt.chainCount - 1) * pt.chainRows; // the last chain takes the remainder, never fewer rows than the others
      if ((r = grow_noise_table(c, ((size_t)maxRows * p.blocksX + x.chainBlocksBefore) * 3, e.stream)) != limg_hip_success) return r;
      p.noise = (const uint8_t *)c->noise.table.p;
      p.noiseLast = (uint32_t)(c->noise.count - 1);
    }
    p.chainCallsOut = x.chainPhase == 1 ? x.dChainCalls : nullptr;
    p.chainBase = x.chainPhase == 2 ? x.dChainBase : nullptr;
    return limg_hip_success;
  }

  // the persistent kernel's ticket (16 B) and one 8-byte look-back descriptor per work strip, zero at its start: k_fit_tpb clears them on its way (one launch
  // and its gaps less per image); without that kernel, a memset
  limg_hip_result fused_scratch(EncodeJob &e, const limg_hip_compact_out *compact)
  {
    limg_hip_context *const c = e.c;
    EncodeParams &p = e.p;
    limg_hip_result r;
    PersistentScratch ps;
    if ((r = persistent_scratch(c, e.strips, e.x.batchCount + 1, e.stream, ps)) != limg_hip_success) return r; // (room for one ticket per sub-batch)
    p.ticket = ps.ticket; p.desc = ps.desc; p.timeout = ps.timeout; p.park = ps.park;
    p.zeroLookback = p.prefit ? 1 : 0;
    if (!p.prefit) HIP_TRY(hipMemsetAsync(p.ticket, 0, 16 + e.strips * 8, e.stream));
#ifdef LIMG_HIP_TEST_HOOKS
    p.lookbackSpins = c->topt.lookback_spins > 0 ? (uint32_t)c->topt.lookback_spins : (1u << 22);
    p.testSkipStrip = c->topt.skip_publish_strip > 0 ? (uint32_t)c->topt.skip_publish_strip - 1u : ~0u;
    p.testBaseErrStrip = c->topt.base_error_strip > 0 ? (uint32_t)c->topt.base_error_strip - 1u : ~0u;
#endif
    p.compactOut = compact != nullptr || e.plan.wantStats; // the statistics are reduced from the raster-order shift words
    return limg_hip_success;
  }

  // workgroups per CU of the persistent kernel: 6 once the float stage is out (7 fit and were measured: no faster, the kernel is issue-bound), 5 with it inside;
  // limg_hip_options.test_wg_per_cu lowers it (A/B runs), never above the launch bound the park slots are sized for
  int wg_per_cu(const limg_hip_context *c, int deflt)
  {
    const int t = TOPT(c, wg_per_cu);
    return (t >= 1 && t < deflt) ? t : deflt;
  }

  // k_encode_list_rated's arguments -- and a view of k_encode_list_mixed's table -- for `batchCount` images of shape sh from the table entries batch / rated on: geometry and partition,
  // the arrays from those images' first block and strip, the 16-byte access flags, the look-back; forced shifts, record limit and the noise table (grown before this) as the context has them.
  RatedListParams rated_list_params(const limg_hip_context *c, const EncodeShape &sh, const Partition &pt, const ImageIO *batch, const RatedImage *rated, uint32_t batchCount,
                                    limg_hip_block_record *records, float *invN, uint32_t *shifts, uint32_t *stripWords, const VecAccess &vec, const PersistentScratch &ps)
  {
    RatedListParams r;
    memset(&r, 0, sizeof(r));
    r.batch = batch; r.rated = rated;
    r.batchCount = batchCount; r.imageStrips = (uint32_t)sh.strips;
    r.sizeX = (uint32_t)sh.sizeX; r.sizeY = (uint32_t)sh.sizeY; r.blocksX = (uint32_t)sh.blocksX; r.blocksY = (uint32_t)sh.blocksY; r.stripsX = (uint32_t)sh.stripsX;
    forced_shifts(c->opt.forced_shift, r.forced);
    r.recordLimit = record_limit(c);
    r.chainCount = pt.chainCount; r.chainRows = pt.chainRows;
    r.records = records; r.invN = invN; r.shifts = shifts; r.stripWords = stripWords;
    r.noise = (const uint8_t *)c->noise.table.p; r.noiseLast = (uint32_t)(c->noise.count - 1);
    r.vecIn = vec.in; r.vecFactors = vec.factors; r.vecFactors8 = vec.factors8;
    r.desc = ps.desc; r.ticket = ps.ticket; r.timeout = ps.timeout; r.park = ps.park;
    return r;
  }

  // The persistent launch of a job, or of the sub-batch q of it that starts at image i0 of the list: k_encode_persistent, or -- a list with one error factor per
  // image -- k_encode_list_rated on the same scratch, with the threshold table offset as the image table is.
  void launch_persistent(const EncodeJob &e, const EncodeParams &q, size_t i0, int workgroups)
  {
    if (!e.rated) { launch_encode_persistent(q, e.channels, workgroups, e.stream); return; }
    const PersistentScratch ps = { q.ticket, q.desc, q.timeout, q.park };
    const VecAccess vec = { q.vecIn != 0, false, q.vecFactors8 != 0, false, q.vecFactors != 0 };
    const RatedListParams r = rated_list_params(e.c, EncodeShape(q.sizeX, q.sizeY), { q.chainCount, q.chainRows }, q.batch, e.rated + i0, q.batchCount, q.records, q.invN, q.shifts, q.stripWords, vec, ps);
    launch_encode_list_rated(r, e.channels, q.floatFast != 0, workgroups, e.stream);
  }

  // A list of images as a PIPELINE of launch pairs (limg_hip_options.batch_sub_images): k_fit_tpb of sub-batch k + 1 runs on a stream of the context's own next to
  // the persistent kernel of sub-batch k.  On content with short searches (BASELINE configs 2 / 4: ~2 trials per block) the persistent kernel waits for its plane
  // stores a third of the time while k_fit_tpb is pure vector work: side by side they fill each other's gaps.  The persistent kernel leaves the float stage room
  // to be resident: 5 workgroups per CU instead of 6 (at 6 x 80 VGPRs nothing else fits on a SIMD) for every sub-batch but the last.
  // Measured on 4096^2 random-gradient lists (profiles/archive/r04_pipeline_sweep.md): 64 images 66.5 -> 73.3 Gpixel/s in sub-batches of 8 (4: 70.9, 16: 71.9); 16 images
  // +3.5 % in sub-batches of 4; 8 images and fewer: nothing to gain (the lone first float stage and the 5-workgroup launches cost what the overlap saves).
  // Timeline: {k_fit_tpb of the first sub-batch -- the only float-stage work that runs alone --, the rest, -}.
  limg_hip_result encode_sub_batches(EncodeJob &e)
  {
    const size_t subImages = e.plan.subImages;
    limg_hip_context *const c = e.c;
    const EncodeParams &p = e.p;
    const size_t batchCount = e.x.batchCount;
    const hipStream_t stream = e.stream;
    // A/B hook (limg_hip_options.test_pipeline): bits 0..3 = 1 + k_fit_tpb's wave priority, bits 4..7 = workgroups per CU of the overlapped persistent launches,
    // bits 8..15 = images of the first sub-batch (whose float stage runs alone)
    const uint32_t knobs = (uint32_t)TOPT(c, pipeline);
    const int fitPrio = (knobs & 15u) ? (int)(knobs & 15u) - 1 : 0, wgOverlapRaw = ((knobs >> 4) & 15u) ? (int)((knobs >> 4) & 15u) : 5,
              wgOverlap = wgOverlapRaw > 6 ? 6 : wgOverlapRaw; // never above the launch bound the park slots are sized for
    const size_t firstSub = ((knobs >> 8) & 255u) && ((knobs >> 8) & 255u) < subImages ? (size_t)((knobs >> 8) & 255u) : subImages;
    const size_t nSub = 1 + (batchCount - firstSub + subImages - 1) / subImages;
    limg_hip_result r;
    hipStream_t fs;
    if ((r = c->enc.fitStream.get(fs)) != limg_hip_success) return r;
    if ((r = c->enc.pipeEvents.ensure(2 * nSub + 1, hipEventDisableTiming)) != limg_hip_success) return r;
    const size_t imgBlocks = (size_t)p.blocksX * p.blocksY, imgStrips = (size_t)p.imageStrips;
    auto sub = [&](size_t k) -> EncodeParams
    {
      EncodeParams q = p;
      const size_t i0 = k == 0 ? 0 : firstSub + (k - 1) * subImages, want = k == 0 ? firstSub : subImages, n = batchCount - i0 < want ? batchCount - i0 : want;
      q.batch = p.batch + i0; q.batchCount = (uint32_t)n;
      q.io = e.x.batch[i0]; // (what the kernels read when a sub-batch is a single image)
      q.records = p.records + i0 * imgBlocks; q.shifts = p.shifts + i0 * imgBlocks; q.invN = p.invN + i0 * imgBlocks * 4;
      if (p.stripWords) q.stripWords = p.stripWords + i0 * imgStrips; // (a sub-batch numbers its strips from 0: its payload words land at the list's offsets, where the packer reads one list)
      uint8_t *lb = (uint8_t *)c->enc.lookback.p + k * 16 + i0 * imgStrips * 8; // sub-batch k: its ticket, then the descriptors of its strips
      q.ticket = (uint32_t *)lb; q.desc = (unsigned long long *)(lb + 16);
      q.fitPrio = k == 0 ? 0 : fitPrio;
      return q;
    };
    hipEvent_t *ev = c->enc.pipeEvents.data(); // [0]: fork; [1 + 2 k]: k_fit_tpb of sub-batch k done; [2 + 2 k]: the persistent kernel of sub-batch k is next on `stream`
    e.tl.mark();
    HIP_TRY(hipEventRecord(ev[0], stream)); // everything the caller's stream holds so far (inputs, the image table, earlier encodes that use the scratch)
    HIP_TRY(hipStreamWaitEvent(fs, ev[0], 0));
    launch_fit_tpb(sub(0), e.channels, fs);
    HIP_TRY(hipEventRecord(ev[1], fs));
    for (size_t k = 0; k < nSub; k++)
    {
      HIP_TRY(hipStreamWaitEvent(stream, ev[1 + 2 * k], 0));
      if (k == 0) e.tl.mark();
      if (k + 1 < nSub)
      {
        HIP_TRY(hipEventRecord(ev[2 + 2 * k], stream));
        HIP_TRY(hipStreamWaitEvent(fs, ev[2 + 2 * k], 0));
        launch_fit_tpb(sub(k + 1), e.channels, fs);
        HIP_TRY(hipEventRecord(ev[3 + 2 * k], fs));
      }
      launch_persistent(e, sub(k), k == 0 ? 0 : firstSub + (k - 1) * subImages, c->enc.persistentWorkgroups / 5 * (k + 1 < nSub ? wgOverlap : wg_per_cu(c, 6)));
    }
    e.tl.mark();
    return limg_hip_success;
  }

  // k_fit_tpb (where the float stage is its own launch) + the persistent kernel: E step, look-back scan and F step of every strip in one launch.
  // Timeline: {k_fit_tpb, k_encode_persistent, -}; with the float stage inside the kernel {k_encode_persistent, -, -}.
  void encode_fused(EncodeJob &e)
  {
    const EncodeParams &p = e.p;
    if (p.prefit)
    {
      e.tl.mark();
      launch_fit_tpb(p, e.channels, e.stream);
    }
    e.tl.mark();
    launch_persistent(e, p, 0, e.c->enc.persistentWorkgroups / 5 * wg_per_cu(e.c, p.prefit ? 6 : 5));
    e.tl.mark();
  }

  // phase 2 of a chain encode: the E step and the scan of this very image ran in phase 1 -- records, shift words, strip bases and the pre-dither factor bytes are
  // where they left them.  A chain encode's timeline runs over its two phases, two events each: {E step + scan, exchange between the phases, F step}.
  void encode_chain_phase2(EncodeJob &e)
  {
    e.tl.mark();
    launch_dither_store(e.p, e.channels, e.stream);
  }

  // The split path on an image of whole blocks: [k_fit_tpb] + k_fit_search, the strip scan, k_dither_store.  Also pass 1 of the merged-block encoder (records only),
  // `_perf` (nothing to dither into, nothing to store) and phase 1 of a chain encode (E step + scan).  Timeline: {k_fit_tpb + k_fit_search, scan, k_dither_store}.
  void encode_split(EncodeJob &e)
  {
    const EncodeParams &p = e.p;
    e.tl.mark();
    if (p.prefit) launch_fit_tpb(p, e.channels, e.stream);
    if (p.prefit && p.fitOnly) return; // pass 1 of the merged-block encoder: the records are all it wants
    launch_fit_search(p, e.channels, e.stream);
    if (e.x.chainPhase != 1) e.tl.mark();
    if (!e.dInfo) return;
    launch_strip_scan(p, e.stream);
    if (e.x.chainPhase == 1) return;
    e.tl.mark();
    launch_dither_store(p, e.channels, e.stream);
  }

  // sizeX % 8 == 0, sizeY % 8 != 0, at least two block rows (reference: the rx x ry gather of src/limg.cpp:1899-1905 only ever sees ry < 8 in the last block row,
  // and a dither call over 8 ry pixels is ry AES rounds, :824-879): the block rows above the last one are an image of whole blocks -- k_fit_tpb + persistent kernel
  // with the chain partition of the WHOLE image -- and the last row goes through the split path's kernels as a one-row sub-image whose chain starts where the
  // persistent kernel's last strip left it: that call count is the low word of the strip's look-back descriptor, and the chain value there comes from the embedded
  // checkpoints (at most 1023 calls on foot).  The host's share is then one block row: blocksX shift words down, <= 3 blocksX calls of ry rounds, their noise up.
  // Timeline: the rows above record three events, the last row none, this call the fourth.
  limg_hip_result encode_height_ragged(const EncodeJob &e, const uint32_t *dIn, int hasAlpha, const limg_hip_compact_out *compact, uint32_t errorFactor, int poolThreads, int fast)
  {
    limg_hip_context *const c = e.c;
    const EncodeShape sh(e.sizeX, e.sizeY);
    const size_t sizeX = e.sizeX, topY = (sh.blocksY - 1) * kBlock;
    c->chain.in = nullptr;
    c->stats.state = 0;
    limg_hip_result r;
    EncodeExtra xt;
    xt.streamRaw = e.x.streamRaw; xt.inner = true; xt.part = &e.pt; xt.scratchRows = sh.blocksY;
    if ((r = encode_device(c, dIn, sizeX, topY, hasAlpha, e.dInfo, compact, errorFactor, poolThreads, fast, e.stream, xt)) != limg_hip_success) return r;
    // the last block row
    limg_hip_encode3d_info low = *e.dInfo;
    advance_planes(low, topY * sizeX); // pixels above the last block row, in every plane
    EncodeExtra xb;
    xb.streamRaw = e.x.streamRaw; xb.inner = xb.innerLast = true; xb.scratchRow0 = sh.blocksY - 1; xb.scratchRows = sh.blocksY;
    const Partition one = { 1, 0 };
    xb.part = &one;
    const bool sameChain = chain_of_row(e.pt.chainCount, e.pt.chainRows, (uint32_t)sh.blocksY - 1) == chain_of_row(e.pt.chainCount, e.pt.chainRows, (uint32_t)sh.blocksY - 2);
    if (sameChain) xb.dPrevDesc = (const unsigned long long *)((const uint8_t *)c->enc.lookback.p + 16) + ((sh.blocksY - 1) * sh.stripsX - 1);
    return encode_device(c, dIn + topY * sizeX, sizeX, e.sizeY - topY, hasAlpha, &low, compact, errorFactor, 0, fast, e.stream, xb);
  }
}

namespace limg_hip
{
  limg_hip_result ensure_device_status(limg_hip_context *c, hipStream_t stream)
  {
    if (c->enc.devStatus.p) return limg_hip_success;
    const limg_hip_result r = c->enc.devStatus.ensure(16);
    if (r == limg_hip_success) HIP_TRY(hipMemsetAsync(c->enc.devStatus.p, 0, 16, stream));
    return r;
  }

  limg_hip_result persistent_scratch(limg_hip_context *c, size_t strips, size_t tickets, hipStream_t stream, PersistentScratch &ps)
  {
    limg_hip_result r;
    if ((r = c->enc.lookback.ensure(16 * tickets + strips * 8)) != limg_hip_success) return r;
    if ((r = ensure_device_status(c, stream)) != limg_hip_success) return r;
    if ((r = c->enc.park.ensure((size_t)(c->enc.persistentWorkgroups / 5 * 6) * 2 * 8192)) != limg_hip_success) return r; // 6 workgroups per CU: the kernel's launch bound
    ps = { (uint32_t *)c->enc.lookback.p, (unsigned long long *)((uint8_t *)c->enc.lookback.p + 16), (uint32_t *)c->enc.devStatus.p, (uint8_t *)c->enc.park.p };
    return limg_hip_success;
  }

  limg_hip_result encode_list_chunk(limg_hip_context *c, const ListChunkImage *images, size_t n, int hasAlpha, int poolThreads, uint32_t *stripWords, uint8_t *hostTables,
                                    uint8_t *devTables, hipStream_t stream, ListChunkTotals &totals, bool fitOnly)
  {
    // what an outer call resets (encode_device): the context's per-block scratch is reused -- no chain encode's phase 1 is pending any more --, its statistics are stale
    c->chain.in = nullptr;
    if (!c->stats.accumulate) c->stats.state = 0;
    const ChunkTables T = chunk_tables(n);
    RatedListParams *const views = (RatedListParams *)(hostTables + T.views);
    ListImage *const list = (ListImage *)(hostTables + T.images);
    ImageIO *const io = (ImageIO *)(hostTables + T.io);
    RatedImage *const rated = (RatedImage *)(hostTables + T.rated);
    uint32_t *const firstStrip = (uint32_t *)(hostTables + T.firstStrip), *const firstUnit = (uint32_t *)(hostTables + T.firstUnit);
    const ImageIO *const dIo = (const ImageIO *)(devTables + T.io);
    const RatedImage *const dRated = (const RatedImage *)(devTables + T.rated);
    ListChunkTotals &tot = totals = {};
    for (size_t i = 0; i < n; i++)
    {
      const ListChunkImage &im = images[i];
      list[i] = list_image(tot, im.sizeX, im.sizeY, poolThreads, im.in, im.fac);
      firstStrip[i] = list[i].firstStrip; firstUnit[i] = list[i].firstUnit;
      io[i].in = im.in; io[i].info.pFactorsA = im.fac[0]; io[i].info.pFactorsB = im.fac[1]; io[i].info.pFactorsC = im.fac[2];
      const Thresholds t = thresholds(im.errorFactor);
      rated[i].maxPixel32 = t.maxPixel32; rated[i].blockLimitFull = t.blockLimitFull; rated[i].maxBlock = t.maxBlock; rated[i].crushBits = (int32_t)t.crushBits; rated[i].errorFactor = im.errorFactor;
    }
    limg_hip_result r;
    PersistentScratch ps = {};
    if (fitOnly)
    { // no noise table, and of the persistent launch's scratch only what the fit grid clears on its way: the ticket and the look-back descriptors
      if ((r = c->enc.lookback.ensure(16 * 2 + (size_t)tot.strips * 8)) != limg_hip_success) return r;
      ps.ticket = (uint32_t *)c->enc.lookback.p; ps.desc = (unsigned long long *)((uint8_t *)c->enc.lookback.p + 16);
    }
    else
    {
      if ((r = grow_noise_table(c, (size_t)tot.noiseCalls, stream)) != limg_hip_success) return r; // the largest per-chain need of any image: every image starts at the seed
      if ((r = persistent_scratch(c, tot.strips, 2, stream, ps)) != limg_hip_success) return r;
    }
    limg_hip_block_record *const records = (limg_hip_block_record *)c->enc.records.p;
    float *const invN = (float *)c->enc.invN.p;
    uint32_t *const shifts = (uint32_t *)c->enc.shifts.p;
    for (size_t i = 0; !fitOnly && i < n; i++)
    { // the view of image i: RatedListParams as its own launch would have them, the per-block arrays from its first block
      const ListImage &im = list[i];
      const VecAccess vec = { (im.vec & kListVecIn) != 0, false, (im.vec & kListVecFactors8) != 0, false, (im.vec & kListVecFactors) != 0 };
      views[i] = rated_list_params(c, EncodeShape(im.sizeX, im.sizeY), { im.chainCount, im.chainRows }, dIo + i, dRated + i, 1, records + im.firstBlock, invN + 4 * im.firstBlock, shifts + im.firstBlock,
                                   stripWords, vec, ps);
    }
    launch_set_words(devTables, hostTables, T.bytes, stream); // through kernel arguments: stream-ordered, the host copy may die right away
    const bool floatFast = c->opt.float_mode == 1;
    const int channels = hasAlpha ? 4 : 3;
    FitListParams f; MixedListParams m;
    memset(&f, 0, sizeof(f)); memset(&m, 0, sizeof(m));
    f.images = (const ListImage *)(devTables + T.images); f.batch = dIo; f.firstUnit = (const uint32_t *)(devTables + T.firstUnit);
    f.nImages = (uint32_t)n; f.nUnits = tot.units;
    f.records = records; f.invN = invN; f.desc = ps.desc; f.ticket = ps.ticket;
    m.views = (const RatedListParams *)(devTables + T.views); m.batch = dIo; m.rated = dRated; m.firstStrip = (const uint32_t *)(devTables + T.firstStrip);
    m.nImages = (uint32_t)n; m.nStrips = tot.strips; m.ticket = ps.ticket; m.park = ps.park;
    Timeline tl(c, stream, 4); // {k_fit_tpb_list, k_encode_list_mixed, -}; fitOnly: {k_fit_tpb_list, -, -}
    tl.mark();
    launch_fit_tpb_list(f, channels, floatFast, tot.vecInAll, stream);
    tl.mark();
    if (fitOnly)
    { // the records and invN are all the caller wants (the size probes of the chunk): in the context's float mode, as the full form leaves them
      tl.close();
      HIP_TRY(hipGetLastError());
      return limg_hip_success;
    }
    launch_encode_list_mixed(m, channels, floatFast, c->enc.persistentWorkgroups / 5 * wg_per_cu(c, 6), stream);
    tl.mark();
    tl.close();
    // limg_hip_last_stats: the counters of every image of the chunk, added up (and to what the call's earlier parts left)
    for (size_t i = 0; c->opt.collect_stats && i < n; i++)
      if ((r = shift_stats(c, shifts + list[i].firstBlock, EncodeShape(list[i].sizeX, list[i].sizeY), list[i].blocksY, (uint64_t)list[i].sizeX * list[i].sizeY, c->stats.accumulate || i > 0,
                           stream)) != limg_hip_success)
        return r;
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  // One 8x8 encode, whichever of its paths applies: the facts, the plan (limg_hip_encode_plan.h), its refusal if there is one -- before anything is grown or
  // enqueued --, the parameters, the plan's path.
  limg_hip_result encode_device(limg_hip_context *c, const uint32_t *dIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_encode3d_info *dInfo,
                                const limg_hip_compact_out *compact, uint32_t errorFactor, int poolThreads, int fast, hipStream_t stream, const EncodeExtra &x)
  {
    EncodeFacts f = {};
    f.nullArgument = !c || !dIn;
    f.sizeX = sizeX; f.sizeY = sizeY;
    f.planes = plane_set(dInfo);
    f.callerRecords = compact && compact->pRecords; f.callerShifts = compact && compact->pShifts;
    f.recordsAligned = compact && (((uintptr_t)compact->pRecords) & 15u) == 0;
    f.poolThreads = poolThreads; f.fast = fast != 0;
    f.part = x.part ? *x.part : partition(sizeY, poolThreads);
    f.chainPhase = x.chainPhase; f.batchCount = x.batchCount;
    f.inner = x.inner; f.innerLast = x.innerLast; f.fitOnly = x.fitOnly; f.fitFloatMode = x.fitFloatMode; f.streamRaw = x.streamRaw;
    f.stripWords = x.stripWords != nullptr; f.errorFactors = x.errorFactors != nullptr; f.ratedTable = x.ratedTable != nullptr; f.dPrevDesc = x.dPrevDesc != nullptr;
    if (c)
    {
      const limg_hip_options &o = c->opt;
      f.force_split_kernels = o.force_split_kernels; f.legacy_float_stage = o.legacy_float_stage; f.dither_pcg = o.dither_pcg; f.float_mode = o.float_mode;
      f.collect_stats = o.collect_stats; f.batch_sub_images = o.batch_sub_images; f.ragged_bands = o.ragged_bands;
      f.whole_image_ragged = TOPT(c, whole_image_ragged);
    }
    f.checkpoint_reach = checkpoint_reach();
    const EncodePlan plan = encode_plan(f);
    // what a call that is no part of a larger one resets, as far as it gets: the context's per-block scratch is about to be reused, its statistics are about to be stale
    const bool outer = x.chainPhase == 0 && !x.inner;
    if (outer && plan.verdict > kRefusedNull) c->chain.in = nullptr;
    if (outer && plan.verdict > kRefusedChain && !c->stats.accumulate) c->stats.state = 0;
    if (plan.code != limg_hip_success) return plan.code;
    HIP_TRY(hipSetDevice(c->device));

    EncodeJob e = { c, stream, x, dInfo, sizeX, sizeY, plan, Timeline(c, stream, plan.marks) };
    e.channels = hasAlpha ? 4 : 3;
    e.pt = f.part;
    limg_hip_result r = limg_hip_success;
    if (plan.path != kPathHeightRagged)
    {
      if ((r = encode_params(e, dIn, compact, errorFactor, fast)) != limg_hip_success) return r;
      if (plan.fused && (r = fused_scratch(e, compact)) != limg_hip_success) return r;
    }
    switch (plan.path)
    {
      case kPathHeightRagged: r = encode_height_ragged(e, dIn, hasAlpha, compact, errorFactor, poolThreads, fast); break;
      case kPathSubBatches: r = encode_sub_batches(e); break;
      case kPathFused: encode_fused(e); break;
      case kPathChainPhase2: encode_chain_phase2(e); break;
      case kPathSplit: encode_split(e); break;
      case kPathRagged: r = encode_ragged(e); break;
    }
    if (r != limg_hip_success) return r;
    e.tl.close();
    HIP_TRY(hipGetLastError());
    return encode_stats(e, compact);
  }
}

extern "C"
{
  limg_hip_result limg_hip_host_partition(size_t sizeY, int poolThreads, uint32_t *pChainCount, uint32_t *pChainBlockRows)
  {
    if (!pChainCount || !pChainBlockRows) return limg_hip_error_ArgumentNull;
    const Partition pt = partition(sizeY, poolThreads);
    *pChainCount = pt.chainCount;
    *pChainBlockRows = pt.chainRows;
    return limg_hip_success;
  }

  limg_hip_result limg_hip_host_accurate_table(uint32_t *pOut, size_t dwords)
  {
    if (!pOut) return limg_hip_error_ArgumentNull;
    if (dwords != kAccTableDwords) return limg_hip_error_InvalidParameter;
    expand_accurate_table(pOut);
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode3d_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_encode3d_info *pInfo,
                                           const limg_hip_compact_out *pCompact, uint32_t errorFactor, int poolThreads, int fastBitCrushing, void *stream)
  {
    return encode_device(c, pIn, sizeX, sizeY, hasAlpha, pInfo, pCompact, errorFactor, poolThreads, fastBitCrushing, (hipStream_t)stream);
  }

  // The reference encodes a list of images by calling limg_encode3d_test(_perf) once per image (src/main.cpp:278-323).  Here the images of one shape go through ONE
  // launch pair: one k_fit_tpb grid over the blocks of all images and one persistent launch whose tickets run through the strips of image 0, image 1, ...;
  // every image starts its own dither chain(s), so each image's planes are those of a single encode.  A small image alone cannot fill the chip for long
  // (a 4096^2 image is ~5 strips per workgroup: ramp-up and drain are a third of its encode); a batch amortises both.
  limg_hip_result limg_hip_encode3d_batch_device(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                 const limg_hip_encode3d_info *pInfos, uint32_t errorFactor, int poolThreads, int fastBitCrushing, void *stream)
  {
    if (!c || !ppIn || !pInfos) return limg_hip_error_ArgumentNull;
    if (count == 0) return limg_hip_success;
    const EncodeShape sh(sizeX, sizeY);
    if (!sh.valid) return limg_hip_error_InvalidParameter;
    bool full = true;
    for (size_t i = 0; i < count; i++)
    {
      if (!ppIn[i]) return limg_hip_error_ArgumentNull;
      const PlaneSet planes = plane_set(&pInfos[i]);
      if (planes == kPlanesInvalid) return limg_hip_error_ArgumentNull;
      full = full && planes == kPlanesFull;
    }
    const size_t chunk = list_chunk(c, sh.blocks, sh.strips); // longer lists go in several launch pairs
    const bool oneByOne = count == 1 || !full || !list_in_one_pair(sh, c->opt);
    std::vector<ImageIO> table;
    limg_hip_result r = limg_hip_success;
    for (size_t i0 = 0; i0 < count && r == limg_hip_success;)
    {
      const size_t n = oneByOne ? 1 : (count - i0 < chunk ? count - i0 : chunk);
      c->stats.accumulate = i0 != 0; // limg_hip_last_stats: all images of the list together, however many launch pairs it took
      if (n == 1) r = encode_device(c, ppIn[i0], sizeX, sizeY, hasAlpha, &pInfos[i0], nullptr, errorFactor, poolThreads, fastBitCrushing, (hipStream_t)stream);
      else
      {
        table.resize(n);
        for (size_t i = 0; i < n; i++) { table[i].in = ppIn[i0 + i]; table[i].info = pInfos[i0 + i]; }
        EncodeExtra x;
        x.batch = table.data(); x.batchCount = n;
        r = encode_device(c, ppIn[i0], sizeX, sizeY, hasAlpha, &pInfos[i0], nullptr, errorFactor, poolThreads, fastBitCrushing, (hipStream_t)stream, x);
      }
      i0 += n;
    }
    c->stats.accumulate = false;
    return r;
  }

  limg_hip_result limg_hip_encode3d_chain_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const limg_hip_encode3d_info *pInfo,
                                                 uint32_t errorFactor, int fastBitCrushing, int phase, uint64_t *pCallsDevice, const uint64_t *pChainBaseDevice,
                                                 size_t blocksBefore, void *stream)
  {
    if (phase != 1 && phase != 2) return limg_hip_error_InvalidParameter;
    if (!c || (phase == 1 && !pCallsDevice) || (phase == 2 && !pChainBaseDevice) || !pInfo) return limg_hip_error_ArgumentNull;
    // phase 2 continues the phase 1 the context holds: same strip, same planes (phase 1 left the pre-dither factor bytes in them), same parameters, and a noise
    // table that was sized for the same chain position
    if (phase == 2 && (c->chain.in != pIn || c->chain.x != sizeX || c->chain.y != sizeY || c->chain.fac[0] != pInfo->pFactorsA || c->chain.fac[1] != pInfo->pFactorsB ||
                       c->chain.fac[2] != pInfo->pFactorsC || c->chain.alpha != (hasAlpha != 0) || c->chain.ef != errorFactor || c->chain.fast != (fastBitCrushing != 0) ||
                       c->chain.before != blocksBefore))
      return limg_hip_error_InvalidParameter; // no matching phase 1 pending
    c->chain.in = nullptr;
    EncodeExtra x;
    x.chainPhase = phase; x.dChainCalls = (unsigned long long *)pCallsDevice; x.dChainBase = (const unsigned long long *)pChainBaseDevice; x.chainBlocksBefore = blocksBefore;
    const limg_hip_result r = encode_device(c, pIn, sizeX, sizeY, hasAlpha, pInfo, nullptr, errorFactor, 0, fastBitCrushing, (hipStream_t)stream, x);
    if (r == limg_hip_success && phase == 1)
    {
      c->chain.in = pIn; c->chain.x = sizeX; c->chain.y = sizeY; c->chain.before = blocksBefore;
      c->chain.fac[0] = pInfo->pFactorsA; c->chain.fac[1] = pInfo->pFactorsB; c->chain.fac[2] = pInfo->pFactorsC;
      c->chain.alpha = hasAlpha != 0; c->chain.ef = errorFactor; c->chain.fast = fastBitCrushing != 0;
    }
    return r;
  }

  // The reference's limg_encode3d_test accumulates its bit statistics on its own stack (`accum_bits`, src/limg.cpp:1975-1976) and prints them before it returns
  // (:2232-2248): they are always the statistics of THAT call, whatever other threads encode meanwhile.  Same here: the counters are fetched inside the region the
  // context's mutex covers, and collect_stats is switched on for this call only -- no option of a shared context is modified for good.
  limg_hip_result limg_hip_encode3d_stats(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, limg_hip_encode3d_info *pInfo, uint32_t errorFactor,
                                          int poolThreads, int fastBitCrushing, uint64_t *pCounters30, uint64_t *pPixels)
  {
    if (!c || !pCounters30) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    const int32_t was = c->opt.collect_stats;
    c->opt.collect_stats = 1;
    limg_hip_result r = limg_hip_encode3d(c, pIn, sizeX, sizeY, hasAlpha, pInfo, errorFactor, poolThreads, fastBitCrushing);
    if (r == limg_hip_success) r = limg_hip_last_stats(c, pCounters30, pPixels);
    c->opt.collect_stats = was;
    return r;
  }
}
