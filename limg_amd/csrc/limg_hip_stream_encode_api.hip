// limg_hip_stream_encode_api.hip -- the version 1 stream's encode family of the C ABI: limg_hip_encode_stream, limg_hip_encode_stream_batch, limg_hip_encode_stream_batch_ef, limg_hip_stream_sizes,
// limg_hip_encode_stream_budget, limg_hip_encode_stream_budget_batch, limg_hip_encode_stream_quality, limg_hip_encode_stream_quality_batch, limg_hip_encode_stream_list
// (a list of mixed shapes), limg_hip_encode_stream_quality_list, limg_hip_encode_stream_budget_list and limg_hip_stream_sizes_list, each with its _device form.  The 8x8 encode in compact mode + the packer of limg_hip_stream.hip; the size probe's kernels are limg_hip_rate.hip, the search limg_hip_rate_step.h; the quality
// entries measure with the error windows of limg_hip_stream_window_api.hip and search with limg_hip_quality_step.h.  What the twenty-four entries do alike -- a call's shape,
// the argument checks and how a list entry opens, a list's staging, the probe's parameters, the searches' enqueue, the results -- is written once, in the anonymous
// namespace below.  Which launches a list takes is decided in limg_hip_list_plan.h (list_route) and nowhere here: encode_list, budget_list and sizes_list walk its
// steps.  No kernel is defined here.
#include "limg_hip_context.h"
#include "limg_hip_quality_step.h"

#include <algorithm>
#include <vector>

using namespace limg_hip;

namespace
{
  typedef limg_hip_stream_list_item ListItem;

  // ---- a call's shape: everything the entries derive from (sizeX, sizeY) ----
  struct StreamShape : EncodeShape // blocks and strips; whole: the strip form of the packer, the batched kernels, the probe
  {
    size_t px, planeStride, tiles, bound;
    uint64_t fixedBytes; // header + table: a stream is this + 8 x its payload words
    StreamShape(size_t x, size_t y)
      : EncodeShape(x, y), px(x * y), planeStride((px + 255) & ~(size_t)255), tiles((blocks + 255) / 256), bound(limg_hip_stream_bound(x, y)),
        fixedBytes(sizeof(limg_hip_stream_header) + (uint64_t)blocks * sizeof(limg_hip_stream_block)) {}
  };

  // the probe kernel of one image: where a list goes in one launch pair (list_in_one_pair), under the default search
  bool rate_probe_applies(const limg_hip_context *c, const StreamShape &sh, int fast) { return list_in_one_pair(sh, c->opt) && fast != 0; }

  // ---- argument checks, in the contract's order (include/limg_hip.h) ----
  // The single entries.  pointers: the entry's other pointers are all there.  dStream: a device form's stream buffer, which must hold the bound and be 16-byte aligned.
  limg_hip_result check_single(const void *c, const void *pIn, bool pointers, const StreamShape &sh, const uint8_t *dStream = nullptr, size_t capacity = 0)
  {
    if (!c || !pIn || !pointers) return limg_hip_error_ArgumentNull;
    if (sh.bound == 0) return limg_hip_error_InvalidParameter;
    if (dStream && capacity < sh.bound) return limg_hip_error_OutOfBounds;
    if (((uintptr_t)dStream & 15u) != 0) return limg_hip_error_InvalidParameter;
    return limg_hip_success;
  }
  // The list entries; the element checks hold for the `count` elements there are.  deviceStreams: ppStreams are device buffers (16-byte aligned).
  limg_hip_result check_list(const void *c, bool pointers, size_t count, const uint32_t *const *ppIn, uint8_t *const *ppStreams, const StreamShape &sh, size_t capacityEach,
                             bool deviceStreams)
  {
    if (!c || !ppIn || !ppStreams || !pointers) return limg_hip_error_ArgumentNull;
    for (size_t i = 0; i < count; i++)
      if (!ppIn[i] || !ppStreams[i]) return limg_hip_error_ArgumentNull;
    if (sh.bound == 0) return limg_hip_error_InvalidParameter;
    if (capacityEach < sh.bound) return limg_hip_error_OutOfBounds;
    for (size_t i = 0; deviceStreams && i < count; i++)
      if (((uintptr_t)ppStreams[i] & 15u) != 0) return limg_hip_error_InvalidParameter;
    return limg_hip_success;
  }

  // minErrorFactor / maxErrorFactor of the search entries -> the bounds of h = errorFactor / 2, then the `count` results (RESULT: the budget or the quality entries')
  // and the budgets -- pMaxBytes == NULL: the quality entries, whose limit may be 0 (the bound rules hold for an empty list too)
  template <class RESULT>
  limg_hip_result check_search(size_t count, const size_t *pMaxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, const RESULT *pResults, uint32_t &hLo, uint32_t &hHi)
  {
    const uint32_t lo = minErrorFactor ? minErrorFactor : 2u, hi = maxErrorFactor ? maxErrorFactor : 1024u;
    if ((lo & 1u) || (hi & 1u) || lo < 2u || hi < 2u || lo > hi) return limg_hip_error_InvalidParameter;
    for (size_t i = 0; i < count; i++)
      if ((pMaxBytes && pMaxBytes[i] == 0) || pResults[i].struct_size < sizeof(RESULT)) return limg_hip_error_InvalidParameter;
    hLo = lo / 2u; hHi = hi / 2u;
    return limg_hip_success;
  }

  // The items as the caller's array holds them (itemSize apart), checked in the contract's order.  deviceForm: the streams are device buffers.  streams == false:
  // the call writes no stream (the sizes list) -- pStream and capacity are not read.
  limg_hip_result check_items(const void *c, bool pointers, size_t count, const ListItem *pItems, size_t itemSize, bool deviceForm, std::vector<ListItem> &items,
                              bool streams = true)
  {
    if (!c || !pItems || !pointers) return limg_hip_error_ArgumentNull;
    if (itemSize < sizeof(ListItem)) return limg_hip_error_InvalidParameter;
    items.resize(count);
    for (size_t i = 0; i < count; i++)
    {
      memcpy(&items[i], (const uint8_t *)pItems + i * itemSize, sizeof(ListItem));
      const ListItem &it = items[i];
      if (!it.pIn || (streams && !it.pStream)) return limg_hip_error_ArgumentNull;
      const size_t bound = (it.sizeX && it.sizeY) ? limg_hip_stream_bound(it.sizeX, it.sizeY) : 0;
      if (bound == 0) return limg_hip_error_InvalidParameter;
      if (streams && deviceForm && ((uintptr_t)it.pStream & 15u) != 0) return limg_hip_error_InvalidParameter;
      if (streams && deviceForm && it.capacity < bound) return limg_hip_error_OutOfBounds;
      if (it.reserved != 0) return limg_hip_error_InvalidParameter;
    }
    return limg_hip_success;
  }

  // ---- how every list entry opens: the list's own checks (check_list / check_items, its form's rule), the search's (search(count) -> its result; no_search where
  // there is none), then an empty list -- success with nothing done -- and a count beyond 31 bits.  go: the entry has work to do; else it returns the result ----
  limg_hip_result no_search(size_t) { return limg_hip_success; }
  template <class SEARCH>
  limg_hip_result open_list(limg_hip_result listChecks, size_t count, SEARCH &&search, bool &go)
  {
    go = false;
    limg_hip_result r = listChecks;
    if (r != limg_hip_success || (r = search(count)) != limg_hip_success || count == 0) return r;
    if (count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    go = true;
    return limg_hip_success;
  }

  // (the caller's struct_size may be larger than ours: only the members are written)
  void fill_result(limg_hip_budget_result &res, uint32_t ef, uint32_t probes, uint32_t within, uint64_t bytes) { res.errorFactor = ef; res.probes = probes; res.withinBudget = within; res.bytes = bytes; }
  void fill_result(limg_hip_quality_result &res, uint32_t ef, uint32_t probes, uint32_t within, uint64_t bytes, uint64_t errorSum)
  {
    res.errorFactor = ef; res.probes = probes; res.withinTarget = within; res.bytes = bytes; res.errorSum = errorSum;
  }

  // `count` sizes the device holds as 64-bit words -> the caller's size_t: ONE download, waits for `s`
  limg_hip_result download_sizes(const void *dSizes, size_t count, size_t *pBytes, hipStream_t s)
  {
    std::vector<unsigned long long> sizes(count);
    HIP_TRY(hipMemcpyAsync(sizes.data(), dSizes, count * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < count; i++) pBytes[i] = (size_t)sizes[i];
    return limg_hip_success;
  }

  // ---- the packers' set-up, single and batched ----
  uint32_t stream_flags(const limg_hip_context *c, int fast) { return (fast ? 1u : 0u) | (c->opt.dither_pcg ? 2u : 0u); }
  // the strip form's grid: 16 one-wave workgroups per CU (128 vector registers each: 4 per SIMD), no more than there are strips
  uint32_t pack_waves(const limg_hip_context *c, size_t strips)
  {
    const size_t slots = (size_t)device_cus(c) * 16;
    return (uint32_t)(strips < slots ? strips : slots);
  }

  // ---- a list, whichever way it came: items.  A same-shape list (ppIn, ppStreams, one shape, capacityEach) as items, and items as the arrays a same-shape entry takes ----
  // (efs: one error factor per image, else errorFactor for all)
  std::vector<ListItem> as_items(size_t n, const uint32_t *const *ppIn, uint8_t *const *ppStreams, size_t capacityEach, size_t sizeX, size_t sizeY, uint32_t errorFactor = 0,
                                 const uint32_t *efs = nullptr)
  {
    std::vector<ListItem> items(n);
    for (size_t i = 0; i < n; i++) items[i] = { ppIn[i], ppStreams[i], (uint64_t)capacityEach, (uint32_t)sizeX, (uint32_t)sizeY, efs ? efs[i] : errorFactor, 0u };
    return items;
  }
  struct ItemArrays
  {
    std::vector<const uint32_t *> in;
    std::vector<uint8_t *> streams;
    std::vector<uint32_t> efs;
    size_t capacityEach = SIZE_MAX; // the smallest of the items'
    explicit ItemArrays(const std::vector<ListItem> &items)
    {
      for (const ListItem &it : items) { in.push_back(it.pIn); streams.push_back(it.pStream); efs.push_back(it.errorFactor); capacityEach = std::min(capacityEach, (size_t)it.capacity); }
    }
  };

  // ---- host forms of the list entries.  Staging: the images side by side in host.in, the streams at worst-case size side by side in stream.buf, every slice
  // rounded up to 256 bytes; `staged`: the items with both pointers and the capacity replaced ----
  size_t stage_up(size_t v) { return (v + 255) & ~(size_t)255; }
  // the images alone (the sizes list, which writes no stream): `staged` = the items with pIn replaced
  limg_hip_result stage_inputs(limg_hip_context *c, const std::vector<ListItem> &items, std::vector<ListItem> &staged)
  {
    HIP_TRY(hipSetDevice(c->device));
    staged = items;
    size_t inBytes = 0;
    for (const ListItem &it : items) inBytes += stage_up((size_t)it.sizeX * it.sizeY * 4);
    const limg_hip_result r = c->host.in.ensure(inBytes);
    if (r != limg_hip_success) return r;
    size_t inAt = 0;
    for (size_t i = 0; i < items.size(); i++)
    {
      const size_t px4 = (size_t)items[i].sizeX * items[i].sizeY * 4;
      staged[i].pIn = (const uint32_t *)((const uint8_t *)c->host.in.p + inAt);
      HIP_TRY(hipMemcpy((void *)staged[i].pIn, items[i].pIn, px4, hipMemcpyHostToDevice));
      inAt += stage_up(px4);
    }
    return limg_hip_success;
  }
  limg_hip_result stage_items(limg_hip_context *c, const std::vector<ListItem> &items, std::vector<ListItem> &staged)
  {
    limg_hip_result r;
    if ((r = stage_inputs(c, items, staged)) != limg_hip_success) return r;
    size_t outBytes = 0;
    for (ListItem &it : staged) { it.capacity = stage_up(limg_hip_stream_bound(it.sizeX, it.sizeY)); outBytes += (size_t)it.capacity; }
    if ((r = c->stream.buf.ensure(outBytes)) != limg_hip_success) return r;
    size_t outAt = 0;
    for (ListItem &it : staged) { it.pStream = (uint8_t *)c->stream.buf.p + outAt; outAt += (size_t)it.capacity; }
    return limg_hip_success;
  }

  // fresh results for a host form's device call, which the caller's are filled from afterwards (its struct_size may be larger than ours)
  template <class RESULT>
  std::vector<RESULT> own_results(size_t count)
  {
    std::vector<RESULT> results(count);
    for (size_t i = 0; i < count; i++) { memset(&results[i], 0, sizeof(results[i])); results[i].struct_size = sizeof(RESULT); }
    return results;
  }

  // what the device call left for image i, to the caller -> the bytes of its stream.  The entries without a search report sizes.
  size_t report(size_t *to, const size_t *from, size_t i) { to[i] = from[i]; return from[i]; }
  size_t report(limg_hip_budget_result *to, const limg_hip_budget_result *from, size_t i)
  { fill_result(to[i], from[i].errorFactor, from[i].probes, from[i].withinBudget, from[i].bytes); return (size_t)from[i].bytes; }
  size_t report(limg_hip_quality_result *to, const limg_hip_quality_result *from, size_t i)
  { fill_result(to[i], from[i].errorFactor, from[i].probes, from[i].withinTarget, from[i].bytes, from[i].errorSum); return (size_t)from[i].bytes; }
  // A host form (its arguments have been checked): the staging, deviceCall(staged) on the null stream -- it leaves image i's result in own[i] --, the device status, every image's result
  // to the caller, OutOfBounds -- all reported, no stream written: the single host call's rule -- where a stream is larger than its item's capacity, then each stream down at its own size.
  template <class RESULT, class CALL>
  limg_hip_result host_list(limg_hip_context *c, const std::vector<ListItem> &items, const RESULT *own, RESULT *pResults, CALL &&deviceCall)
  {
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    std::vector<ListItem> staged;
    limg_hip_result r;
    if ((r = stage_items(c, items, staged)) != limg_hip_success) return r;
    if ((r = deviceCall(staged)) != limg_hip_success) return r;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r;
    std::vector<size_t> bytes(items.size());
    bool fits = true;
    for (size_t i = 0; i < items.size(); i++) { bytes[i] = report(pResults, own, i); fits = fits && bytes[i] <= items[i].capacity; }
    if (!fits) return limg_hip_error_OutOfBounds;
    for (size_t i = 0; i < items.size(); i++) HIP_TRY(hipMemcpy(items[i].pStream, staged[i].pStream, bytes[i], hipMemcpyDeviceToHost));
    return limg_hip_success;
  }

  // ---- size probe and budget search (kernels: limg_hip_rate.hip; the search: limg_hip_rate_step.h) ----
  // The probes of n images: one state and one counter per image, the probe kernel's parameters.  One shape: n == 1 the single-image kernels, n > 1 the _batch ones.
  // images != NULL: a chunk of mixed shapes, the _list probe and the _batch begin and step with the chunk's ListImage table (fixedBytes is then every image's own).
  struct Probe
  {
    size_t n; int channels; bool floatFast; uint64_t fixedBytes;
    RateDevice *states; unsigned long long *counters;
    RateProbeParams one; RateProbeBatchParams many;
    const ListImage *images = nullptr; RateProbeListParams list;
    bool single() const { return n == 1 && !images; }
    void launch(hipStream_t s) const
    {
      if (images) launch_rate_probe_list(list, channels, floatFast, s);
      else if (n == 1) launch_rate_probe(one, channels, floatFast, s);
      else launch_rate_probe_batch(many, channels, floatFast, s);
    }
    // between two probes; dList: the list form (sizes at dBytes, image after image)
    void step(hipStream_t s, const uint32_t *dList = nullptr, unsigned long long *dBytes = nullptr, uint32_t listCount = 0) const
    {
      if (single()) launch_rate_step(states, counters, fixedBytes, dList, dBytes, listCount, s);
      else launch_rate_step_batch(states, counters, (uint32_t)n, fixedBytes, s, images, dList, dBytes, listCount);
    }
  };

  // what RateProbeParams and RateProbeBatchParams name alike.  vecIn: 16-byte loads, which every image of the launch allows (vec_access)
  template <class P>
  void fill_probe(P &p, const limg_hip_context *c, const StreamShape &sh, bool vecIn)
  {
    memset(&p, 0, sizeof(p));
    p.sizeX = (uint32_t)sh.sizeX; p.sizeY = (uint32_t)sh.sizeY; p.blocksX = (uint32_t)sh.blocksX; p.blocksY = (uint32_t)sh.blocksY; p.stripsX = (uint32_t)sh.stripsX;
    p.vecIn = vecIn;
    p.recordLimit = record_limit(c);
    forced_shifts(c->opt.forced_shift, p.forced);
    p.records = (const limg_hip_block_record *)c->enc.records.p; p.invN = (const float *)c->enc.invN.p;
  }

  // The records of k_fit_tpb in the context's float mode (the `fitOnly` route, which the merged-block encoder's pass 1 also takes), image after image in enc.records
  // from ONE grid -- encode_params puts a list's image table on the device --, and the probe on them.
  limg_hip_result probe_setup(limg_hip_context *c, const StreamShape &sh, const uint32_t *const *ppIn, size_t n, int hasAlpha, int poolThreads, hipStream_t s, Probe &pr)
  {
    limg_hip_result r;
    if ((r = c->stream.rateState.ensure(n * sizeof(RateDevice))) != limg_hip_success) return r;
    if ((r = c->stream.rateCounter.ensure(n * 8)) != limg_hip_success) return r;
    std::vector<ImageIO> table(n > 1 ? n : 0);
    VecAccess vec = vec_access(ppIn[0], nullptr, sh.sizeX, false);
    for (size_t i = 0; i < n; i++) { vec &= vec_access(ppIn[i], nullptr, sh.sizeX, false); if (n > 1) table[i].in = ppIn[i]; }
    EncodeExtra x;
    x.fitOnly = true; x.fitFloatMode = true;
    if (n > 1) { x.batch = table.data(); x.batchCount = n; }
    if ((r = encode_device(c, ppIn[0], sh.sizeX, sh.sizeY, hasAlpha, nullptr, nullptr, 0, poolThreads, 1, s, x)) != limg_hip_success) return r;
    pr.n = n; pr.channels = hasAlpha ? 4 : 3; pr.floatFast = c->opt.float_mode == 1; pr.fixedBytes = sh.fixedBytes;
    pr.states = (RateDevice *)c->stream.rateState.p; pr.counters = (unsigned long long *)c->stream.rateCounter.p;
    fill_probe(pr.one, c, sh, vec.in);
    pr.one.io.in = ppIn[0]; pr.one.state = pr.states; pr.one.counter = pr.counters;
    fill_probe(pr.many, c, sh, vec.in);
    pr.many.batch = (const ImageIO *)c->enc.batchTable.p; pr.many.nImages = (uint32_t)n; pr.many.imageStrips = (uint32_t)sh.strips;
    pr.many.states = pr.states; pr.many.counters = pr.counters;
    return limg_hip_success;
  }

  // The probe of a chunk of n > 1 images of mixed shapes (eligible items: list_item_eligible): the chunk's tables and k_fit_tpb_list alone (encode_list_chunk's fitOnly
  // form) -- records and invN image after image from each image's firstBlock --, and k_rate_probe_list on them.  Everything it needs has been grown by the caller
  // (grow_list_probe).
  limg_hip_result list_probe_setup(limg_hip_context *c, const ListItem *its, size_t n, int hasAlpha, int poolThreads, hipStream_t s, Probe &pr)
  {
    const ChunkTables T = chunk_tables(n);
    std::vector<uint8_t> host(T.bytes, 0);
    uint8_t *const dev = (uint8_t *)c->stream.listTable.p;
    std::vector<ListChunkImage> images(n);
    for (size_t i = 0; i < n; i++) images[i] = { its[i].pIn, its[i].sizeX, its[i].sizeY, 0u, { nullptr, nullptr, nullptr } };
    ListChunkTotals tot;
    const limg_hip_result r = encode_list_chunk(c, images.data(), n, hasAlpha, poolThreads, nullptr, host.data(), dev, s, tot, true);
    if (r != limg_hip_success) return r;
    pr.n = n; pr.channels = hasAlpha ? 4 : 3; pr.floatFast = c->opt.float_mode == 1; pr.fixedBytes = 0;
    pr.states = (RateDevice *)c->stream.rateState.p; pr.counters = (unsigned long long *)c->stream.rateCounter.p;
    pr.images = (const ListImage *)(dev + T.images);
    RateProbeListParams &p = pr.list;
    memset(&p, 0, sizeof(p));
    p.images = pr.images; p.batch = (const ImageIO *)(dev + T.io); p.firstStrip = (const uint32_t *)(dev + T.firstStrip);
    p.nImages = (uint32_t)n; p.nStrips = tot.strips;
    p.recordLimit = record_limit(c);
    forced_shifts(c->opt.forced_shift, p.forced);
    p.records = (const limg_hip_block_record *)c->enc.records.p; p.invN = (const float *)c->enc.invN.p;
    p.states = pr.states; p.counters = pr.counters;
    return limg_hip_success;
  }

  // The searches of pr's n images over [hLo, hHi], image i's for budgets[i]: begin, then every launch any of them can need, enqueued at once -- probes behind the end of
  // an image's search return at once --, ONE download of the states and ONE wait.  hStates: n, host.
  limg_hip_result run_searches(const Probe &pr, const size_t *budgets, uint32_t hLo, uint32_t hHi, hipStream_t s, RateDevice *hStates)
  {
    const size_t n = pr.n;
    if (pr.single()) launch_rate_begin(pr.states, pr.counters, rate_begin(hLo, hHi, budgets[0]), 2u * hHi, s);
    else launch_rate_begin_batch(pr.states, pr.counters, budgets, n, hLo, hHi, s);
    for (uint32_t i = 0, probes = rate_max_probes(hLo, hHi); i < probes; i++)
    {
      pr.launch(s);
      pr.step(s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hStates, pr.states, n * sizeof(RateDevice), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++)
      if (!hStates[i].search.done) return limg_hip_error_Generic;
    return limg_hip_success;
  }
  // ... of n images of one shape
  limg_hip_result run_searches(limg_hip_context *c, const StreamShape &sh, const uint32_t *const *ppIn, const size_t *budgets, size_t n, uint32_t hLo, uint32_t hHi,
                               int hasAlpha, int poolThreads, hipStream_t s, RateDevice *hStates)
  {
    Probe pr;
    const limg_hip_result r = probe_setup(c, sh, ppIn, n, hasAlpha, poolThreads, s, pr);
    return r != limg_hip_success ? r : run_searches(pr, budgets, hLo, hHi, s, hStates);
  }
}

namespace
{
  // The sizes of `count` finished streams, gathered from their headers on the device: ONE download, waits for `s`.  images: the list (its `stream` members), which goes
  // into the context's table (stream.table, `count` entries) first; NULL: the table names the streams already.
  limg_hip_result list_bytes(limg_hip_context *c, const StreamImage *images, size_t count, size_t *pBytes, hipStream_t s)
  {
    limg_hip_result r;
    if ((r = c->stream.sizes.ensure(count * 8)) != limg_hip_success) return r;
    if (images) launch_set_stream_table((StreamImage *)c->stream.table.p, images, count, s);
    launch_stream_gather_bytes((const StreamImage *)c->stream.table.p, count, (unsigned long long *)c->stream.sizes.p, s);
    HIP_TRY(hipGetLastError());
    return download_sizes(c->stream.sizes.p, count, pBytes, s);
  }

  // ---- the lists' routes.  limg_hip_list_plan.h decides (list_route: which items take which launches, in which order, what restarts the statistics, what the
  // largest chunk needs); the walkers -- encode_list here, budget_list and sizes_list below -- grow what the plan's `most` says, loop over its steps and finish with
  // the sizes or the results.  They decide nothing.  Their lists are checked, not empty, and counted in 31 bits (open_list) ----
  ListPlan route(const limg_hip_context *c, const std::vector<ListItem> &items, ListJob job, bool sameShape, int fastBitCrushing)
  {
    std::vector<ListPlanItem> in(items.size());
    for (size_t i = 0; i < items.size(); i++) in[i] = list_plan_item(items[i].sizeX, items[i].sizeY, items[i].errorFactor, fastBitCrushing, c->opt);
    return list_route(in.data(), in.size(), job, sameShape, fastBitCrushing, c->opt, batch_hook(c));
  }
  // a step's items, in the step's order
  std::vector<ListItem> step_items(const std::vector<ListItem> &items, const ListPlan &plan, const ListStep &st)
  {
    std::vector<ListItem> its(st.count);
    for (size_t k = 0; k < st.count; k++) its[k] = items[plan.order[st.first + k]];
    return its;
  }

  // One chunk of n > 1 images of one shape: ONE compact-mode batched encode -- records, shift words and the strips' payload words in the context's raster arrays,
  // image after image; the factor planes in per-image slices of stream.fac -- and one scan + one pack launch over the chunk.  own: the encode is
  // k_encode_list_rated's (thresholds per image from a device table: `rated`, 32 bytes per image) and the scan writes every header's own error factor; else the
  // chunk shares its first image's.  table: the chunk's n entries of the streams' table.  Everything it needs has been grown by the caller.
  limg_hip_result same_chunk(limg_hip_context *c, const ListItem *its, size_t n, bool own, RatedImage *rated, StreamImage *table, int hasAlpha, int poolThreads,
                             int fastBitCrushing, hipStream_t s)
  {
    const StreamShape sh(its[0].sizeX, its[0].sizeY);
    std::vector<ImageIO> io(n, ImageIO{});
    std::vector<StreamImage> images(n);
    std::vector<uint32_t> efs(n);
    for (size_t i = 0; i < n; i++)
    {
      uint8_t *fac = (uint8_t *)c->stream.fac.p + i * 3 * sh.planeStride; // 256-byte aligned slices
      io[i].in = its[i].pIn;
      io[i].info.pFactorsA = fac; io[i].info.pFactorsB = fac + sh.planeStride; io[i].info.pFactorsC = fac + 2 * sh.planeStride;
      images[i].stream = its[i].pStream;
      images[i].fac[0] = fac; images[i].fac[1] = fac + sh.planeStride; images[i].fac[2] = fac + 2 * sh.planeStride;
      efs[i] = its[i].errorFactor;
    }
    limg_hip_compact_out comp = { (limg_hip_block_record *)c->enc.records.p, (uint32_t *)c->enc.shifts.p };
    EncodeExtra x;
    x.batch = io.data(); x.batchCount = n;
    x.streamRaw = true; x.stripWords = (uint32_t *)c->stream.units.p;
    if (own) { x.errorFactors = efs.data(); x.ratedTable = rated; }
    const limg_hip_result r = encode_device(c, its[0].pIn, sh.sizeX, sh.sizeY, hasAlpha, &io[0].info, &comp, efs[0], poolThreads, fastBitCrushing, s, x);
    if (r != limg_hip_success) return r;
    launch_set_stream_table(table, images.data(), n, s);
    StreamBatchParams b;
    memset(&b, 0, sizeof(b));
    b.sizeX = (uint32_t)sh.sizeX; b.sizeY = (uint32_t)sh.sizeY; b.blocksX = (uint32_t)sh.blocksX; b.blocksY = (uint32_t)sh.blocksY; b.nBlocks = (uint32_t)sh.blocks;
    b.channels = hasAlpha ? 4 : 3; b.errorFactor = efs[0]; b.flags = stream_flags(c, fastBitCrushing);
    b.stripsX = (uint32_t)sh.stripsX; b.imageStrips = (uint32_t)sh.strips; b.nImages = (uint32_t)n; b.nStrips = (uint32_t)(n * sh.strips);
    b.nWaves = pack_waves(c, n * sh.strips); // as the single call -- for the whole chunk
    b.images = table;
    b.records = comp.pRecords; b.shifts = comp.pShifts; b.stripWords = (uint32_t *)c->stream.units.p;
    b.rated = own ? rated : nullptr; // (the chunk's table, as the encode just wrote it)
    Timeline tl(c, s, 4); // {scan + pack of the chunk, -, -}
    tl.mark();
    launch_stream_pack_batch(b, s);
    tl.close();
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  // One chunk of eligible items of more than one shape: the images' factor planes in slices of stream.fac, the chunk's table block with this layer's part of it
  // (the StreamImage entries), the encode layer's launch pair on them (encode_list_chunk), ONE scan, ONE pack.  Everything it needs has been grown by the caller.
  limg_hip_result mixed_chunk(limg_hip_context *c, const ListItem *its, size_t n, int hasAlpha, int poolThreads, int fastBitCrushing, hipStream_t s)
  {
    const ChunkTables T = chunk_tables(n);
    std::vector<uint8_t> host(T.bytes, 0);
    uint8_t *const dev = (uint8_t *)c->stream.listTable.p;
    StreamImage *streams = (StreamImage *)(host.data() + T.streams);
    std::vector<ListChunkImage> images(n);
    size_t facAt = 0;
    for (size_t i = 0; i < n; i++)
    {
      const ListItem &it = its[i];
      images[i].in = it.pIn; images[i].sizeX = it.sizeX; images[i].sizeY = it.sizeY; images[i].errorFactor = it.errorFactor;
      for (int k = 0; k < 3; k++) { streams[i].fac[k] = images[i].fac[k] = (uint8_t *)c->stream.fac.p + facAt; facAt += list_plane_stride(it.sizeX, it.sizeY); }
      streams[i].stream = it.pStream;
    }
    uint32_t *const stripWords = (uint32_t *)c->stream.units.p;
    ListChunkTotals tot;
    const limg_hip_result r = encode_list_chunk(c, images.data(), n, hasAlpha, poolThreads, stripWords, host.data(), dev, s, tot);
    if (r != limg_hip_success) return r;
    StreamListParams b;
    memset(&b, 0, sizeof(b));
    b.images = (const ListImage *)(dev + T.images); b.streams = (const StreamImage *)(dev + T.streams); b.rated = (const RatedImage *)(dev + T.rated); b.firstStrip = (const uint32_t *)(dev + T.firstStrip);
    b.nImages = (uint32_t)n; b.nStrips = tot.strips; b.nWaves = pack_waves(c, tot.strips);
    b.channels = hasAlpha ? 4u : 3u; b.flags = stream_flags(c, fastBitCrushing);
    b.records = (const limg_hip_block_record *)c->enc.records.p; b.shifts = (const uint32_t *)c->enc.shifts.p; b.stripWords = stripWords;
    Timeline tl(c, s, 4); // {scan + pack of the chunk, -, -}
    tl.mark();
    launch_stream_pack_list(b, s);
    tl.close();
    HIP_TRY(hipGetLastError());
    return limg_hip_success;
  }

  // The encode of a list, item i at its own errorFactor (job: kListShared -- they are all the same -- or kListOwn), stream i what the single call writes for item i.
  // sameShape: a same-shape entry's list.  ratedStorage: device memory for the threshold table of an own-factor chunk (32 bytes per image) where the caller has some
  // to spare -- the budgeted list's search states, which its searches are done with --, else the context's own (stream.rated).  Everything the largest chunk needs
  // is there before the first launch: nothing is grown (and so freed) between the steps of a list.  limg_hip_last_stats: as the plan's `restart` says.
  limg_hip_result encode_list(limg_hip_context *c, const std::vector<ListItem> &items, ListJob job, bool sameShape, int hasAlpha, size_t *pBytes, int poolThreads,
                              int fastBitCrushing, void *stream, RatedImage *ratedStorage = nullptr)
  {
    const size_t count = items.size();
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const ListPlan plan = route(c, items, job, sameShape, fastBitCrushing);
    const ListNeeds &most = plan.most;
    limg_hip_result r;
    if ((r = c->stream.table.ensure(count * sizeof(StreamImage))) != limg_hip_success) return r;
    if (most.images > 1)
    {
      PersistentScratch ps;
      if (plan.mixed && (r = c->stream.listTable.ensure(chunk_tables(most.images).bytes)) != limg_hip_success) return r;
      if ((r = c->stream.fac.ensure(most.facBytes)) != limg_hip_success) return r;
      if ((r = c->stream.units.ensure((size_t)most.strips * 4)) != limg_hip_success) return r;
      if ((r = c->enc.records.ensure((size_t)most.blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
      if ((r = c->enc.shifts.ensure((size_t)most.blocks * 4)) != limg_hip_success) return r;
      if (plan.mixed && (r = c->enc.invN.ensure((size_t)most.blocks * 16)) != limg_hip_success) return r;
      if (plan.mixed && (r = persistent_scratch(c, (size_t)most.strips, 2, s, ps)) != limg_hip_success) return r;
      if (plan.rated && !ratedStorage)
      {
        if ((r = c->stream.rated.ensure(most.images * sizeof(RatedImage))) != limg_hip_success) return r;
        ratedStorage = (RatedImage *)c->stream.rated.p;
      }
    }
    std::vector<StreamImage> images(count); // the streams in list order, for the sizes
    for (size_t i = 0; i < count; i++) images[i].stream = items[i].pStream;
    StreamImage *const table = (StreamImage *)c->stream.table.p;
    for (const ListStep &st : plan.steps)
    {
      const size_t i = plan.order[st.first];
      c->stats.accumulate = !st.restart;
      if (st.kind == kStepSingle)
      {
        const ListItem &it = items[i];
        r = limg_hip_encode_stream_device(c, it.pIn, it.sizeX, it.sizeY, hasAlpha, it.pStream, (size_t)it.capacity, nullptr, it.errorFactor, poolThreads, fastBitCrushing, stream);
        if (r == limg_hip_success && pBytes && plan.inPlace) launch_set_stream_table(table + i, &images[i], 1, s); // (for the sizes below)
      }
      else if (st.kind == kStepSame) // (its table entries: at the step's place in the plan's order, which under inPlace is the list's)
        r = same_chunk(c, step_items(items, plan, st).data(), st.count, st.own, ratedStorage, table + st.first, hasAlpha, poolThreads, fastBitCrushing, s);
      else r = mixed_chunk(c, step_items(items, plan, st).data(), st.count, hasAlpha, poolThreads, fastBitCrushing, s);
      if (r != limg_hip_success) break;
    }
    c->stats.accumulate = false;
    if (r != limg_hip_success || !pBytes) return r;
    return list_bytes(c, plan.inPlace ? nullptr : images.data(), count, pBytes, s);
  }

  // ---- the same-shape encode entries, with one error factor (efs == NULL) or one per image (efs: host, count).  pointers: the entry's other pointers are there ----
  limg_hip_result stream_list_device(limg_hip_context *c, bool pointers, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                     uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, uint32_t errorFactor, const uint32_t *efs, int poolThreads,
                                     int fastBitCrushing, void *stream)
  {
    bool go;
    const limg_hip_result r = open_list(check_list(c, pointers, count, ppIn, ppStreams, StreamShape(sizeX, sizeY), capacityEach, true), count, no_search, go);
    if (!go) return r;
    return encode_list(c, as_items(count, ppIn, ppStreams, capacityEach, sizeX, sizeY, errorFactor, efs), efs ? kListOwn : kListShared, true, hasAlpha, pBytes, poolThreads,
                       fastBitCrushing, stream);
  }
  // the host form: upload, encode_list on the null stream, status, the streams down at their own sizes (capacityEach holds the bound: every stream fits)
  limg_hip_result stream_list_host(limg_hip_context *c, bool pointers, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                   uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, uint32_t errorFactor, const uint32_t *efs, int poolThreads, int fastBitCrushing)
  {
    bool go;
    const limg_hip_result r = open_list(check_list(c, pointers && pBytes != nullptr, count, ppIn, ppStreams, StreamShape(sizeX, sizeY), capacityEach, false), count, no_search, go);
    if (!go) return r;
    return host_list(c, as_items(count, ppIn, ppStreams, capacityEach, sizeX, sizeY, errorFactor, efs), pBytes, pBytes, [&](const std::vector<ListItem> &staged) {
      return encode_list(c, staged, efs ? kListOwn : kListShared, true, hasAlpha, pBytes, poolThreads, fastBitCrushing, nullptr);
    });
  }

  // ---- the byte budget and the size probe of a list (kernels: limg_hip_rate.hip -- of a mixed chunk k_rate_probe_list and the _batch begin / step with the chunk's
  // ListImage table) ----
  // everything the probes of the largest mixed chunk need, before the first launch: the tables, the fit grid's records, invN and look-back words, one state and one
  // counter per image
  limg_hip_result grow_list_probe(limg_hip_context *c, const ListNeeds &most)
  {
    limg_hip_result r;
    if ((r = c->stream.listTable.ensure(chunk_tables(most.images).bytes)) != limg_hip_success) return r;
    if ((r = c->enc.records.ensure((size_t)most.blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
    if ((r = c->enc.invN.ensure((size_t)most.blocks * 16)) != limg_hip_success) return r;
    if ((r = c->enc.lookback.ensure(16 * 2 + (size_t)most.strips * 8)) != limg_hip_success) return r;
    if ((r = c->stream.rateState.ensure(most.images * sizeof(RateDevice))) != limg_hip_success) return r;
    return c->stream.rateCounter.ensure(most.images * 8);
  }

  // The budgeted list: result i and stream i the single budget call's for item i with pMaxBytes[i].  A chunk's records come from ONE grid (k_fit_tpb for one shape,
  // k_fit_tpb_list for a mixed chunk), its searches are 1 + 2 x rate_max_probes launches with ONE download and ONE wait; then the chunk is ONE list encode at the
  // error factors the searches chose -- encode_list on the chunk (it runs its own float stage: reusing the probe's records is a follow-up), whose statistics are
  // those limg_hip_last_stats reports.
  limg_hip_result budget_list(limg_hip_context *c, const std::vector<ListItem> &items, bool sameShape, int hasAlpha, const size_t *pMaxBytes, uint32_t minErrorFactor,
                              uint32_t maxErrorFactor, uint32_t hLo, uint32_t hHi, int poolThreads, int fastBitCrushing, limg_hip_budget_result *pResults, void *stream)
  {
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const ListPlan plan = route(c, items, kListBudget, sameShape, fastBitCrushing);
    limg_hip_result r;
    if (plan.mixed && (r = grow_list_probe(c, plan.most)) != limg_hip_success) return r;
    std::vector<RateDevice> states;
    std::vector<size_t> budgets;
    for (const ListStep &st : plan.steps)
    {
      const size_t *idx = &plan.order[st.first], m = st.count;
      if (st.kind == kStepSingle)
      {
        const ListItem &it = items[idx[0]];
        if ((r = limg_hip_encode_stream_budget_device(c, it.pIn, it.sizeX, it.sizeY, hasAlpha, it.pStream, (size_t)it.capacity, pMaxBytes[idx[0]], minErrorFactor, maxErrorFactor,
                                                      poolThreads, fastBitCrushing, &pResults[idx[0]], stream)) != limg_hip_success)
          return r;
        continue;
      }
      // 1. + 2. the chunk's records and its searches
      std::vector<ListItem> its = step_items(items, plan, st);
      states.resize(m); budgets.resize(m);
      for (size_t k = 0; k < m; k++) budgets[k] = pMaxBytes[idx[k]];
      Probe pr;
      if (st.kind == kStepMixed) r = list_probe_setup(c, its.data(), m, hasAlpha, poolThreads, s, pr);
      else r = probe_setup(c, StreamShape(its[0].sizeX, its[0].sizeY), ItemArrays(its).in.data(), m, hasAlpha, poolThreads, s, pr);
      if (r != limg_hip_success || (r = run_searches(pr, budgets.data(), hLo, hHi, s, states.data())) != limg_hip_success) return r;
      // 3. the final encodes, whatever the searches chose: the chunk as a list at the chosen factors.  One shape: thresholds per image, or, where all chose the same
      // value, the shared-factor list, whose thresholds are kernel arguments; the threshold table -- 32 bytes per image -- in the chunk's search states -- 72 per
      // image --, which are on the host by now: no context memory of its own
      static_assert(sizeof(RatedImage) <= sizeof(RateDevice), "the threshold table fits the search states");
      bool same = true;
      for (size_t k = 0; k < m; k++) { its[k].errorFactor = 2u * states[k].search.next; same = same && its[k].errorFactor == its[0].errorFactor; }
      if (st.kind == kStepMixed) r = encode_list(c, its, kListOwn, false, hasAlpha, nullptr, poolThreads, fastBitCrushing, stream);
      else r = encode_list(c, its, same ? kListShared : kListOwn, true, hasAlpha, nullptr, poolThreads, fastBitCrushing, stream, (RatedImage *)c->stream.rateState.p);
      if (r != limg_hip_success) return r;
      for (size_t k = 0; k < m; k++) // bytes: what the probe measured at the result -- the packer's totalBytes
        fill_result(pResults[idx[k]], its[k].errorFactor, states[k].search.probes, states[k].search.within, states[k].search.bestBytes);
    }
    return limg_hip_success;
  }

  // The sizes of every item at every factor (factorCount in 1 .. 2^31 - 1): pBytes[i * factorCount + k].  Per mixed chunk ONE k_fit_tpb_list grid, one begin,
  // factorCount pairs of k_rate_probe_list and the list form of the step, ONE download and ONE wait.  The single call is limg_hip_stream_sizes_device, which has its
  // own fallback.
  limg_hip_result sizes_list(limg_hip_context *c, const std::vector<ListItem> &items, int hasAlpha, const uint32_t *pErrorFactors, size_t factorCount, size_t *pBytes,
                             int poolThreads, int fastBitCrushing, void *stream)
  {
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const ListPlan plan = route(c, items, kListSizes, false, fastBitCrushing);
    limg_hip_result r;
    if (plan.mixed)
    {
      if ((r = grow_list_probe(c, plan.most)) != limg_hip_success) return r;
      if ((r = c->stream.rateList.ensure(plan.most.images * factorCount * 8 + factorCount * 4)) != limg_hip_success) return r;
    }
    const std::vector<uint32_t> list(pErrorFactors, pErrorFactors + factorCount); // (the caller's array may be pageable and may die when the call returns)
    std::vector<size_t> sizes;
    for (const ListStep &st : plan.steps)
    {
      const size_t *idx = &plan.order[st.first], m = st.count;
      if (st.kind == kStepSingle)
      {
        const ListItem &it = items[idx[0]];
        if ((r = limg_hip_stream_sizes_device(c, it.pIn, it.sizeX, it.sizeY, hasAlpha, pErrorFactors, factorCount, pBytes + idx[0] * factorCount, poolThreads, fastBitCrushing,
                                              stream)) != limg_hip_success)
          return r;
        continue;
      }
      Probe pr;
      if ((r = list_probe_setup(c, step_items(items, plan, st).data(), m, hasAlpha, poolThreads, s, pr)) != limg_hip_success) return r;
      unsigned long long *dBytes = (unsigned long long *)c->stream.rateList.p;
      uint32_t *dList = (uint32_t *)(dBytes + m * factorCount);
      HIP_TRY(hipMemcpyAsync(dList, list.data(), factorCount * 4, hipMemcpyHostToDevice, s));
      launch_rate_begin_batch(pr.states, pr.counters, nullptr, m, 0, 0, s, dList);
      for (size_t k = 0; k < factorCount; k++)
      {
        pr.launch(s);
        pr.step(s, dList, dBytes, (uint32_t)factorCount);
      }
      HIP_TRY(hipGetLastError());
      sizes.resize(m * factorCount);
      if ((r = download_sizes(dBytes, m * factorCount, sizes.data(), s)) != limg_hip_success) return r; // (its wait also: `list` is no longer read by this chunk)
      for (size_t k = 0; k < m; k++)
        for (size_t f = 0; f < factorCount; f++) pBytes[idx[k] * factorCount + f] = sizes[k * factorCount + f];
    }
    return limg_hip_success;
  }
}

extern "C"
{
  limg_hip_result limg_hip_encode_stream_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                size_t *pBytes, uint32_t errorFactor, int poolThreads, int fastBitCrushing, void *stream)
  {
    const StreamShape sh(sizeX, sizeY);
    limg_hip_result r;
    if ((r = check_single(c, pIn, pStream != nullptr, sh, pStream, capacity)) != limg_hip_success) return r;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if ((r = c->stream.fac.ensure(sh.planeStride * 3)) != limg_hip_success) return r;
    // strip form of the packer (images of whole blocks): the encode kernel leaves one payload-word count per work strip (limg_hip_stream.hip)
    const bool stripForm = sh.whole && c->opt.force_split_kernels == 0;
    if ((r = c->stream.tiles.ensure(sh.tiles * 4)) != limg_hip_success) return r;
    if (stripForm && (r = c->stream.units.ensure(sh.strips * 4)) != limg_hip_success) return r;
    if ((r = c->enc.records.ensure(sh.blocks * sizeof(limg_hip_block_record))) != limg_hip_success) return r;
    if ((r = c->enc.shifts.ensure(sh.blocks * 4)) != limg_hip_success) return r;
    limg_hip_encode3d_info info;
    memset(&info, 0, sizeof(info));
    info.pFactorsA = (uint8_t *)c->stream.fac.p; info.pFactorsB = info.pFactorsA + sh.planeStride; info.pFactorsC = info.pFactorsB + sh.planeStride;
    limg_hip_compact_out comp = { (limg_hip_block_record *)c->enc.records.p, (uint32_t *)c->enc.shifts.p };
    EncodeExtra xs;
    xs.streamRaw = true; xs.stripWords = stripForm ? (uint32_t *)c->stream.units.p : nullptr;
    if ((r = encode_device(c, pIn, sizeX, sizeY, hasAlpha, &info, &comp, errorFactor, poolThreads, fastBitCrushing, s, xs)) != limg_hip_success) return r;

    StreamParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.sizeX = (uint32_t)sizeX; sp.sizeY = (uint32_t)sizeY; sp.blocksX = (uint32_t)sh.blocksX; sp.blocksY = (uint32_t)sh.blocksY;
    sp.nBlocks = (uint32_t)sh.blocks; sp.nTiles = (uint32_t)sh.tiles; sp.channels = hasAlpha ? 4 : 3; sp.errorFactor = errorFactor;
    sp.flags = stream_flags(c, fastBitCrushing);
    sp.fac[0] = info.pFactorsA; sp.fac[1] = info.pFactorsB; sp.fac[2] = info.pFactorsC;
    sp.records = comp.pRecords; sp.shifts = comp.pShifts;
    sp.stream = pStream; sp.tileBase = (uint32_t *)c->stream.tiles.p;
    if (stripForm)
    {
      sp.stripWords = (uint32_t *)c->stream.units.p;
      sp.stripsX = (uint32_t)sh.stripsX; sp.nStrips = (uint32_t)sh.strips;
      sp.nWaves = pack_waves(c, sh.strips);
    }
    Timeline tl(c, s, 4); // {scan + pack, -, -}
    tl.mark();
    launch_stream_pack(sp, s);
    tl.close();
    HIP_TRY(hipGetLastError());
    return pBytes ? stream_total_bytes(pStream, s, pBytes) : limg_hip_success;
  }

  limg_hip_result limg_hip_encode_stream(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity, size_t *pBytes,
                                         uint32_t errorFactor, int poolThreads, int fastBitCrushing)
  {
    const StreamShape sh(sizeX, sizeY);
    const limg_hip_result ok = check_single(c, pIn, pStream && pBytes, sh);
    if (ok != limg_hip_success) return ok;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    return encode_stream_host(c, pIn, sizeX, sizeY, pStream, capacity, pBytes, sh.bound, [&](const uint32_t *dIn, uint8_t *dStream, size_t bound, size_t *bytes) {
      return limg_hip_encode_stream_device(c, dIn, sizeX, sizeY, hasAlpha, dStream, bound, bytes, errorFactor, poolThreads, fastBitCrushing, nullptr);
    });
  }

  // ---- size probe and budget search (contract: include/limg_hip.h) ----
  limg_hip_result limg_hip_stream_sizes_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const uint32_t *pErrorFactors, size_t count,
                                               size_t *pBytes, int poolThreads, int fastBitCrushing, void *stream)
  {
    const StreamShape sh(sizeX, sizeY);
    limg_hip_result r;
    if ((r = check_single(c, pIn, pErrorFactors && pBytes, sh)) != limg_hip_success) return r;
    if (count == 0) return limg_hip_success;
    if (count > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (!rate_probe_applies(c, sh, fastBitCrushing))
    { // one ordinary stream encode per entry, into context staging
      if ((r = c->stream.buf.ensure(sh.bound)) != limg_hip_success) return r;
      for (size_t i = 0; i < count; i++)
        if ((r = limg_hip_encode_stream_device(c, pIn, sizeX, sizeY, hasAlpha, (uint8_t *)c->stream.buf.p, sh.bound, &pBytes[i], pErrorFactors[i], poolThreads, fastBitCrushing,
                                               stream)) != limg_hip_success)
          return r;
      return limg_hip_success;
    }
    if ((r = c->stream.rateList.ensure(count * 12)) != limg_hip_success) return r;
    Probe pr;
    if ((r = probe_setup(c, sh, &pIn, 1, hasAlpha, poolThreads, s, pr)) != limg_hip_success) return r;
    unsigned long long *dBytes = (unsigned long long *)c->stream.rateList.p;
    uint32_t *dList = (uint32_t *)(dBytes + count);
    std::vector<uint32_t> list(pErrorFactors, pErrorFactors + count); // (the caller's array may be pageable and may die when the call returns)
    HIP_TRY(hipMemcpyAsync(dList, list.data(), count * 4, hipMemcpyHostToDevice, s));
    launch_rate_begin(pr.states, pr.counters, rate_begin(0, 0, 0), list[0], s);
    for (size_t i = 0; i < count; i++)
    {
      pr.launch(s);
      pr.step(s, dList, dBytes, (uint32_t)count);
    }
    HIP_TRY(hipGetLastError());
    return download_sizes(dBytes, count, pBytes, s); // (its wait also: `list` is no longer read)
  }

  limg_hip_result limg_hip_stream_sizes(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, const uint32_t *pErrorFactors, size_t count,
                                        size_t *pBytes, int poolThreads, int fastBitCrushing)
  {
    limg_hip_result r;
    if ((r = check_single(c, pIn, pErrorFactors && pBytes, StreamShape(sizeX, sizeY))) != limg_hip_success) return r;
    if (count == 0) return limg_hip_success;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    uint8_t *const noStream = nullptr;
    std::vector<ListItem> staged;
    if ((r = stage_inputs(c, as_items(1, &pIn, &noStream, 0, sizeX, sizeY), staged)) != limg_hip_success) return r;
    r = limg_hip_stream_sizes_device(c, staged[0].pIn, sizeX, sizeY, hasAlpha, pErrorFactors, count, pBytes, poolThreads, fastBitCrushing, nullptr);
    return r != limg_hip_success ? r : limg_hip_check_device_status(c);
  }

  limg_hip_result limg_hip_encode_stream_budget_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                       size_t maxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                       limg_hip_budget_result *pResult, void *stream)
  {
    const StreamShape sh(sizeX, sizeY);
    uint32_t hLo, hHi;
    limg_hip_result r;
    if ((r = check_single(c, pIn, pStream && pResult, sh, pStream, capacity)) != limg_hip_success) return r;
    if ((r = check_search(1, &maxBytes, minErrorFactor, maxErrorFactor, pResult, hLo, hHi)) != limg_hip_success) return r;
    HIP_TRY(hipSetDevice(c->device));
    RateDevice search;
    RateState &st = search.search = rate_begin(hLo, hHi, maxBytes);
    size_t bytes = 0;
    bool written = false; // pStream holds the stream at the result
    if (rate_probe_applies(c, sh, fastBitCrushing) &&
        (r = run_searches(c, sh, &pIn, &maxBytes, 1, hLo, hHi, hasAlpha, poolThreads, (hipStream_t)stream, &search)) != limg_hip_success)
      return r;
    while (!st.done)
    { // no probe kernel (behind one the search is over): the same search, a whole stream encode per size
      const uint32_t h = st.next;
      if ((r = limg_hip_encode_stream_device(c, pIn, sizeX, sizeY, hasAlpha, pStream, capacity, &bytes, 2u * h, poolThreads, fastBitCrushing, stream)) != limg_hip_success) return r;
      rate_step(st, bytes);
      written = st.done && st.next == h;
    }
    // bytes: the final encode's, from its header
    if (!written && (r = limg_hip_encode_stream_device(c, pIn, sizeX, sizeY, hasAlpha, pStream, capacity, &bytes, 2u * st.next, poolThreads, fastBitCrushing, stream)) != limg_hip_success)
      return r;
    fill_result(*pResult, 2u * st.next, st.probes, st.within, bytes);
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode_stream_budget(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                size_t maxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                limg_hip_budget_result *pResult)
  {
    const StreamShape sh(sizeX, sizeY);
    uint32_t hLo, hHi;
    limg_hip_result ok;
    if ((ok = check_single(c, pIn, pStream && pResult, sh)) != limg_hip_success) return ok;
    if ((ok = check_search(1, &maxBytes, minErrorFactor, maxErrorFactor, pResult, hLo, hHi)) != limg_hip_success) return ok;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    size_t bytes = 0;
    return encode_stream_host(c, pIn, sizeX, sizeY, pStream, capacity, &bytes, sh.bound, [&](const uint32_t *dIn, uint8_t *dStream, size_t bound, size_t *n) {
      const limg_hip_result r = limg_hip_encode_stream_budget_device(c, dIn, sizeX, sizeY, hasAlpha, dStream, bound, maxBytes, minErrorFactor, maxErrorFactor, poolThreads,
                                                                     fastBitCrushing, pResult, nullptr);
      if (r == limg_hip_success) *n = (size_t)pResult->bytes;
      return r;
    });
  }

  // ---- batched stream encode: a list of same-shape images, stream i = limg_hip_encode_stream_device of image i (stream_list_device / stream_list_host above) ----
  limg_hip_result limg_hip_encode_stream_batch_device(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                      uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, uint32_t errorFactor, int poolThreads,
                                                      int fastBitCrushing, void *stream)
  {
    return stream_list_device(c, true, count, ppIn, sizeX, sizeY, hasAlpha, ppStreams, capacityEach, pBytes, errorFactor, nullptr, poolThreads, fastBitCrushing, stream);
  }

  limg_hip_result limg_hip_encode_stream_batch(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                               uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, uint32_t errorFactor, int poolThreads, int fastBitCrushing)
  {
    return stream_list_host(c, true, count, ppIn, sizeX, sizeY, hasAlpha, ppStreams, capacityEach, pBytes, errorFactor, nullptr, poolThreads, fastBitCrushing);
  }

  // ... and each image at its own error factor: stream i = limg_hip_encode_stream_device of image i at pErrorFactors[i]
  limg_hip_result limg_hip_encode_stream_batch_ef_device(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                         uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, const uint32_t *pErrorFactors, int poolThreads,
                                                         int fastBitCrushing, void *stream)
  {
    return stream_list_device(c, pErrorFactors != nullptr, count, ppIn, sizeX, sizeY, hasAlpha, ppStreams, capacityEach, pBytes, 0, pErrorFactors, poolThreads, fastBitCrushing,
                              stream);
  }

  limg_hip_result limg_hip_encode_stream_batch_ef(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                  uint8_t *const *ppStreams, size_t capacityEach, size_t *pBytes, const uint32_t *pErrorFactors, int poolThreads,
                                                  int fastBitCrushing)
  {
    return stream_list_host(c, pErrorFactors != nullptr, count, ppIn, sizeX, sizeY, hasAlpha, ppStreams, capacityEach, pBytes, 0, pErrorFactors, poolThreads, fastBitCrushing);
  }

  // ---- budgeted stream encode of a list: result i = limg_hip_encode_stream_budget_device of image i with pMaxBytes[i] (contract: include/limg_hip.h; budget_list above) ----
  limg_hip_result limg_hip_encode_stream_budget_batch_device(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                             uint8_t *const *ppStreams, size_t capacityEach, const size_t *pMaxBytes, uint32_t minErrorFactor,
                                                             uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing, limg_hip_budget_result *pResults, void *stream)
  {
    uint32_t hLo, hHi;
    bool go;
    const limg_hip_result r = open_list(check_list(c, pMaxBytes && pResults, count, ppIn, ppStreams, StreamShape(sizeX, sizeY), capacityEach, true), count,
                                        [&](size_t n) { return check_search(n, pMaxBytes, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    if (!go) return r;
    return budget_list(c, as_items(count, ppIn, ppStreams, capacityEach, sizeX, sizeY), true, hasAlpha, pMaxBytes, minErrorFactor, maxErrorFactor, hLo, hHi, poolThreads,
                       fastBitCrushing, pResults, stream);
  }

  limg_hip_result limg_hip_encode_stream_budget_batch(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                      uint8_t *const *ppStreams, size_t capacityEach, const size_t *pMaxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor,
                                                      int poolThreads, int fastBitCrushing, limg_hip_budget_result *pResults)
  {
    uint32_t hLo, hHi;
    bool go; // (capacityEach: host_list's rule, behind the encode)
    const limg_hip_result r = open_list(check_list(c, pMaxBytes && pResults, count, ppIn, ppStreams, StreamShape(sizeX, sizeY), SIZE_MAX, false), count,
                                        [&](size_t n) { return check_search(n, pMaxBytes, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    if (!go) return r;
    std::vector<limg_hip_budget_result> results = own_results<limg_hip_budget_result>(count);
    return host_list(c, as_items(count, ppIn, ppStreams, capacityEach, sizeX, sizeY), results.data(), pResults, [&](const std::vector<ListItem> &staged) {
      return budget_list(c, staged, true, hasAlpha, pMaxBytes, minErrorFactor, maxErrorFactor, hLo, hHi, poolThreads, fastBitCrushing, results.data(), nullptr);
    });
  }
}

// ---- stream encode to a quality target (contract: include/limg_hip.h; the search: limg_hip_quality_step.h) ----
namespace
{
  // The searches of n images over [hLo, hHi], image i's for limits[i], round by round: the images whose search is not over are encoded at their own next value by ONE
  // limg_hip_encode_stream_batch_ef_device call (a list of one: the single stream encode) into their own buffers, measured against their own pixels by ONE error
  // launch over the whole images and stepped behind ONE download of the round's sums, which waits for `stream`.  Then at most one more list encode, for the images
  // whose buffer does not hold the stream of their result, and the streams' sizes from their headers.  The arguments have been checked.
  // items: image i's pixels, stream buffer, capacity and size (its errorFactor is not read); mixed: the shapes may differ -- the rounds' encodes are then
  // limg_hip_encode_stream_list_device calls (the error launch takes jobs of any shape as it is)
  limg_hip_result quality_searches(limg_hip_context *c, size_t n, const limg_hip_stream_list_item *items, bool mixed, int hasAlpha, const uint64_t *limits, uint32_t hLo,
                                   uint32_t hHi, int poolThreads, int fastBitCrushing, limg_hip_quality_result *pResults, void *stream)
  {
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    limg_hip_result r;
    if ((r = c->stream.errorSums.ensure(n * 8)) != limg_hip_success) return r;
    if ((r = c->stream.table.ensure(n * sizeof(StreamImage))) != limg_hip_success) return r;
    std::vector<QualityState> st(n);
    std::vector<uint32_t> held(n, 0u); // the h whose stream image i's buffer holds (0: none yet)
    for (size_t i = 0; i < n; i++) st[i] = quality_begin(hLo, hHi, limits[i]);
    std::vector<size_t> active;
    std::vector<limg_hip_stream_list_item> list;
    std::vector<limg_hip_error_window_job> jobs;
    std::vector<unsigned long long> sums;
    // the images of `active` at 2 x their search's next value (where it is over: at the result)
    auto encode_active = [&]() {
      list.clear();
      for (size_t i : active)
      {
        held[i] = quality_next(st[i]);
        list.push_back(items[i]); list.back().errorFactor = 2u * held[i]; list.back().reserved = 0;
      }
      if (mixed) return limg_hip_encode_stream_list_device(c, list.size(), list.data(), sizeof(limg_hip_stream_list_item), hasAlpha, nullptr, poolThreads, fastBitCrushing, stream);
      const ItemArrays a(list);
      return limg_hip_encode_stream_batch_ef_device(c, list.size(), a.in.data(), items[0].sizeX, items[0].sizeY, hasAlpha, a.streams.data(), a.capacityEach, nullptr, a.efs.data(),
                                                    poolThreads, fastBitCrushing, stream);
    };
    for (uint32_t round = 0, most = rate_max_probes(hLo, hHi); round <= most; round++)
    {
      active.clear();
      for (size_t i = 0; i < n; i++)
        if (!quality_done(st[i])) active.push_back(i);
      if (active.empty()) break;
      if (round == most) return limg_hip_error_Generic; // (cannot happen: no search asks for more)
      if ((r = encode_active()) != limg_hip_success) return r;
      jobs.clear();
      for (size_t i : active)
      { // (streamBytes: the buffer's size -- the stream's own length is in its header, on the device)
        const size_t sizeX = items[i].sizeX, sizeY = items[i].sizeY;
        const limg_hip_error_window_job j = { items[i].pStream, (size_t)items[i].capacity, sizeX, sizeY, { 0, 0, sizeX, sizeY, items[i].pIn, sizeX } };
        jobs.push_back(j);
      }
      if ((r = limg_hip_decode_stream_windows_error_device(c, jobs.data(), jobs.size(), (uint64_t *)c->stream.errorSums.p, nullptr, stream)) != limg_hip_success) return r;
      sums.resize(active.size());
      HIP_TRY(hipMemcpyAsync(sums.data(), c->stream.errorSums.p, active.size() * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (size_t k = 0; k < active.size(); k++) quality_step(st[active[k]], sums[k]);
    }
    active.clear();
    for (size_t i = 0; i < n; i++)
      if (held[i] != quality_next(st[i])) active.push_back(i);
    if (!active.empty() && (r = encode_active()) != limg_hip_success) return r;
    // bytes: the totalBytes of the streams the buffers hold now
    std::vector<StreamImage> images(n);
    std::vector<size_t> bytes(n);
    for (size_t i = 0; i < n; i++) images[i].stream = items[i].pStream;
    if ((r = list_bytes(c, images.data(), n, bytes.data(), s)) != limg_hip_success) return r;
    for (size_t i = 0; i < n; i++)
      fill_result(pResults[i], 2u * quality_next(st[i]), quality_probes(st[i]), quality_within(st[i]), bytes[i], quality_error_sum(st[i]));
    return limg_hip_success;
  }

  // the host form of both list entries (the arguments have been checked)
  limg_hip_result quality_list_host(limg_hip_context *c, const std::vector<ListItem> &items, bool mixed, int hasAlpha, const uint64_t *limits, uint32_t hLo, uint32_t hHi,
                                    int poolThreads, int fastBitCrushing, limg_hip_quality_result *pResults)
  {
    std::vector<limg_hip_quality_result> results = own_results<limg_hip_quality_result>(items.size());
    return host_list(c, items, results.data(), pResults, [&](const std::vector<ListItem> &staged) {
      return quality_searches(c, staged.size(), staged.data(), mixed, hasAlpha, limits, hLo, hHi, poolThreads, fastBitCrushing, results.data(), nullptr);
    });
  }
}

extern "C"
{
  limg_hip_result limg_hip_encode_stream_quality_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                        uint64_t maxErrorSum, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                        limg_hip_quality_result *pResult, void *stream)
  {
    const StreamShape sh(sizeX, sizeY);
    uint32_t hLo, hHi;
    limg_hip_result r;
    if ((r = check_single(c, pIn, pStream && pResult, sh, pStream, capacity)) != limg_hip_success) return r;
    if ((r = check_search(1, nullptr, minErrorFactor, maxErrorFactor, pResult, hLo, hHi)) != limg_hip_success) return r;
    return quality_searches(c, 1, as_items(1, &pIn, &pStream, capacity, sizeX, sizeY).data(), false, hasAlpha, &maxErrorSum, hLo, hHi, poolThreads, fastBitCrushing, pResult, stream);
  }

  limg_hip_result limg_hip_encode_stream_quality(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t sizeY, int hasAlpha, uint8_t *pStream, size_t capacity,
                                                 uint64_t maxErrorSum, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                 limg_hip_quality_result *pResult)
  {
    const StreamShape sh(sizeX, sizeY);
    uint32_t hLo, hHi;
    limg_hip_result ok;
    if ((ok = check_single(c, pIn, pStream && pResult, sh)) != limg_hip_success) return ok;
    if ((ok = check_search(1, nullptr, minErrorFactor, maxErrorFactor, pResult, hLo, hHi)) != limg_hip_success) return ok;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    size_t bytes = 0;
    return encode_stream_host(c, pIn, sizeX, sizeY, pStream, capacity, &bytes, sh.bound, [&](const uint32_t *dIn, uint8_t *dStream, size_t bound, size_t *n) {
      const limg_hip_result r = limg_hip_encode_stream_quality_device(c, dIn, sizeX, sizeY, hasAlpha, dStream, bound, maxErrorSum, minErrorFactor, maxErrorFactor, poolThreads,
                                                                      fastBitCrushing, pResult, nullptr);
      if (r == limg_hip_success) *n = (size_t)pResult->bytes;
      return r;
    });
  }

  // ---- ... of a list: result i = limg_hip_encode_stream_quality_device of image i with pMaxErrorSums[i] ----
  limg_hip_result limg_hip_encode_stream_quality_batch_device(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                              uint8_t *const *ppStreams, size_t capacityEach, const uint64_t *pMaxErrorSums, uint32_t minErrorFactor,
                                                              uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing, limg_hip_quality_result *pResults, void *stream)
  {
    uint32_t hLo, hHi;
    bool go;
    const limg_hip_result r = open_list(check_list(c, pMaxErrorSums && pResults, count, ppIn, ppStreams, StreamShape(sizeX, sizeY), capacityEach, true), count,
                                        [&](size_t n) { return check_search(n, nullptr, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    if (!go) return r;
    return quality_searches(c, count, as_items(count, ppIn, ppStreams, capacityEach, sizeX, sizeY).data(), false, hasAlpha, pMaxErrorSums, hLo, hHi, poolThreads, fastBitCrushing, pResults,
                            stream);
  }

  limg_hip_result limg_hip_encode_stream_quality_batch(limg_hip_context *c, size_t count, const uint32_t *const *ppIn, size_t sizeX, size_t sizeY, int hasAlpha,
                                                       uint8_t *const *ppStreams, size_t capacityEach, const uint64_t *pMaxErrorSums, uint32_t minErrorFactor,
                                                       uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing, limg_hip_quality_result *pResults)
  {
    uint32_t hLo, hHi;
    bool go; // (capacityEach: host_list's rule, behind the encode)
    const limg_hip_result r = open_list(check_list(c, pMaxErrorSums && pResults, count, ppIn, ppStreams, StreamShape(sizeX, sizeY), SIZE_MAX, false), count,
                                        [&](size_t n) { return check_search(n, nullptr, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    if (!go) return r;
    return quality_list_host(c, as_items(count, ppIn, ppStreams, capacityEach, sizeX, sizeY), false, hasAlpha, pMaxErrorSums, hLo, hHi, poolThreads, fastBitCrushing, pResults);
  }
}

// ---- the lists of mixed shapes (contract: include/limg_hip.h; the layout and the route: limg_hip_list_plan.h; the walkers: encode_list, budget_list, sizes_list above) ----
extern "C"
{
  limg_hip_result limg_hip_encode_stream_list_device(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha, size_t *pBytes,
                                                     int poolThreads, int fastBitCrushing, void *stream)
  {
    std::vector<ListItem> items;
    bool go;
    const limg_hip_result r = open_list(check_items(c, true, count, pItems, itemSize, true, items), count, no_search, go);
    return !go ? r : encode_list(c, items, kListOwn, false, hasAlpha, pBytes, poolThreads, fastBitCrushing, stream);
  }

  limg_hip_result limg_hip_encode_stream_list(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha, size_t *pBytes,
                                              int poolThreads, int fastBitCrushing)
  {
    std::vector<ListItem> items;
    bool go;
    const limg_hip_result r = open_list(check_items(c, pBytes != nullptr, count, pItems, itemSize, false, items), count, no_search, go);
    if (!go) return r;
    std::vector<size_t> bytes(count);
    return host_list(c, items, bytes.data(), pBytes, [&](const std::vector<ListItem> &staged) {
      return encode_list(c, staged, kListOwn, false, hasAlpha, bytes.data(), poolThreads, fastBitCrushing, nullptr);
    });
  }

  limg_hip_result limg_hip_encode_stream_quality_list_device(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                                             const uint64_t *pMaxErrorSums, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads,
                                                             int fastBitCrushing, limg_hip_quality_result *pResults, void *stream)
  {
    std::vector<ListItem> items;
    uint32_t hLo, hHi;
    bool go;
    const limg_hip_result r = open_list(check_items(c, pMaxErrorSums && pResults, count, pItems, itemSize, true, items), count,
                                        [&](size_t n) { return check_search(n, nullptr, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    return !go ? r : quality_searches(c, count, items.data(), true, hasAlpha, pMaxErrorSums, hLo, hHi, poolThreads, fastBitCrushing, pResults, stream);
  }

  limg_hip_result limg_hip_encode_stream_quality_list(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                                      const uint64_t *pMaxErrorSums, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                      limg_hip_quality_result *pResults)
  {
    std::vector<ListItem> items;
    uint32_t hLo, hHi;
    bool go;
    const limg_hip_result r = open_list(check_items(c, pMaxErrorSums && pResults, count, pItems, itemSize, false, items), count,
                                        [&](size_t n) { return check_search(n, nullptr, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    return !go ? r : quality_list_host(c, items, true, hasAlpha, pMaxErrorSums, hLo, hHi, poolThreads, fastBitCrushing, pResults);
  }

  // ---- ... to a byte budget per item, and the sizes of every item at a list of error factors (budget_list / sizes_list above) ----
  limg_hip_result limg_hip_encode_stream_budget_list_device(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                                            const size_t *pMaxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                            limg_hip_budget_result *pResults, void *stream)
  {
    std::vector<ListItem> items;
    uint32_t hLo, hHi;
    bool go;
    const limg_hip_result r = open_list(check_items(c, pMaxBytes && pResults, count, pItems, itemSize, true, items), count,
                                        [&](size_t n) { return check_search(n, pMaxBytes, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    return !go ? r : budget_list(c, items, false, hasAlpha, pMaxBytes, minErrorFactor, maxErrorFactor, hLo, hHi, poolThreads, fastBitCrushing, pResults, stream);
  }

  limg_hip_result limg_hip_encode_stream_budget_list(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                                     const size_t *pMaxBytes, uint32_t minErrorFactor, uint32_t maxErrorFactor, int poolThreads, int fastBitCrushing,
                                                     limg_hip_budget_result *pResults)
  {
    std::vector<ListItem> items;
    uint32_t hLo, hHi;
    bool go;
    const limg_hip_result r = open_list(check_items(c, pMaxBytes && pResults, count, pItems, itemSize, false, items), count,
                                        [&](size_t n) { return check_search(n, pMaxBytes, minErrorFactor, maxErrorFactor, pResults, hLo, hHi); }, go);
    if (!go) return r;
    std::vector<limg_hip_budget_result> results = own_results<limg_hip_budget_result>(count);
    return host_list(c, items, results.data(), pResults, [&](const std::vector<ListItem> &staged) {
      return budget_list(c, staged, false, hasAlpha, pMaxBytes, minErrorFactor, maxErrorFactor, hLo, hHi, poolThreads, fastBitCrushing, results.data(), nullptr);
    });
  }

  // (an empty factor list, like an empty list: success with nothing done)
  limg_hip_result limg_hip_stream_sizes_list_device(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                                    const uint32_t *pErrorFactors, size_t factorCount, size_t *pBytes, int poolThreads, int fastBitCrushing, void *stream)
  {
    std::vector<ListItem> items;
    bool go;
    const limg_hip_result r = open_list(check_items(c, pErrorFactors && pBytes, count, pItems, itemSize, true, items, false), factorCount ? count : 0, no_search, go);
    if (!go) return r;
    if (factorCount > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    return sizes_list(c, items, hasAlpha, pErrorFactors, factorCount, pBytes, poolThreads, fastBitCrushing, stream);
  }

  limg_hip_result limg_hip_stream_sizes_list(limg_hip_context *c, size_t count, const limg_hip_stream_list_item *pItems, size_t itemSize, int hasAlpha,
                                             const uint32_t *pErrorFactors, size_t factorCount, size_t *pBytes, int poolThreads, int fastBitCrushing)
  {
    std::vector<ListItem> items, staged;
    bool go;
    limg_hip_result r = open_list(check_items(c, pErrorFactors && pBytes, count, pItems, itemSize, false, items, false), factorCount ? count : 0, no_search, go);
    if (!go) return r;
    if (factorCount > 0x7FFFFFFFull) return limg_hip_error_InvalidParameter;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    if ((r = stage_inputs(c, items, staged)) != limg_hip_success) return r;
    r = sizes_list(c, staged, hasAlpha, pErrorFactors, factorCount, pBytes, poolThreads, fastBitCrushing, nullptr);
    return r != limg_hip_success ? r : limg_hip_check_device_status(c);
  }
}
