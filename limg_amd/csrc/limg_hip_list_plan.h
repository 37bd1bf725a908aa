// limg_hip_list_plan.h -- the layout of a stream-encode list whose images differ in shape (limg_hip_encode_stream_list*), stated ONCE for the host route and the
// kernels that walk it: which items may share the launches, where an image's blocks, strips and float-stage units start in the chunk's concatenated arrays, the
// 16-byte access flags and the dither-chain partition of THAT image, a chunk's totals and its noise need, and where a chunk ends -- and the ROUTE of every list
// entry of the stream encode family, same-shape or mixed (list_route: which items go through which launches, in which order, and what the largest chunk needs).  A
// host compiler builds it on its own (tests/helpers/list_plan_check.cpp).  Plain C++: no HIP types, nothing but the standard library.
#ifndef LIMG_HIP_LIST_PLAN_H
#define LIMG_HIP_LIST_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "limg_hip_encode_plan.h"
#include "limg_hip_encode_rules.h"

namespace limg_hip
{
  // ---- eligibility: what k_encode_list_rated asks of its list, per item -- whole blocks, the default search, the persistent path behind k_fit_tpb ----
  inline bool list_item_eligible(size_t sizeX, size_t sizeY, int fastBitCrushing, const limg_hip_options &o)
  {
    const EncodeShape sh(sizeX, sizeY);
    return sh.valid && list_in_one_pair(sh, o) && fastBitCrushing != 0;
  }

  constexpr uint32_t kListUnitBlocks = 64; // a float-stage unit: up to 64 adjacent blocks of one block row of ONE image (a wave of k_fit_tpb_list)

  // ---- one image of a chunk: its own geometry and where its slices start ----
  // The device table entry (64 bytes, next to the ImageIO / RatedImage / StreamImage entries of the same index): read with scalar loads, once per work item.
  struct ListImage
  {
    uint64_t firstBlock;  // of its slice of the records, invN (x 4 floats) and shift words
    uint32_t firstStrip;  // its first work strip id: look-back descriptors and payload words are indexed by firstStrip + local strip
    uint32_t strips;      // stripsX * blocksY
    uint32_t firstUnit;   // its first float-stage unit; it has ceil(blocksX / 64) * blocksY of them
    uint32_t sizeX, sizeY, blocksX, blocksY, stripsX;
    uint32_t nBlocks;     // blocksX * blocksY (a stream's table has 32-bit indices: limg_hip_stream_bound)
    uint32_t chainCount, chainRows; // partition(sizeY, poolThreads): every image starts its own chains
    uint32_t vec;         // kListVec*: the 16-byte access flags of THIS image (not the & over the list: widths differ)
    uint32_t pad[2];
  };
  static_assert(sizeof(ListImage) == 64, "one entry of the list table");
  enum { kListVecIn = 1u, kListVecPlanes = 2u, kListVecFactors8 = 4u, kListVecDecoded = 8u, kListVecFactors = 16u };

  inline uint32_t list_vec_bits(const VecAccess &v)
  {
    return (v.in ? kListVecIn : 0u) | (v.planes ? kListVecPlanes : 0u) | (v.factors8 ? kListVecFactors8 : 0u) | (v.decoded ? kListVecDecoded : 0u) | (v.factors ? kListVecFactors : 0u);
  }
  inline uint32_t list_units(const EncodeShape &sh) { return (uint32_t)(((sh.blocksX + kListUnitBlocks - 1) / kListUnitBlocks) * sh.blocksY); }
  // dither calls the longest chain of an image can make: every block at most 3; the last chain takes the remainder, never fewer rows than the others
  inline uint64_t list_chain_calls(const EncodeShape &sh, const Partition &pt)
  {
    uint64_t maxRows = sh.blocksY;
    if (pt.chainCount > 1 && (uint64_t)(pt.chainCount - 1) * pt.chainRows < sh.blocksY) maxRows = sh.blocksY - (uint64_t)(pt.chainCount - 1) * pt.chainRows;
    return maxRows * sh.blocksX * 3;
  }

  // ---- a chunk: the images [i0, i0 + n) of the eligible list, concatenated ----
  struct ListChunkTotals
  {
    uint64_t blocks;     // records / invN / shift words of the chunk
    uint32_t strips;     // work strips (32-bit ids)
    uint32_t units;      // float-stage units
    uint64_t noiseCalls; // the noise table's need: the LARGEST per-chain call count of any image (every image starts its own chains at the seed), not their sum
    bool vecInAll;       // every image's rows may be read 16 bytes per lane: the float stage's DIRECT instances
  };

  // Where the chunk that starts at image i0 ends: the plane batch's rule (1 GiB of block records, 32-bit strip ids, the test build's batch_chunk = images per
  // chunk) counted in blocks and strips SUMMED over the images; at least one image.  blocks[i], strips[i]: of image i, both > 0.  On images of ONE shape its chunks
  // are those of list_chunk (limg_hip_encode_rules.h), `list_chunk(blocks, strips, hook)` images each: tests/test_list_plan_cpu.py.
  inline size_t list_chunk_end(const uint64_t *blocks, const uint64_t *strips, size_t count, size_t i0, size_t hook)
  {
    const uint64_t maxBlocks = (1ull << 30) / sizeof(limg_hip_block_record), maxStrips = 0x7FFFFFFFull;
    uint64_t b = 0, s = 0;
    size_t i = i0;
    for (; i < count; i++)
    {
      if (hook > 0 && i - i0 >= hook) break;
      if (i > i0 && (b + blocks[i] > maxBlocks || s + strips[i] > maxStrips)) break;
      b += blocks[i]; s += strips[i];
    }
    return i > i0 ? i : (i0 < count ? i0 + 1 : i0);
  }

  // entry i of a chunk, given the totals of the images in front of it (which it then advances).  in / facs: the image's input and its three factor planes.
  inline ListImage list_image(ListChunkTotals &t, size_t sizeX, size_t sizeY, int poolThreads, const uint32_t *in, uint8_t *const fac[3])
  {
    const EncodeShape sh(sizeX, sizeY);
    const Partition pt = partition(sizeY, poolThreads);
    limg_hip_encode3d_info info = {};
    info.pFactorsA = fac[0]; info.pFactorsB = fac[1]; info.pFactorsC = fac[2];
    const VecAccess v = vec_access(in, &info, sizeX, false);
    ListImage e = {};
    e.firstBlock = t.blocks; e.firstStrip = t.strips; e.firstUnit = t.units;
    e.strips = (uint32_t)sh.strips;
    e.sizeX = (uint32_t)sizeX; e.sizeY = (uint32_t)sizeY; e.blocksX = (uint32_t)sh.blocksX; e.blocksY = (uint32_t)sh.blocksY; e.stripsX = (uint32_t)sh.stripsX;
    e.nBlocks = (uint32_t)sh.blocks;
    e.chainCount = pt.chainCount; e.chainRows = pt.chainRows;
    e.vec = list_vec_bits(v);
    const uint64_t calls = list_chain_calls(sh, pt);
    if (t.blocks == 0 && t.strips == 0) t.vecInAll = true;
    t.vecInAll = t.vecInAll && v.in;
    if (calls > t.noiseCalls) t.noiseCalls = calls;
    t.blocks += sh.blocks; t.strips += (uint32_t)sh.strips; t.units += list_units(sh);
    return e;
  }

  // one of an image's three factor planes in the chunk's scratch: 256-byte aligned slices
  inline size_t list_plane_stride(size_t sizeX, size_t sizeY) { return (sizeX * sizeY + 255) & ~(size_t)255; }

  // ---- the tables of one chunk of n images, side by side in one device block: where each part starts (16-byte aligned), given the bytes of one entry of each part:
  // the image's view (RatedListParams), its ListImage, ImageIO, RatedImage, StreamImage and its two prefix words ----
  struct ChunkEntrySizes { size_t view, image, io, rated, stream, firstStrip, firstUnit; };
  struct ChunkTables
  {
    size_t views, images, io, rated, streams, firstStrip, firstUnit, bytes;
    ChunkTables(size_t n, const ChunkEntrySizes &e)
    {
      auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
      views = 0; images = up(views + n * e.view); io = up(images + n * e.image); rated = up(io + n * e.io);
      streams = up(rated + n * e.rated); firstStrip = up(streams + n * e.stream); firstUnit = up(firstStrip + n * e.firstStrip); bytes = up(firstUnit + n * e.firstUnit);
    }
  };

  // ---- what the largest chunk of a list asks of the scratch: over the steps of more than one image (one image alone takes the single call), each member the
  // maximum over them -- everything is grown once, before the first launch.  facBytes: the images' three factor planes each ----
  struct ListNeeds { size_t images; uint64_t blocks, strips; size_t facBytes; };
  inline void list_needs_max(ListNeeds &most, const ListNeeds &n)
  {
    if (n.images > most.images) most.images = n.images;
    if (n.blocks > most.blocks) most.blocks = n.blocks;
    if (n.strips > most.strips) most.strips = n.strips;
    if (n.facBytes > most.facBytes) most.facBytes = n.facBytes;
  }
  // ... of the chunks list_chunk_end cuts a list of eligible items into (what list_route's `most` is for a mixed-shape encode).  facBytes[i]: image i's planes
  inline ListNeeds list_needs(const uint64_t *blocks, const uint64_t *strips, const size_t *facBytes, size_t count, size_t hook)
  {
    ListNeeds most = {};
    for (size_t i0 = 0; i0 < count;)
    {
      const size_t i1 = list_chunk_end(blocks, strips, count, i0, hook);
      ListNeeds n = { i1 - i0, 0, 0, 0 };
      for (size_t i = i0; i < i1; i++) { n.blocks += blocks[i]; n.strips += strips[i]; n.facBytes += facBytes[i]; }
      if (n.images > 1) list_needs_max(most, n);
      i0 = i1;
    }
    return most;
  }

  // ---- the route of a list: which launches its items take, in which order.  ONE pure function for every list entry of the stream encode family; the entries'
  // walkers (limg_hip_stream_encode_api.hip) grow what `most` says and loop over the steps, and decide nothing ----
  enum ListJob { kListShared, kListOwn, kListBudget, kListSizes }; // encode at one factor / at each item's own; search each item's factor for a budget; the sizes at a list of factors
  enum ListStepKind
  {
    kStepSingle, // one item through the single call of the job
    kStepSame,   // n > 1 items of one shape in one launch pair (budget: behind one shared probe grid and the searches on it)
    kStepMixed   // n > 1 eligible items, whatever their shapes, in the mixed launches (encode_list_chunk; budget and sizes: the list probe on its fit grid)
  };
  // blocks and strips are inputs of their own (not derived from the shape here), as list_chunk_end takes them: synthetic counts can be asked about without memory
  struct ListPlanItem { size_t sizeX, sizeY; uint64_t blocks, strips; size_t facBytes; bool eligible; uint32_t errorFactor; }; // facBytes: its three factor planes
  inline ListPlanItem list_plan_item(size_t sizeX, size_t sizeY, uint32_t errorFactor, int fastBitCrushing, const limg_hip_options &o)
  {
    const EncodeShape sh(sizeX, sizeY);
    return { sizeX, sizeY, sh.blocks, sh.strips, 3 * list_plane_stride(sizeX, sizeY), list_item_eligible(sizeX, sizeY, fastBitCrushing, o), errorFactor };
  }
  struct ListStep
  {
    ListStepKind kind;
    bool own;     // kStepSame of an encode: each image at its own factor (k_encode_list_rated); false: the chunk shares one
    bool restart; // limg_hip_last_stats starts over with this step (the first; on the sorted route the first of every factor's group); the others add to it
    size_t first, count; // its items: order[first, first + count)
  };
  struct ListPlan
  {
    std::vector<size_t> order; // item indices, step after step: every item once
    std::vector<ListStep> steps;
    ListNeeds most = {};   // of the steps of more than one item, member by member; facBytes: the encodes only (a probe writes no factor plane)
    bool mixed = false;    // there are kStepMixed steps (then there is no kStepSame)
    bool rated = false;    // there are own-factor chunks: a threshold table of most.images entries
    bool inPlace = false;  // a same-shape encode cut in list order: step after step leaves its items' entries of the streams' table, entry i = item i
  };

  // The rules, each once.  same_shape / budget_same take items of ONE shape (by index); list_route below names which entry takes which.
  struct ListRouter
  {
    const ListPlanItem *items; ListJob job; int fast; const limg_hip_options &opt; size_t hook;
    ListPlan plan;
    bool restart = true;

    void step(ListStepKind kind, bool own, const size_t *idx, size_t n)
    {
      plan.steps.push_back({ kind, n > 1 && own, restart, plan.order.size(), n });
      plan.order.insert(plan.order.end(), idx, idx + n);
      restart = false;
      if (n < 2) return;
      ListNeeds need = { n, 0, 0, 0 };
      for (size_t i = 0; i < n; i++)
      {
        const ListPlanItem &it = items[idx[i]];
        need.blocks += it.blocks; need.strips += it.strips;
        if (job == kListShared || job == kListOwn) need.facBytes += it.facBytes;
      }
      list_needs_max(plan.most, need);
      plan.mixed = plan.mixed || kind == kStepMixed;
      plan.rated = plan.rated || (kind == kStepSame && own);
    }
    bool pair(const std::vector<size_t> &idx) const { return list_in_one_pair(EncodeShape(items[idx[0]].sizeX, items[idx[0]].sizeY), opt); }
    // `chunk` images per step, in the order of idx; a (last) chunk of one is a single
    void chunks_of(const std::vector<size_t> &idx, size_t chunk, bool own)
    {
      for (size_t i0 = 0, n; i0 < idx.size(); i0 += n)
      {
        n = idx.size() - i0 < chunk ? idx.size() - i0 : chunk;
        step(n == 1 ? kStepSingle : kStepSame, own, &idx[i0], n);
      }
    }
    // An encode of images of one shape, at a shared factor or (own) each at its own.  Own factors outside k_encode_list_rated's reach -- a list of one, no launch
    // pair (partial edge blocks, the split path, the float stage inside the encode kernel), the accurate search --: sorted by factor (stable), every distinct value
    // as a shared-factor list of its own.  Else singles in list order where there is no launch pair (or one image), else chunks of list_chunk -- a shared-factor list
    // takes them under the accurate search too.  -> the list was cut in list order by the chunk rule (ListPlan::inPlace)
    bool same_shape(std::vector<size_t> idx, bool own)
    {
      const size_t n = idx.size();
      const bool pairs = n > 1 && pair(idx);
      if (own && (!pairs || fast == 0))
      {
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return items[a].errorFactor < items[b].errorFactor; });
        for (size_t g0 = 0, g1; g0 < n; g0 = g1)
        {
          for (g1 = g0; g1 < n && items[idx[g1]].errorFactor == items[idx[g0]].errorFactor;) g1++;
          restart = true;
          same_shape(std::vector<size_t>(idx.begin() + g0, idx.begin() + g1), false);
        }
        return false;
      }
      chunks_of(idx, pairs ? list_chunk((size_t)items[idx[0]].blocks, (size_t)items[idx[0]].strips, hook) : 1, own);
      return pairs;
    }
    // The budget searches of images of one shape: chunks of list_chunk behind one shared probe grid each where the probe applies and there is something to share, else
    // the single budget call each.  A chunk's final encode is same_shape on that chunk, at a shared factor where all its searches chose one value, else at own factors.
    void budget_same(const std::vector<size_t> &idx)
    {
      const bool probes = idx.size() > 1 && pair(idx) && fast != 0;
      chunks_of(idx, probes ? list_chunk((size_t)items[idx[0]].blocks, (size_t)items[idx[0]].strips, hook) : 1, false);
    }
    // An items entry.  The eligible items first, in list order: one alone is a single; of one shape (not the sizes: their probe takes any shapes as they come) the
    // same-shape rule of the job; else chunks of list_chunk_end, a chunk of one being a single.  Then the others as singles, in list order.  The final encode of a
    // budget's mixed chunk is this route (kListOwn) of that chunk.
    void items_form(size_t count)
    {
      std::vector<size_t> shared, alone;
      for (size_t i = 0; i < count; i++) (items[i].eligible ? shared : alone).push_back(i);
      bool oneShape = job != kListSizes;
      for (size_t i : shared) oneShape = oneShape && items[i].sizeX == items[shared[0]].sizeX && items[i].sizeY == items[shared[0]].sizeY;
      if (shared.size() == 1) step(kStepSingle, false, &shared[0], 1);
      else if (!shared.empty() && oneShape)
      {
        if (job == kListBudget) budget_same(shared);
        else same_shape(shared, true);
      }
      else
      {
        std::vector<uint64_t> blocks, strips;
        for (size_t i : shared) { blocks.push_back(items[i].blocks); strips.push_back(items[i].strips); }
        for (size_t i0 = 0, i1; i0 < shared.size(); i0 = i1)
        {
          i1 = list_chunk_end(blocks.data(), strips.data(), shared.size(), i0, hook);
          step(i1 - i0 == 1 ? kStepSingle : kStepMixed, true, &shared[i0], i1 - i0);
        }
      }
      for (size_t i : alone) step(kStepSingle, false, &i, 1);
    }
  };

  // sameShape: a same-shape entry (limg_hip_encode_stream_batch*, _budget_batch: one shape for the whole list; there is no such entry for the sizes), else an items
  // entry (limg_hip_encode_stream_list, _budget_list, limg_hip_stream_sizes_list; their items carry own factors: not kListShared).  opt: what list_in_one_pair reads.
  // hook: the test build's batch_chunk, 0 = none.
  inline ListPlan list_route(const ListPlanItem *items, size_t count, ListJob job, bool sameShape, int fastBitCrushing, const limg_hip_options &opt, size_t hook)
  {
    ListRouter r = { items, job, fastBitCrushing, opt, hook };
    if (count == 0) return r.plan;
    if (!sameShape) r.items_form(count);
    else
    {
      std::vector<size_t> all(count);
      for (size_t i = 0; i < count; i++) all[i] = i;
      if (job == kListBudget) r.budget_same(all);
      else r.plan.inPlace = r.same_shape(all, job == kListOwn);
    }
    return r.plan;
  }
}

#endif
