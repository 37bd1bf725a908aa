// list_plan_check.cpp -- limg_amd/csrc/limg_hip_list_plan.h built by the host compiler alone; answers tests/test_list_plan_cpu.py's questions, one line each.
//   L <pool> <n> { <w> <h> <inAlign> <facAlign> } x n   the chunk made of these images, in order (the pointers: 0x10000 + the given offsets, the three factor
//                                                       planes alike) -> per image "firstBlock firstStrip strips firstUnit blocksX blocksY stripsX nBlocks
//                                                       chainCount chainRows vec", then "| blocks strips units noiseCalls vecInAll"
//   E <w> <h> <fast> <split> <legacy>                   eligibility -> 0 / 1
//   C <hook> <n> { <blocks> <strips> } x n              chunk boundaries with synthetic counts (no memory) -> the end of every chunk
//   T <n> <view> <image> <io> <rated> <stream> <firstStrip> <firstUnit>   the table block of a chunk of n images with these entry sizes -> the seven offsets, bytes
//   N <hook> <n> { <blocks> <strips> <facBytes> } x n   what the largest chunk of a mixed-shape encode of these (eligible, all of different shapes) needs: the
//                                                       plan's `most` -> "images blocks strips facBytes" (MISMATCH where list_needs, which the walkers took it from, differs)
//   P <w> <h>                                           one factor plane's slice -> bytes
//   R <job> <same> <fast> <split> <legacy> <hook> <n> { <w> <h> <errorFactor> } x n
//                                                       the route (list_route) of these items -- job: 0 shared factor, 1 own factors, 2 budget, 3 sizes; same: a
//                                                       same-shape entry -> the steps, "S i" a single, "C<own> i j .." a same-shape chunk, "M i j .." a mixed chunk,
//                                                       each separated by ";", for the encodes a "!" in front of a step that restarts the statistics; then
//                                                       "| images blocks strips facBytes | inPlace"
//   O ...                                               the same question answered by the decisions of the five walkers as they stood before list_route, lifted
//                                                       literally into old_route below: the same line
//   K <hook> <n> <blocks> <strips>                      n images of one shape cut by list_chunk(blocks, strips, hook) images at a time -> the end of every chunk
#include "../../limg_amd/csrc/limg_hip_list_plan.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace limg_hip;

namespace
{
  struct Asked
  {
    int job = 0, same = 0, fast = 0;
    limg_hip_options o;
    size_t hook = 0;
    std::vector<ListPlanItem> items;
    bool encode() const { return job == kListShared || job == kListOwn; }
  };

  struct Line
  {
    std::ostringstream out;
    bool encode;
    void step(char kind, bool own, bool restart, const size_t *idx, size_t n)
    {
      if (restart && encode) out << '!';
      out << kind;
      if (kind == 'C') out << (own ? 1 : 0);
      for (size_t i = 0; i < n; i++) out << ' ' << idx[i];
      out << ';';
    }
    std::string end(const ListNeeds &m, bool inPlace)
    {
      out << " | " << m.images << ' ' << m.blocks << ' ' << m.strips << ' ' << m.facBytes << " | " << (inPlace ? 1 : 0);
      return out.str();
    }
  };

  // ---- the walkers' decisions as they stood: stream_list_device (with encode_grouped), limg_hip_encode_stream_budget_batch_device, stream_items_device, struct
  // ListRoute with budget_items_device and sizes_items_device -- conditions, loops and their order lifted; a launch became a printed step, an `ensure` a maximum ----
  struct OldRoute
  {
    const Asked &q;
    Line line;
    ListNeeds most = {};
    bool inPlace = false;
    void grow(size_t images, uint64_t blocks, uint64_t strips, size_t fac)
    {
      if (images > most.images) most.images = images;
      if (blocks > most.blocks) most.blocks = blocks;
      if (strips > most.strips) most.strips = strips;
      if (fac > most.facBytes) most.facBytes = fac;
    }
    void stream_list_device(const std::vector<size_t> &in, bool efs, bool entry)
    {
      const ListPlanItem &a = q.items[in[0]];
      const size_t count = in.size();
      const EncodeShape sh(a.sizeX, a.sizeY);
      const size_t chunk = list_chunk((size_t)a.blocks, (size_t)a.strips, q.hook);
      const bool batch_applies = list_in_one_pair(sh, q.o);
      const bool grouped = efs && (count == 1 || !batch_applies || q.fast == 0);
      const bool oneByOne = grouped || count == 1 || !batch_applies;
      const size_t mostImages = oneByOne ? 1 : (count < chunk ? count : chunk);
      if (mostImages > 1) grow(mostImages, mostImages * a.blocks, mostImages * a.strips, mostImages * (((a.sizeX * a.sizeY + 255) & ~(size_t)255) * 3));
      if (grouped)
      { // encode_grouped
        std::vector<size_t> order(in);
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return q.items[x].errorFactor < q.items[y].errorFactor; });
        for (size_t g0 = 0; g0 < count;)
        {
          const uint32_t ef = q.items[order[g0]].errorFactor;
          size_t g1 = g0;
          std::vector<size_t> group;
          for (; g1 < count && q.items[order[g1]].errorFactor == ef; g1++) group.push_back(order[g1]);
          if (g1 - g0 == 1) line.step('S', false, true, &group[0], 1); // (stats.accumulate is false here)
          else stream_list_device(group, false, false);
          g0 = g1;
        }
      }
      for (size_t i0 = 0; !grouped && i0 < count;)
      {
        const size_t n = oneByOne ? 1 : (count - i0 < chunk ? count - i0 : chunk);
        const bool accumulate = i0 != 0;
        if (n == 1) line.step('S', false, !accumulate, &in[i0], 1);
        else line.step('C', efs, !accumulate, &in[i0], n);
        i0 += n;
      }
      if (entry) inPlace = !oneByOne; // list_bytes(c, oneByOne ? images.data() : nullptr, ...)
    }
    void budget_batch_device(const std::vector<size_t> &in)
    {
      const ListPlanItem &a = q.items[in[0]];
      const size_t count = in.size();
      const EncodeShape sh(a.sizeX, a.sizeY);
      const bool rate_probe_applies = list_in_one_pair(sh, q.o) && q.fast != 0;
      const size_t chunk = count == 1 || !rate_probe_applies ? 1 : list_chunk((size_t)a.blocks, (size_t)a.strips, q.hook);
      for (size_t i0 = 0; i0 < count;)
      {
        const size_t n = count - i0 < chunk ? count - i0 : chunk;
        if (n == 1) { line.step('S', false, false, &in[i0++], 1); continue; }
        line.step('C', false, false, &in[i0], n);
        grow(n, n * a.blocks, n * a.strips, 0); // (probe_setup and the chunk's own encode grow as they go)
        i0 += n;
      }
    }
    void items(size_t count)
    {
      std::vector<size_t> shared, alone;
      for (size_t i = 0; i < count; i++) (list_item_eligible(q.items[i].sizeX, q.items[i].sizeY, q.fast, q.o) ? shared : alone).push_back(i);
      bool oneShape = true;
      for (size_t i : shared) oneShape = oneShape && q.items[i].sizeX == q.items[shared[0]].sizeX && q.items[i].sizeY == q.items[shared[0]].sizeY;
      std::vector<uint64_t> blocks, strips;
      std::vector<size_t> fac;
      for (size_t i : shared) { blocks.push_back(q.items[i].blocks); strips.push_back(q.items[i].strips); fac.push_back(q.encode() ? q.items[i].facBytes : 0); }
      bool first = true;
      auto single = [&](size_t i) { line.step('S', false, first, &i, 1); first = false; };
      auto chunks = [&]() {
        const ListNeeds m = list_needs(blocks.data(), strips.data(), fac.data(), shared.size(), q.hook);
        grow(m.images, m.blocks, m.strips, m.facBytes);
        for (size_t i0 = 0; i0 < shared.size();)
        {
          const size_t i1 = list_chunk_end(blocks.data(), strips.data(), shared.size(), i0, q.hook);
          if (i1 - i0 == 1) single(shared[i0]);
          else { line.step('M', true, first, &shared[i0], i1 - i0); first = false; }
          i0 = i1;
        }
      };
      if (q.job == kListSizes) chunks(); // sizes_items_device: no one-shape case
      else if (shared.size() == 1) single(shared[0]);
      else if (!shared.empty() && oneShape)
      {
        if (q.job == kListBudget) budget_batch_device(shared);
        else stream_list_device(shared, true, false);
        first = false;
      }
      else if (!shared.empty()) chunks();
      for (size_t i : alone) single(i);
    }
    std::string answer()
    {
      line.encode = q.encode();
      const size_t count = q.items.size();
      std::vector<size_t> all(count);
      for (size_t i = 0; i < count; i++) all[i] = i;
      if (!q.same) items(count);
      else if (q.job == kListBudget) budget_batch_device(all);
      else stream_list_device(all, q.job == kListOwn, true);
      return line.end(most, inPlace);
    }
  };

  std::string new_route(const Asked &q)
  {
    const ListPlan plan = list_route(q.items.data(), q.items.size(), (ListJob)q.job, q.same != 0, q.fast, q.o, q.hook);
    Line line;
    line.encode = q.encode();
    size_t at = 0;
    for (const ListStep &st : plan.steps)
    {
      if (st.first != at || st.count == 0 || (st.kind == kStepSingle) != (st.count == 1)) return "BROKEN";
      line.step(st.kind == kStepSingle ? 'S' : st.kind == kStepSame ? 'C' : 'M', st.own, st.restart, &plan.order[st.first], st.count);
      at += st.count;
    }
    if (at != plan.order.size() || at != q.items.size()) return "BROKEN";
    bool mixed = false, rated = false;
    for (const ListStep &st : plan.steps) { mixed = mixed || st.kind == kStepMixed; rated = rated || (st.kind == kStepSame && st.own); }
    if (mixed != plan.mixed || rated != plan.rated) return "BROKEN";
    return line.end(plan.most, plan.inPlace);
  }
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line))
  {
    std::istringstream in(line);
    char q = 0;
    in >> q;
    if (q == 'L')
    {
      int pool = 0;
      size_t n = 0;
      in >> pool >> n;
      ListChunkTotals t = {};
      std::ostringstream out;
      for (size_t i = 0; i < n; i++)
      {
        unsigned long long w = 0, h = 0, ia = 0, fa = 0;
        in >> w >> h >> ia >> fa;
        uint8_t *fac[3] = { (uint8_t *)(uintptr_t)(0x10000 + fa), (uint8_t *)(uintptr_t)(0x10000 + fa), (uint8_t *)(uintptr_t)(0x10000 + fa) };
        const ListImage e = list_image(t, (size_t)w, (size_t)h, pool, (const uint32_t *)(uintptr_t)(0x10000 + ia), fac);
        out << e.firstBlock << ' ' << e.firstStrip << ' ' << e.strips << ' ' << e.firstUnit << ' ' << e.blocksX << ' ' << e.blocksY << ' ' << e.stripsX << ' ' << e.nBlocks << ' '
            << e.chainCount << ' ' << e.chainRows << ' ' << e.vec << ' ';
        if (e.sizeX != w || e.sizeY != h) out << "SIZE ";
      }
      out << "| " << t.blocks << ' ' << t.strips << ' ' << t.units << ' ' << t.noiseCalls << ' ' << (t.vecInAll ? 1 : 0);
      puts(out.str().c_str());
    }
    else if (q == 'E')
    {
      unsigned long long w = 0, h = 0;
      int fast = 0, split = 0, legacy = 0;
      in >> w >> h >> fast >> split >> legacy;
      limg_hip_options o;
      memset(&o, 0, sizeof(o));
      o.force_split_kernels = split; o.legacy_float_stage = legacy;
      printf("%d\n", list_item_eligible((size_t)w, (size_t)h, fast, o) ? 1 : 0);
    }
    else if (q == 'C')
    {
      size_t hook = 0, n = 0;
      in >> hook >> n;
      std::vector<uint64_t> blocks(n), strips(n);
      for (size_t i = 0; i < n; i++) in >> blocks[i] >> strips[i];
      std::ostringstream out;
      for (size_t i0 = 0; i0 < n;)
      {
        const size_t i1 = list_chunk_end(blocks.data(), strips.data(), n, i0, hook);
        if (i1 <= i0) { out << "STUCK"; break; }
        out << i1 << ' ';
        i0 = i1;
      }
      puts(out.str().c_str());
    }
    else if (q == 'T')
    {
      size_t n = 0;
      ChunkEntrySizes e = {};
      in >> n >> e.view >> e.image >> e.io >> e.rated >> e.stream >> e.firstStrip >> e.firstUnit;
      const ChunkTables t(n, e);
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", t.views, t.images, t.io, t.rated, t.streams, t.firstStrip, t.firstUnit, t.bytes);
    }
    else if (q == 'N')
    {
      size_t hook = 0, n = 0;
      in >> hook >> n;
      std::vector<uint64_t> blocks(n), strips(n);
      std::vector<size_t> fac(n);
      for (size_t i = 0; i < n; i++) in >> blocks[i] >> strips[i] >> fac[i];
      std::vector<ListPlanItem> items(n);
      for (size_t i = 0; i < n; i++) items[i] = { 8 * (i + 1), 8, blocks[i], strips[i], fac[i], true, 100u };
      limg_hip_options o;
      memset(&o, 0, sizeof(o));
      const ListNeeds m = list_route(items.data(), n, kListOwn, false, 1, o, hook).most, was = list_needs(blocks.data(), strips.data(), fac.data(), n, hook);
      if (n > 1 && (m.images != was.images || m.blocks != was.blocks || m.strips != was.strips || m.facBytes != was.facBytes)) puts("MISMATCH");
      else printf("%zu %llu %llu %zu\n", m.images, (unsigned long long)m.blocks, (unsigned long long)m.strips, m.facBytes);
    }
    else if (q == 'P')
    {
      unsigned long long w = 0, h = 0;
      in >> w >> h;
      printf("%zu\n", list_plane_stride((size_t)w, (size_t)h));
    }
    else if (q == 'R' || q == 'O')
    {
      Asked a;
      int split = 0, legacy = 0;
      size_t n = 0;
      in >> a.job >> a.same >> a.fast >> split >> legacy >> a.hook >> n;
      memset(&a.o, 0, sizeof(a.o));
      a.o.force_split_kernels = split; a.o.legacy_float_stage = legacy;
      for (size_t i = 0; i < n; i++)
      {
        unsigned long long w = 0, h = 0, ef = 0;
        in >> w >> h >> ef;
        a.items.push_back(list_plan_item((size_t)w, (size_t)h, (uint32_t)ef, a.fast, a.o));
      }
      OldRoute old = { a, {} };
      puts((q == 'R' ? new_route(a) : old.answer()).c_str());
    }
    else if (q == 'K')
    {
      size_t hook = 0, n = 0, blocks = 0, strips = 0;
      in >> hook >> n >> blocks >> strips;
      const size_t chunk = list_chunk(blocks, strips, hook);
      std::ostringstream out;
      for (size_t i0 = 0; i0 < n;)
      {
        i0 += n - i0 < chunk ? n - i0 : chunk;
        out << i0 << ' ';
      }
      puts(out.str().c_str());
    }
    else puts("?");
  }
  return 0;
}
