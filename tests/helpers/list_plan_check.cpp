// list_plan_check.cpp -- limg_amd/csrc/limg_hip_list_plan.h built by the host compiler alone; answers tests/test_list_plan_cpu.py's questions, one line each.
//   L <pool> <n> { <w> <h> <inAlign> <facAlign> } x n   the chunk made of these images, in order (the pointers: 0x10000 + the given offsets, the three factor
//                                                       planes alike) -> per image "firstBlock firstStrip strips firstUnit blocksX blocksY stripsX nBlocks
//                                                       chainCount chainRows vec", then "| blocks strips units noiseCalls vecInAll"
//   E <w> <h> <fast> <split> <legacy>                   eligibility -> 0 / 1
//   C <hook> <n> { <blocks> <strips> } x n              chunk boundaries with synthetic counts (no memory) -> the end of every chunk
//   T <n> <view> <image> <io> <rated> <stream> <firstStrip> <firstUnit>   the table block of a chunk of n images with these entry sizes -> the seven offsets, bytes
//   N <hook> <n> { <blocks> <strips> <facBytes> } x n   what the largest chunk needs -> "images blocks strips facBytes"
//   P <w> <h>                                           one factor plane's slice -> bytes
#include "../../limg_amd/csrc/limg_hip_list_plan.h"

#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace limg_hip;

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
      const ListNeeds m = list_needs(blocks.data(), strips.data(), fac.data(), n, hook);
      printf("%zu %llu %llu %zu\n", m.images, (unsigned long long)m.blocks, (unsigned long long)m.strips, m.facBytes);
    }
    else if (q == 'P')
    {
      unsigned long long w = 0, h = 0;
      in >> w >> h;
      printf("%zu\n", list_plane_stride((size_t)w, (size_t)h));
    }
    else puts("?");
  }
  return 0;
}
