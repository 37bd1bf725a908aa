// list_plan_check.cpp -- limg_amd/csrc/limg_hip_list_plan.h built by the host compiler alone; answers tests/test_list_plan_cpu.py's questions, one line each.
//   L <pool> <n> { <w> <h> <inAlign> <facAlign> } x n   the chunk made of these images, in order (the pointers: 0x10000 + the given offsets, the three factor
//                                                       planes alike) -> per image "firstBlock firstStrip strips firstUnit blocksX blocksY stripsX nBlocks
//                                                       chainCount chainRows vec", then "| blocks strips units noiseCalls vecInAll"
//   E <w> <h> <fast> <split> <legacy>                   eligibility -> 0 / 1
//   C <hook> <n> { <blocks> <strips> } x n              chunk boundaries with synthetic counts (no memory) -> the end of every chunk
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
    else puts("?");
  }
  return 0;
}
