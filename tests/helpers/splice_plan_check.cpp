// splice_plan_check -- limg_amd/csrc/limg_hip_splice_plan.h asked from a program of its own: the header is host-only C++, so the host compiler builds it alone
// (tests/test_splice_plan_cpu.py, under the undefined-behaviour sanitizer).
// One question per line of standard input:   sizeX sizeY count  { srcSizeX srcSizeY srcBx srcBy dstBx dstBy blocksW blocksH } x count
// One answer line each:                      0                                                  the rules refuse the call
//                                            1 nRuns nItems { piece srcEntry dstEntry count itemBase } x nRuns
#include "../../limg_amd/csrc/limg_hip_splice_plan.h"

#include <stdio.h>

#include <sstream>
#include <string>

int main()
{
  char *line = nullptr;
  size_t cap = 0;
  while (getline(&line, &cap, stdin) > 0)
  {
    std::istringstream in(line);
    unsigned long long sizeX = 0, sizeY = 0, count = 0;
    if (!(in >> sizeX >> sizeY >> count)) { fprintf(stderr, "bad question: %s", line); return 2; }
    std::vector<limg_hip::SplicePiece> pieces((size_t)count);
    for (limg_hip::SplicePiece &p : pieces)
      if (!(in >> p.srcSizeX >> p.srcSizeY >> p.srcBx >> p.srcBy >> p.dstBx >> p.dstBy >> p.blocksW >> p.blocksH)) { fprintf(stderr, "bad piece: %s", line); return 2; }
    std::vector<limg_hip::SpliceRun> runs;
    if (!limg_hip::splice_plan(pieces.data(), pieces.size(), sizeX, sizeY, runs)) { puts("0"); continue; }
    std::vector<uint32_t> itemBase(runs.size() + 1);
    const uint32_t nItems = limg_hip::splice_items(runs, itemBase.data());
    std::string out = "1 " + std::to_string(runs.size()) + " " + std::to_string(nItems);
    for (size_t i = 0; i < runs.size(); i++)
      out += " " + std::to_string(runs[i].piece) + " " + std::to_string(runs[i].srcEntry) + " " + std::to_string(runs[i].dstEntry) + " " + std::to_string(runs[i].count) + " " +
             std::to_string(itemBase[i]);
    puts(out.c_str());
  }
  free(line);
  return 0;
}
