// quality_step_check.cpp -- limg_amd/csrc/limg_hip_quality_step.h built by a host compiler on its own: the quality search driven from an error curve.
// stdin: hLo hHi limit, then E(hLo) .. E(hHi).  stdout: "result within probes errorSum maxProbes: h h h ..." -- the values asked for, in order.
// tests/test_stream_error_cpu.py compares that with a Python restatement of the algorithm.
#include "../../limg_amd/csrc/limg_hip_quality_step.h"

#include <stdio.h>
#include <vector>

int main()
{
  unsigned long long hLo, hHi, limit;
  if (scanf("%llu %llu %llu", &hLo, &hHi, &limit) != 3 || hLo > hHi) return 2;
  std::vector<unsigned long long> error(hHi - hLo + 1);
  for (unsigned long long &v : error)
    if (scanf("%llu", &v) != 1) return 2;
  limg_hip::QualityState s = limg_hip::quality_begin((uint32_t)hLo, (uint32_t)hHi, limit);
  std::vector<uint32_t> asked;
  while (!limg_hip::quality_done(s))
  {
    const uint32_t h = limg_hip::quality_next(s);
    if (h < hLo || h > hHi || asked.size() > 80) return 3; // (a search that leaves its range or does not end)
    asked.push_back(h);
    limg_hip::quality_step(s, error[h - hLo]);
  }
  limg_hip::quality_step(s, 0); // a step behind the end changes nothing
  printf("%u %u %u %llu %u:", limg_hip::quality_next(s), limg_hip::quality_within(s), limg_hip::quality_probes(s), (unsigned long long)limg_hip::quality_error_sum(s),
         limg_hip::rate_max_probes((uint32_t)hLo, (uint32_t)hHi));
  for (uint32_t h : asked) printf(" %u", h);
  printf("\n");
  return 0;
}
