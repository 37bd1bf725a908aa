// rate_step_check.cpp -- limg_amd/csrc/limg_hip_rate_step.h built by a host compiler on its own: the budget search driven from a size curve.
// stdin: hLo hHi budget, then size(hLo) .. size(hHi).  stdout: "result within probes bytes maxProbes: h h h ..." -- the values asked for, in order.
// tests/test_rate_step_cpu.py compares that with a Python restatement of the algorithm.
#include "../../limg_amd/csrc/limg_hip_rate_step.h"

#include <stdio.h>
#include <vector>

int main()
{
  unsigned long long hLo, hHi, budget;
  if (scanf("%llu %llu %llu", &hLo, &hHi, &budget) != 3 || hLo > hHi) return 2;
  std::vector<unsigned long long> size(hHi - hLo + 1);
  for (unsigned long long &v : size)
    if (scanf("%llu", &v) != 1) return 2;
  limg_hip::RateState s = limg_hip::rate_begin((uint32_t)hLo, (uint32_t)hHi, budget);
  std::vector<uint32_t> asked;
  while (!s.done)
  {
    if (s.next < hLo || s.next > hHi || asked.size() > 80) return 3; // (a search that leaves its range or does not end)
    asked.push_back(s.next);
    limg_hip::rate_step(s, size[s.next - hLo]);
  }
  limg_hip::rate_step(s, 0); // a step behind the end changes nothing
  printf("%u %u %u %llu %u:", s.next, s.within, s.probes, (unsigned long long)s.bestBytes, limg_hip::rate_max_probes((uint32_t)hLo, (uint32_t)hHi));
  for (uint32_t h : asked) printf(" %u", h);
  printf("\n");
  return 0;
}
