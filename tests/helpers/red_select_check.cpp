// red_select_check.cpp -- host-only check of red_select_dead (limg_amd/csrc/limg_hip_encode_rules.h), built and run by tests/test_red_select_cpu.py.
// The packed trial's two weightings of a pixel's squared differences, restated here: (2, 4, 3) while dR^2 < 0x4000, else (3, 4, 2) -- "with" the select -- and
// (2, 4, 3) always -- "without".  One question per line on stdin, one answer line each:
//   w T   over all 256^3 (|dR|, |dG|, |dB|): "<pixels whose verdict (err > T) differs> <passing pixels whose values differ> <pixels with dR^2 >= 0x4000>"
//   d EF  "<red_select_dead(thresholds(EF).maxPixel32)> <maxPixel32>"
#include <cstdint>
#include <cstdio>

#include "../../limg_amd/csrc/limg_hip_encode_rules.h"

static uint32_t with_select(uint32_t r2, uint32_t g2, uint32_t b2) { return r2 < 0x4000u ? 2 * r2 + 4 * g2 + 3 * b2 : 3 * r2 + 4 * g2 + 2 * b2; }
static uint32_t without_select(uint32_t r2, uint32_t g2, uint32_t b2) { return 2 * r2 + 4 * g2 + 3 * b2; }

int main()
{
  char op;
  unsigned long long v;
  while (std::scanf(" %c %llu", &op, &v) == 2)
  {
    if (op == 'w')
    {
      const uint32_t T = (uint32_t)v;
      unsigned long long verdicts = 0, values = 0, highRed = 0;
      for (uint32_t r = 0; r < 256; r++)
        for (uint32_t g = 0; g < 256; g++)
          for (uint32_t b = 0; b < 256; b++)
          {
            const uint32_t a = with_select(r * r, g * g, b * b), n = without_select(r * r, g * g, b * b);
            const bool failA = a > T, failN = n > T;
            verdicts += failA != failN;
            values += !failA && !failN && a != n;
            highRed += r * r >= 0x4000u;
          }
      std::printf("%llu %llu %llu\n", verdicts, values, highRed);
    }
    else if (op == 'd')
    {
      const limg_hip::Thresholds t = limg_hip::thresholds((uint32_t)v);
      std::printf("%d %u\n", limg_hip::red_select_dead(t.maxPixel32) ? 1 : 0, t.maxPixel32);
    }
    else return 2;
  }
  return 0;
}
