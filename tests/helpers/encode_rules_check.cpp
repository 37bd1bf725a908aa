// encode_rules_check.cpp -- limg_amd/csrc/limg_hip_encode_rules.h built by a host compiler on its own: the header's answers, one line per question.
// stdin, one question per line:  t errorFactor  ->  maxPixel32 maxBlock blockLimitFull crushBits
//                                f a b c        ->  the three kernel values of the forced shift triple
//                                c blocks strips hook  ->  images per launch pair
//                                r              ->  sizeof(limg_hip_block_record)
#include "../../limg_amd/csrc/limg_hip_encode_rules.h"

#include <stdio.h>

int main()
{
  char what;
  while (scanf(" %c", &what) == 1)
  {
    if (what == 't')
    {
      unsigned long long ef;
      if (scanf("%llu", &ef) != 1 || ef > 0xFFFFFFFFull) return 2;
      const limg_hip::Thresholds t = limg_hip::thresholds((uint32_t)ef);
      printf("%llu %llu %llu %llu\n", (unsigned long long)t.maxPixel32, (unsigned long long)t.maxBlock, (unsigned long long)t.blockLimitFull, (unsigned long long)t.crushBits);
    }
    else if (what == 'f')
    {
      int in[3];
      if (scanf("%d %d %d", &in[0], &in[1], &in[2]) != 3) return 2;
      const int32_t option[3] = { in[0], in[1], in[2] };
      int32_t forced[3];
      limg_hip::forced_shifts(option, forced);
      printf("%d %d %d\n", (int)forced[0], (int)forced[1], (int)forced[2]);
    }
    else if (what == 'c')
    {
      unsigned long long blocks, strips, hook;
      if (scanf("%llu %llu %llu", &blocks, &strips, &hook) != 3 || blocks == 0 || strips == 0) return 2;
      printf("%llu\n", (unsigned long long)limg_hip::list_chunk((size_t)blocks, (size_t)strips, (size_t)hook));
    }
    else if (what == 'r') printf("%llu\n", (unsigned long long)sizeof(limg_hip_block_record));
    else return 2;
  }
  return 0;
}
