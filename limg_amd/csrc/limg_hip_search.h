// limg_hip_search.h -- the E step's shift search (a9-a12): the packed 16-bit trial, the fast and the accurate search automata, and the generic-path search.
// Included through limg_hip_phase_e.h by limg_hip_kernels.hip and limg_hip_rate.hip, each one translation unit (the same per-source compile flags cover this code).
#ifndef LIMG_HIP_SEARCH_H
#define LIMG_HIP_SEARCH_H

#include "limg_hip_device.h"
#include "limg_search_table.h"

namespace limg_hip
{
  namespace
  {
    // decision automaton of the default shift search (tools/make_search_table.py); read with scalar loads
    struct __attribute__((aligned(32))) SearchEntry { uint32_t w[8]; };
    __constant__ SearchEntry d_search_tab[LIMG_SEARCH_STATES] = LIMG_SEARCH_TABLE_INIT;

    // ---- a9, packed form ------------------------------------------------------------------------------------------------
    // Same integers as `trial` above, arranged for gfx950's packed 16-bit VALU:
    //  * per factor X the three RGB terms  tXc = (decX * nX[c] + (minX[c] << 8) + 128) >> 8  are kept between trials (R,G packed in one VGPR, B in another) and
    //    only recomputed when that factor's shift changes;
    //  * they are kept NEGATED: -floor(x / 256) == floor((255 - x) / 256), so (d * -n + (255 - m)) >> 8 is minus the term at the same cost, and factor A's
    //    additive constant also carries the pixel (<< 8, per lane).  The three cached values of a channel then sum to  px - estimate  directly: no subtraction in
    //    the trial;
    //  * px - clamp(S, 0, 255) == clamp(px - S, px - 255, px), so the clamp and the difference are one max and one min against per-pixel bounds prepared once per
    //    block;
    //  * the R and G halves of a packed term carry a bias (A 0x3000, B 0x3000, C 0x2000, folded into the additive constants) that keeps every half a positive
    //    16-bit number -- one plain 32-bit add3 then adds the halves independently -- and the biases sum to 0x8000: the sum is the difference in OFFSET BINARY, which
    //    unsigned v_pk_max / v_pk_min clamp correctly against bounds biased the same way, and whose square modulo 2^16 is the square of the difference itself
    //    ((e + 0x8000)^2 = e^2 + 0x10000 e + 2^30, |e| <= 255).  So the bias is never removed;
    //  * the weighted squared error is one v_dot2_u32_u16, one select and one shift-add; without the select where the launch's pixel limit makes it dead (NOSEL).
    // Valid while every term stays inside (-0x2000, 0x2000): a term is (d * n + (min << 8) + 128) >> 8 with d <= 255 and n = max - min, so
    // |term| <= |min| + |n| + 1 <= 3 L + 1 when every record value is at most L in magnitude: L = p.recordLimit = 2700 (3 * 2700 + 1 = 8101 < 8192).  Then every
    // biased half lies in (0, 0x5100) and three of them sum to less than 65536 (no carry between the halves or out of the register).  A fit of byte pixels cannot
    // get near it (|A| <= 765, |B| <= 1020, |C| <= 2040); phase E falls back to the generic 32-bit form otherwise.
    typedef short short2_t __attribute__((ext_vector_type(2)));
    typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));
    __device__ __forceinline__ constexpr int term_bias(int factor) { return factor == 2 ? 0x2000 : 0x3000; } // sum over the factors == 0x8000
    // additive constant of factor f, channel c, for a record minimum `lo`: negated, rounding constant reflected, RG halves biased
    __device__ __forceinline__ int term_const(int f, int c, int lo) { return 255 - ((lo << 8) + 128) + (c < 2 ? (term_bias(f) << 8) : 0); }

    struct TrialState
    {
      // per pixel, fixed for the block
      uint32_t fA, fB, fC;
      uint32_t loRG, hiRG; // (R - 255 + 0x8000) | (G - 255 + 0x8000) << 16 and (R + 0x8000) | (G + 0x8000) << 16
      int pxB, pxBlo;
      // record view: n* = -(max - min) (wave-uniform), m* = term_const(...) (wave-uniform for B and C; factor A's also carry the pixel's channel << 8, per lane)
      int nA[3], nB[3], nC[3];
      int mA[3], mB[3], mC[3];
      // cached terms and the shifts they were built for
      uint32_t tA_RG, tB_RG, tC_RG;
      int tA_B, tB_B, tC_B;
      uint32_t cA, cB, cC;
    };

    __device__ __forceinline__ void make_terms(const uint32_t f, const uint32_t s, const uint32_t mul, const int n[3], const int m[3], uint32_t &tRG, int &tB)
    {
      const int d = (int)mul_u24_uniform(f >> (s & 31u), mul); // mul == shift_mul(s); <= 255 * 256; shift and multiplier are wave-uniform in the packed trial
      const int t0 = mad_i24(d, n[0], m[0]), t1 = mad_i24(d, n[1], m[1]), t2 = mad_i24(d, n[2], m[2]);
      tRG = __builtin_amdgcn_perm((uint32_t)t1, (uint32_t)t0, 0x06050201u); // ((t1 >> 8) & 0xFFFF) << 16 | ((t0 >> 8) & 0xFFFF)
      tB = t2 >> 8;
    }

    // the three factors' cached terms, each rebuilt on demand (shift 8: f >> 8 == 0 => term == minA, as upstream; for B and C upstream zeroes min too,
    // src/limg_bit_crush_simd.h:593-609)
    __device__ __forceinline__ void rebuild_A(TrialState &t, const uint32_t sA, const uint32_t mul) { make_terms(t.fA, sA, mul, t.nA, t.mA, t.tA_RG, t.tA_B); t.cA = sA; }
    __device__ __forceinline__ void rebuild_B(TrialState &t, const uint32_t sB, const uint32_t mul)
    {
      if (sB > 7) { t.tB_RG = (uint32_t)term_bias(1) * 0x10001u; t.tB_B = 0; }
      else make_terms(t.fB, sB, mul, t.nB, t.mB, t.tB_RG, t.tB_B);
      t.cB = sB;
    }
    __device__ __forceinline__ void rebuild_C(TrialState &t, const uint32_t sC, const uint32_t mul)
    {
      if (sC > 7) { t.tC_RG = (uint32_t)term_bias(2) * 0x10001u; t.tC_B = 0; }
      else make_terms(t.fC, sC, mul, t.nC, t.mC, t.tC_RG, t.tC_B);
      t.cC = sC;
    }

    // the trial proper on the cached terms: clamp, differences, weighted squared error per pixel.  NOSEL: the form without the red-weight select, for launches whose
    // pixel limit makes it dead (red_select_dead, limg_hip_encode_rules.h: same ballot, same sums); chosen per launch, a template argument all the way down
    template <bool FULL, bool NOSEL>
    __device__ __forceinline__ uint32_t trial_pixel_error(const TrialState &t, const bool active)
    {
      const uint32_t dRG = t.tA_RG + t.tB_RG + t.tC_RG; // (R - estimate + 0x8000) | (G - estimate + 0x8000) << 16: no carry crosses the halves
      const int dBraw = t.tA_B + t.tB_B + t.tC_B;        // B - estimate
      ushort2_t eu = __builtin_bit_cast(ushort2_t, dRG);
      eu = __builtin_elementwise_max(eu, __builtin_bit_cast(ushort2_t, t.loRG));
      eu = __builtin_elementwise_min(eu, __builtin_bit_cast(ushort2_t, t.hiRG));
      int dB = med3_i32(dBraw, t.pxBlo, t.pxB); // clamp(px - S, px - 255, px)
      const ushort2_t sq = eu * eu; // (d + 0x8000)^2 mod 2^16 == d^2 <= 65025
      const uint32_t sqB = (uint32_t)mul_i24(dB, dB);
      uint32_t err;
      if constexpr (NOSEL)
      { // weights (2, 4, 3) for every pixel: one dot product that also adds dB^2 once, one shift-add for the other two
        const uint32_t h = __builtin_amdgcn_udot2(sq, __builtin_bit_cast(ushort2_t, 0x00040002u), sqB, false);
        err = (sqB << 1) + h;
      }
      else
      {
        // weights (R, G, B) = (2, 4, 3) while dR^2 < 0x4000, else (3, 4, 2)  ==  2 * (dR^2 + 2 dG^2 + dB^2) + (dB^2 or dR^2): one dot product with constant
        // weights, one select (the red square is picked out of the packed pair by the select's operand modifier), one shift-add
        const bool low_red = sq.x < 0x4000;
        const uint32_t half = __builtin_amdgcn_udot2(sq, __builtin_bit_cast(ushort2_t, 0x00020001u), sqB, false);
        const uint32_t extra = low_red ? sqB : (__builtin_bit_cast(uint32_t, sq) & 0xFFFFu);
        err = (half << 1) + extra;
      }
      if (!FULL) err = active ? err : 0u;
      return err;
    }

    // a10 + a11 as a table-driven automaton: one trial loop; the outcome of a trial picks the byte offset of the next state's 32-byte entry, which one scalar load
    // fetches.  The scalar side of the loop is kept minimal -- the scalar unit (one per CU) is a co-bottleneck of this kernel: 8 extra scalar instructions per
    // trial cost 10 % (measured) -- so an entry says WHICH factors its triple changes against its predecessor's (the automaton is a tree: no compares against
    // cached shifts), holds byte offsets (no shifts) and the re-expansion multipliers, and the table's base address stays in SGPRs.  The load is NOT issued
    // ahead for both outcomes: the other waves of the SIMD cover its latency, and the two address computations, the second load and the selects between two
    // prefetched entries were scalar instructions too (measured equal, with less code).
    typedef unsigned int uint8s_t __attribute__((ext_vector_type(8)));
    __device__ __forceinline__ uint8s_t sload8(const SearchEntry *base, uint32_t byteOffset)
    {
      uint8s_t v;
      asm volatile("s_load_dwordx8 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(base), "s"(byteOffset) : "memory");
      return v;
    }

    // ---- the hot subtree of that automaton as straight-line code (limg_search_hot.h, generated) ---------------------------------------------------------------
    // A handful of the tree's states take most of the trials of every workload (tools/search_hot_paths.json).  For those the table walk is replaced by generated
    // nested code: the triple of a state is static, so shift amounts and multipliers are literals (v_lshrrev_b32 with an inline constant issues at full rate, with
    // an SGPR it does not), there is no table load, no wait and no change-mask test, and a term set is a named variable that a later state of the same path reuses
    // where the table walk -- which keeps one set per factor -- builds it again.  Which sets stay live is the generator's decision (its parameter K), not a
    // dynamic register index.  Whole blocks only: search_fast_automaton<true>.
    struct TermSet { uint32_t rg; int b; };
    // factors B and C at shift 8 contribute nothing (rebuild_B / rebuild_C): constant sets, no register
    __device__ __forceinline__ constexpr TermSet terms_shift8(int factor) { return TermSet{ (uint32_t)term_bias(factor) * 0x10001u, 0 }; }
    // make_terms for a literal shift S and its multiplier MUL == shift_mul(S): the same integers.  A factor is a byte (cvt_u8_rne_sat), so at shift 8 the
    // re-expanded value is 0 and the terms are the additive constants; below shift 4 the multiplier is 1 << S and  (f >> S) << S  is one AND with an inline
    // constant; otherwise the shift and the 24-bit multiply take their constants as immediates -- no SGPR, no scalar move.
    template <uint32_t S, uint32_t MUL>
    __device__ __forceinline__ TermSet hot_terms(const uint32_t f, const int n[3], const int m[3])
    {
      static_assert(S <= 8 && (S >= 4 || MUL == (1u << S)), "MUL is shift_mul(S)");
      int t0, t1, t2;
      if constexpr (S == 8) { t0 = m[0]; t1 = m[1]; t2 = m[2]; }
      else
      {
        uint32_t d;
        if constexpr (S < 4) d = f & ~((1u << S) - 1u);
        else asm("v_mul_u32_u24 %0, %2, %1" : "=v"(d) : "v"(f >> S), "n"(MUL));
        t0 = mad_i24((int)d, n[0], m[0]); t1 = mad_i24((int)d, n[1], m[1]); t2 = mad_i24((int)d, n[2], m[2]);
      }
      TermSet r;
      r.rg = __builtin_amdgcn_perm((uint32_t)t1, (uint32_t)t0, 0x06050201u);
      r.b = t2 >> 8;
      return r;
    }
    // one trial of a whole block on three named sets (they become the cached ones): the trial core, the pixel check and -- only if no pixel fails -- the block sum.
    // The two ways to fail reach one successor.  As a boolean (a && b, or two branches to one label in the generated code) that join travels as a lane-mask pair
    // -- s_cselect_b64, s_andn2_b64 and a second branch: profiles/search_hot_ab.md -- so the outcome is one scalar WORD instead: 0 where a pixel fails, else the
    // high word of the block sum's compare mask (wave_sum_below: lane 63's bit is its sign), opaque to the compiler behind the join.  A pixel failure is then its
    // branch over the sum plus the common sign test, a sum failure the sign test alone.  (asm goto would leave only the branches; this compiler drops the asm of
    // an asm goto on gfx950.)
    template <bool NOSEL>
    __device__ __forceinline__ bool hot_trial(TrialState &t, const TermSet &A, const TermSet &B, const TermSet &C, const uint32_t maxPixel32, const uint32_t blockLimit)
    {
      t.tA_RG = A.rg; t.tA_B = A.b; t.tB_RG = B.rg; t.tB_B = B.b; t.tC_RG = C.rg; t.tC_B = C.b;
      const uint32_t err = trial_pixel_error<true, NOSEL>(t, true);
      uint32_t verdict = 0u;
      if (__builtin_amdgcn_ballot_w64(err > maxPixel32) == 0ull) verdict = wave_sum_below_mask(err, blockLimit); // be * 16 < maxBlock * n, see phase E
      asm("" : "+s"(verdict));
      return (int)verdict < 0;
    }
#include "limg_search_hot.h"

    template <bool FULL, bool NOSEL>
    __device__ __forceinline__ void search_fast_automaton(TrialState &t, const bool active, const uint32_t maxPixel32, const uint32_t blockLimit, uint32_t shift[3])
    {
      const SearchEntry *tab = d_search_tab;
      uint8s_t e;
      if constexpr (FULL)
      { // whole blocks: the generated hot subtree first; it ends the search itself or hands over the offset of the table entry to go on with (the state's three
        // sets are the cached ones, and the entry names its changes against exactly that triple)
        uint32_t off;
        if (search_hot<NOSEL>(t, maxPixel32, blockLimit, shift, off)) return;
        asm volatile("" : "+s"(tab)); // opaque: otherwise the address is rematerialised (s_getpc + 2 adds) in every iteration
        e = sload8(tab, off);
      }
      else
      {
        asm volatile("" : "+s"(tab)); // (as above)
        // entry 0 as immediates (the opaque base above would make reading it a memory round trip per block)
        // its three factors are built here, unconditionally and with immediate operands (the loop then starts with nothing to rebuild): the cached terms need no
        // initial value at all
        constexpr uint32_t root[8] = LIMG_SEARCH_ROOT;
        rebuild_A(t, root[0] & 31u, root[5]);
        rebuild_B(t, root[3], root[6]);
        rebuild_C(t, root[4], root[7]);
        e = uint8s_t{ root[0] & ~0xE0u, root[1], root[2], root[3], root[4], root[5], root[6], root[7] };
      }
      while (!(e[0] >> 31))
      { // every field sits in an SGPR of its own: no extraction.  (e[0] & 31 is the shift amount as v_lshrrev_b32 reads it -- the mask costs nothing)
        if (e[0] & 0x20u) rebuild_A(t, e[0] & 31u, e[5]);
        if (e[0] & 0x40u) rebuild_B(t, e[3], e[6]);
        if (e[0] & 0x80u) rebuild_C(t, e[4], e[7]);
        const uint32_t err = trial_pixel_error<FULL, NOSEL>(t, active);
        // two tails on purpose: a pixel failure (the common way to fail) needs no outcome flag, no select and no block sum
        uint32_t off = e[2];
        if (__builtin_amdgcn_ballot_w64(err > maxPixel32) == 0ull)
        {
          if (wave_sum_below(err, blockLimit)) off = e[1]; // be * 16 < maxBlock * n, see phase E
        }
        e = sload8(tab, off);
      }
      shift[0] = e[0] & 31u; shift[1] = e[3]; shift[2] = e[4];
    }

    // a12 as an automaton (limg_search_table_accurate.h, a DAG of ~19 k states in global memory, expanded by the context): which trials the accurate search runs
    // depends on pass / fail outcomes only, so its three nested scalar loops -- which, not the trials, were the cost of this mode -- become one table walk.  What
    // the block errors decide stays here: a passing phase-1 trial becomes the result; a passing phase-2 trial only if its error is below the best so far
    // (src/limg_bit_crush.h:774-826; `have` is always set by then).  A state has several predecessors, so the factors to rebuild come from comparing with the cached
    // shifts (t.cA..cC).
    template <bool FULL, bool NOSEL>
    __device__ __forceinline__ void search_accurate_automaton(TrialState &t, const bool active, const uint32_t maxPixel32, const uint32_t blockLimit, const uint32_t *table,
                                                              uint32_t shift[3])
    {
      const SearchEntry *tab = reinterpret_cast<const SearchEntry *>(table);
      uint32_t bestA = 0, bestB = 0, bestC = 0, minBe = 0xFFFFFFFFu;
      // Measured and NOT adopted (removed from the tree, see git history): the accurate search walks the shift cube row by row -- c innermost
      // (src/limg_bit_crush.h:700-760) -- so factor C's shift changes with nearly every one of its ~70 trials per block while it only takes nine values; its terms for
      // the shifts 0..7 can be built once per block and picked per trial out of a 16-register vector with the wave-uniform shift as the index (VGPR index mode:
      // s_set_gpr_idx_on, two v_mov, s_set_gpr_idx_off; one 16-wide vector because LLVM expands a dynamic extract of up to 8 elements into compares and selects).
      // At equal occupancy that is 2 % faster (4.39 vs 4.49 ms at 5 workgroups per CU), but its 16 registers cost the sixth workgroup per CU, which is worth 7.5 %
      // (4.16 ms without the cache at 6).
      { // the first triple is the fast search's
        constexpr uint32_t root[8] = LIMG_SEARCH_ROOT;
        rebuild_A(t, root[0] & 31u, root[5]);
        rebuild_B(t, root[3], root[6]);
        rebuild_C(t, root[4], root[7]);
      }
      uint8s_t e = sload8(tab, 0u);
      // which factors state 0's triple changes against the root triple built above (every later edge carries its mask in bits 24..26 of the successor offset)
      constexpr uint32_t rootT[8] = LIMG_SEARCH_ROOT;
      uint32_t mask = ((e[0] & 31u) != (rootT[0] & 31u) ? 1u : 0u) | (e[3] != rootT[3] ? 2u : 0u) | (e[4] != rootT[4] ? 4u : 0u);
      while (!(e[0] >> 31))
      {
        const uint32_t a = e[0] & 31u;
        if (mask & 1u) rebuild_A(t, a, e[5]);
        if (mask & 2u) rebuild_B(t, e[3], e[6]);
        if (mask & 4u) rebuild_C(t, e[4], e[7]);
        const uint32_t err = trial_pixel_error<FULL, NOSEL>(t, active);
        uint32_t off = e[2];
        if (__builtin_amdgcn_ballot_w64(err > maxPixel32) == 0ull)
        {
          const uint32_t be = wave_sum(err);
          if (be < blockLimit) // be * 16 < maxBlock * n, see phase E
          {
            off = e[1];
            if (!(e[0] & 0x20u) || be < minBe) { bestA = a; bestB = e[3]; bestC = e[4]; minBe = be; }
          }
        }
        mask = off >> 24;
        e = sload8(tab, off & 0xFFFFFFu);
      }
      shift[0] = bestA; shift[1] = bestB; shift[2] = bestC;
    }

    // generic-path search (see phase E): real function, rarely if ever executed
    __device__ __attribute__((noinline)) uint32_t search_generic(uint32_t px, uint32_t fA, uint32_t fB, uint32_t fC, const int16_t *rec /* LDS */, bool active,
                                                                 uint32_t maxPixel32, uint64_t maxBlockN, bool fast)
    {
      RecU r;
#pragma unroll
      for (int c = 0; c < 3; c++)
      {
        const int loA = rec[c], hiA = rec[4 + c], loB = rec[8 + c], hiB = rec[12 + c], loC = rec[16 + c], hiC = rec[20 + c];
        r.nA[c] = sgpr(hiA - loA); r.nB[c] = sgpr(hiB - loB); r.nC[c] = sgpr(hiC - loC);
        r.mA[c] = sgpr((int)(((uint32_t)loA << 8) + 128u)); r.mB[c] = sgpr((int)(((uint32_t)loB << 8) + 128u)); r.mC[c] = sgpr((int)(((uint32_t)loC << 8) + 128u));
      }
      uint32_t shift[3] = { 0, 0, 0 };
      auto T = [&](uint32_t a, uint32_t bb, uint32_t c, uint32_t &be2) -> bool { return trial(px, fA, fB, fC, r, a, bb, c, active, maxPixel32, maxBlockN, be2); };
      if (fast) search_fast(T, shift);
      else search_accurate(T, shift);
      return shift[0] | (shift[1] << 8) | (shift[2] << 16);
    }
  } // namespace
} // namespace limg_hip

#endif
