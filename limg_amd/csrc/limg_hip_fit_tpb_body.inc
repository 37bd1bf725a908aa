// limg_hip_fit_tpb_body.inc -- the float stage with one lane per block, included as the BODY of k_fit_tpb and of k_fit_tpb_list (limg_hip_fit_tpb.hip): one text for
// both, in two parts.  Not a function, for the reason limg_hip_persistent_loop.inc gives: included, k_fit_tpb's instances are instruction for instruction what they
// were when the text stood in the kernel.
// LIMG_FIT_TPB_TABLE: the RSQRTPS table into LDS (s_tab; FAST, kTpbWaves from the enclosing scope) -> tab.
// Otherwise the body proper.  From the enclosing scope: CH, FAST, DIRECT; p (.sizeX, .blocksX, .vecIn, .records, .invN: of the unit's image); pin (its pixels); byS (the
// unit's block row in p.records / p.invN), bx0, x0, y0, nBlocks, widthPx (the unit); lane, s_px, tab.
#ifdef LIMG_FIT_TPB_TABLE
      if (!FAST)
      {
        const uint4 *src = reinterpret_cast<const uint4 *>(d_rsqrt_x86_tab);
        for (int i = (int)threadIdx.x; i < 256; i += 64 * kTpbWaves)
        {
          const uint4 v = src[i]; // entries 8 i .. 8 i + 7
          const uint32_t q[4] = { v.x, v.y, v.z, v.w };
          uint32_t *dst = s_tab + ((8 * i) ^ 0x400);
#pragma unroll
          for (int k = 0; k < 4; k++) { dst[2 * k] = (q[k] & 0xFFFFu) << 11; dst[2 * k + 1] = (q[k] >> 16) << 11; }
        }
        __syncthreads();
      }
      const unsigned short *tab = reinterpret_cast<const unsigned short *>(s_tab);
#else
      // ---- stage the 8 pixel rows (coalesced 16 bytes per lane) into the block-major layout ----
      if (!DIRECT)
      {
      if (p.vecIn)
      {
#pragma unroll
        for (int row = 0; row < 8; row++)
          for (uint32_t col = (uint32_t)lane * 4u; col < widthPx; col += 256u)
          {
            const uint4 v = *reinterpret_cast<const uint4 *>(pin + (size_t)(y0 + row) * p.sizeX + x0 + col);
            *reinterpret_cast<uint4 *>(&s_px[(col >> 3) * kTpbStride + row * 8 + (col & 7u)]) = v;
          }
      }
      else
      {
        for (int row = 0; row < 8; row++)
          for (uint32_t col = (uint32_t)lane; col < widthPx; col += 64u)
            s_px[(col >> 3) * kTpbStride + row * 8 + (col & 7u)] = pin[(size_t)(y0 + row) * p.sizeX + x0 + col];
      }
      }
      wave_lds_fence();
      if ((uint32_t)lane >= nBlocks) return;
      const uint32_t *my = DIRECT ? pin + (size_t)y0 * p.sizeX + x0 + lane * 8 : s_px + lane * kTpbStride;
      const uint32_t pitch = DIRECT ? p.sizeX : 8u;

      // ---- a4: channel sums (src/limg.cpp:466-497); two channels per 32-bit accumulator, 64 * 255 < 2^16 ----
      uint32_t s02 = 0, s13 = 0;
#pragma unroll
      for (int r = 0; r < 8; r++)
      {
        const uint4 u = *reinterpret_cast<const uint4 *>(my + r * pitch), w = *reinterpret_cast<const uint4 *>(my + r * pitch + 4);
        const uint32_t q[8] = { u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w };
#pragma unroll
        for (int i = 0; i < 8; i++) { s02 += q[i] & 0x00FF00FFu; s13 += (q[i] >> 8) & 0x00FF00FFu; }
      }
      const float inv_count = 0.015625f;
      V4 avg;
      avg.a = float2_t{ (float)(int)(s02 & 0xFFFF), (float)(int)(s02 >> 16) } * inv_count;
      avg.b = float2_t{ (float)(int)(s13 & 0xFFFF), CH == 4 ? (float)(int)(s13 >> 16) : 0.0f } * inv_count;
      const V4 zero4 = { float2_t{ 0.0f, 0.0f }, float2_t{ 0.0f, 0.0f } };

      // the epilogue of a direction sum: dir = sum / N, 1 / (dir . dir) in DPPS order, all-zero test (== serial_sums2 of limg_hip_float_pixel.h)
      auto finish_dir = [&](const V4 &acc, V4 &dir, float &inv, bool &zero)
      {
        dir = acc * inv_count;
        const float pp = dp4<CH>(dir, dir); // plain products even in FAST mode: the lane == pixel path does the same
        zero = dir.a.x == 0.0f && dir.a.y == 0.0f && dir.b.x == 0.0f && dir.b.y == 0.0f;
        inv = FAST ? __builtin_amdgcn_rcpf(pp) : 1.0f / pp;
      };

      // ---- pass 1 (src/limg_factorization.h:602-628): sign-normalised unit vectors of px - avg, summed in pixel order ----
      V4 dirA, dirB = zero4, dirC = zero4, est0 = zero4;
      float invA, invB = 0.0f, invC = 0.0f;
      bool zeroA, zeroB = true, zeroC = true;
      float mm[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
      {
        V4 acc = zero4;
        for_rows(my, pitch, [&](const int, const uint32_t (&q)[8])
        {
#pragma unroll
          for (int i = 0; i < 8; i++)
          {
            V4 d = px_to_v4(q[i]) - avg;
            mask_alpha<CH>(d);
            acc = acc + unit4<CH, FAST, true, true>(tab, d, true);
          }
        });
        finish_dir(acc, dirA, invA, zeroA);
      }

      // ---- pass 2 (:652-688): factor A extrema, residual -> second direction ----
      if (!zeroA)
      {
        V4 acc = zero4;
        float mn = 0.0f, mx = 0.0f; // upstream starts them at 0 (:633-634)
        for_rows(my, pitch, [&](const int, const uint32_t (&q)[8])
        {
#pragma unroll
          for (int i = 0; i < 8; i++)
          {
            const V4 pf = px_to_v4(q[i]);
            const float fA = dp4<CH, FAST>(pf - avg, dirA) * invA;
            mn = vmin(mn, fA); mx = vmax(mx, fA);
            V4 e = pf - (avg + dirA * fA);
            mask_alpha<CH>(e);
            acc = acc + unit4<CH, FAST, true, true>(tab, e, true);
          }
        });
        mm[0] = mn; mm[1] = mx;
        finish_dir(acc, dirB, invB, zeroB);
      }

      // ---- pass 3 ----
      if (!zeroA && !zeroB)
      {
        float mnB = FLT_MAX, mxB = -FLT_MAX;
        if (CH == 4)
        { // :701-738: factor B extrema, residual -> third direction; the A+B estimate of pixel 0 is what pass 4 measures every pixel against (:748-758)
          V4 acc = zero4;
          for_rows(my, pitch, [&](const int r, const uint32_t (&q)[8])
          {
#pragma unroll
            for (int i = 0; i < 8; i++)
            {
              const V4 pf = px_to_v4(q[i]);
              const float fA = dp4<CH, FAST>(pf - avg, dirA) * invA; // recomputed, same operations => same bits as pass 2's
              const V4 estA = avg + dirA * fA;
              const float fB = dp4<CH, FAST>(pf - estA, dirB) * invB;
              mnB = vmin(mnB, fB); mxB = vmax(mxB, fB);
              const V4 estB = estA + dirB * fB;
              if (r == 0 && i == 0) est0 = estB;
              acc = acc + unit4<CH, FAST, true, true>(tab, pf - estB, true);
            }
          });
          mm[2] = mnB; mm[3] = mxB;
          finish_dir(acc, dirC, invC, zeroC);
          // ---- pass 4 (:748-758) ----
          if (!zeroC)
          {
            float mnC = FLT_MAX, mxC = -FLT_MAX;
            for_rows(my, pitch, [&](const int, const uint32_t (&q)[8])
            {
#pragma unroll
              for (int i = 0; i < 8; i++)
              {
                const float fC = dp4<CH, FAST>(px_to_v4(q[i]) - est0, dirC) * invC;
                mnC = vmin(mnC, fC); mxC = vmax(mxC, fC);
              }
            });
            mm[4] = mnC; mm[5] = mxC;
          }
        }
        else
        { // 3 channels (:498-541): dirC = dirA x dirB, B and C extrema in one pass; slots: a = (x0, x2), b = (x1, x3)
          dirC.a.x = dirA.b.x * dirB.a.y - dirA.a.y * dirB.b.x; // A1 B2 - A2 B1
          dirC.b.x = dirA.a.y * dirB.a.x - dirA.a.x * dirB.a.y; // A2 B0 - A0 B2
          dirC.a.y = dirA.a.x * dirB.b.x - dirA.b.x * dirB.a.x; // A0 B1 - A1 B0
          dirC.b.y = 0.0f;
          zeroC = dirC.a.x == 0.0f && dirC.b.x == 0.0f && dirC.a.y == 0.0f;
          if (!zeroC) invC = FAST ? __builtin_amdgcn_rcpf(dp4<CH, FAST>(dirC, dirC)) : 1.0f / dp4<CH, FAST>(dirC, dirC);
          float mnC = zeroC ? 0.0f : FLT_MAX, mxC = zeroC ? 0.0f : -FLT_MAX;
          for_rows(my, pitch, [&](const int, const uint32_t (&q)[8])
          {
#pragma unroll
            for (int i = 0; i < 8; i++)
            {
              const V4 pf = px_to_v4(q[i]);
              const float fA = dp4<CH, FAST>(pf - avg, dirA) * invA;
              const V4 estA = avg + dirA * fA;
              const float fB = dp4<CH, FAST>(pf - estA, dirB) * invB;
              mnB = vmin(mnB, fB); mxB = vmax(mxB, fB);
              if (!zeroC)
              {
                const V4 e = pf - (estA + dirB * fB);
                const float fC = dp4<CH, FAST>(e, dirC) * invC;
                mnC = vmin(mnC, fC); mxC = vmax(mxC, fC);
              }
            }
          });
          mm[2] = mnB; mm[3] = mxB; mm[4] = mnC; mm[5] = mxC;
        }
      }

      // ---- record (src/limg_factorization.h:764-790): avg + extreme * dir for A, extreme * dir for B and C, round to nearest even, int16 ----
      const bool deadA = zeroA, deadB = zeroA || zeroB, deadC = zeroA || zeroB || zeroC;
      auto comp = [](const V4 &v, int c) -> float { return c == 0 ? v.a.x : (c == 1 ? v.b.x : (c == 2 ? v.a.y : v.b.y)); };
      uint32_t words[16];
#pragma unroll
      for (int c = 0; c < 4; c++) words[c] = __float_as_uint(comp(avg, c));
      // Factor by factor, so that nothing but the factor's eight values is live: the record's int16 pairs, and -- a7 (limg_init_color_error_state_3d,
      // src/limg_internal.h:426-452) -- 1 / (n . n) of the INTEGER normal max - min in the serial limg_dot order, 0 for an all-zero normal.  Here that is three
      // divisions per 64 blocks; in the E step (lane == pixel, one lane per (block, factor, channel)) it was four DPP broadcasts and a correctly rounded division per
      // lane and strip: ~7 vector instructions per block.
      float inv[3];
#pragma unroll
      for (int r = 0; r < 3; r++)
      {
        const bool dead = r == 0 ? deadA : (r == 1 ? deadB : deadC);
        const V4 &dir = r == 0 ? dirA : (r == 1 ? dirB : dirC);
        int16_t lo[4], hi[4];
        float sum = 0.0f;
        bool nz = false;
#pragma unroll
        for (int c = 0; c < 4; c++)
        {
          float dv = comp(dir, c), mLo = mm[2 * r], mHi = mm[2 * r + 1];
          if (dead) { mLo = 0.0f; mHi = 0.0f; dv = 0.0f; }
          float vLo = mLo * dv, vHi = mHi * dv;
          if (r == 0) { vLo = comp(avg, c) + vLo; vHi = comp(avg, c) + vHi; }
          int qLo = cvt_rne(vLo), qHi = cvt_rne(vHi);
          if (CH == 3 && c == 3) { qLo = 0; qHi = 0; }
          lo[c] = (int16_t)qLo; hi[c] = (int16_t)qHi;
          if (CH == 4 || c < 3)
          {
            const float n = (float)((int)hi[c] - (int)lo[c]);
            const float sq = n * n;
            sum = sum + sq; // ((0 + s0) + s1) + s2 (+ s3)
            nz = nz || sq != 0.0f;
          }
        }
        inv[r] = nz ? (FAST ? __builtin_amdgcn_rcpf(sum) : 1.0f / sum) : 0.0f;
        words[4 + 4 * r] = (uint32_t)(uint16_t)lo[0] | ((uint32_t)(uint16_t)lo[1] << 16);
        words[5 + 4 * r] = (uint32_t)(uint16_t)lo[2] | ((uint32_t)(uint16_t)lo[3] << 16);
        words[6 + 4 * r] = (uint32_t)(uint16_t)hi[0] | ((uint32_t)(uint16_t)hi[1] << 16);
        words[7 + 4 * r] = (uint32_t)(uint16_t)hi[2] | ((uint32_t)(uint16_t)hi[3] << 16);
      }
      uint4 *dst = reinterpret_cast<uint4 *>(p.records + (size_t)byS * p.blocksX + bx0 + lane);
#pragma unroll
      for (int i = 0; i < 4; i++) dst[i] = make_uint4(words[4 * i], words[4 * i + 1], words[4 * i + 2], words[4 * i + 3]);
      reinterpret_cast<float4 *>(p.invN)[(size_t)byS * p.blocksX + bx0 + lane] = make_float4(inv[0], inv[1], inv[2], 0.0f);
#endif
