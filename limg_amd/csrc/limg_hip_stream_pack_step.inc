// limg_hip_stream_pack_step.inc -- the pack step of the strip-form packers (limg_hip_stream.hip), included INSIDE the strip loop of k_stream_pack_strips and of
// k_stream_pack_strips_batch: one text for both.  Not a function: called through one -- arguments by reference or by value alike -- k_stream_pack_strips gets
// another register allocation and schedule than the one it was measured with; included, its code is instruction for instruction what it was when the step stood
// in its loop.
// From the enclosing scope: p (.stripsX, .blocksX, .stream: the strip's image), strip (its number inside that image), payload (the image's payload area),
// cur / rows (the strip's records and rows, in registers), sRun / sEnt (the wave's LDS), lane, j, h.
// Writes the strip's entries and its contiguous payload run, built in the wave's LDS.
const uint32_t by = strip / p.stripsX, sx = strip - by * p.stripsX;
const uint32_t inStrip = min(32u, p.blocksX - sx * 32u);
const uint32_t bits = rows.bits, words = words_of(bits);
// exclusive prefix of the words over the strip's blocks (both halves compute it)
uint32_t incl = words; // (wave_scan_inclusive over 32 lanes, written out: through a width parameter there this kernel's measured schedule changes)
#pragma unroll
for (int off = 1; off < 32; off <<= 1)
{
  const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 32);
  if (j >= off) incl += up;
}
const uint32_t total = (uint32_t)__shfl((int)incl, 31, 32);
const uint32_t excl = incl - words;
if (h == 0)
{
  uint32_t *e = sEnt + j * 14;
  *reinterpret_cast<uint2 *>(e + 0) = make_uint2(cur.r0.x, cur.r0.y); *reinterpret_cast<uint2 *>(e + 2) = make_uint2(cur.r0.z, cur.r0.w);
  *reinterpret_cast<uint2 *>(e + 4) = make_uint2(cur.r1.x, cur.r1.y); *reinterpret_cast<uint2 *>(e + 6) = make_uint2(cur.r1.z, cur.r1.w);
  *reinterpret_cast<uint2 *>(e + 8) = make_uint2(cur.r2.x, cur.r2.y); *reinterpret_cast<uint2 *>(e + 10) = make_uint2(cur.r2.z, cur.r2.w);
  *reinterpret_cast<uint2 *>(e + 12) = make_uint2(cur.sw | (bits & 0xFF000000u), cur.base + excl);
}
{
  uint32_t *field = sRun + 2u * excl; // dwords
#pragma unroll
  for (int k = 0; k < 3; k++)
  {
    const uint32_t b = (bits >> (8 * k)) & 0xFFu;
    if (b == 0u) continue;
    const uint32_t sh = 8u - b, m1 = (1u << b) - 1u, m4 = m1 * 0x01010101u, mPair = (m1 * 0x00010001u) << b;
    uint32_t *dst = field + (uint32_t)h * b; // rows 4 h .. 4 h + 3 are bytes [4 h b, 4 h b + 4 b) of the field: b dwords
    const uint32_t len0 = b < 4u ? b : 4u, len1 = b - len0; // a row goes in as its low (up to) 4 bytes, then the rest: never more than 3 + 4 bytes in acc
    unsigned long long acc = 0;
    uint32_t fill = 0; // bytes in acc (< 4 between appends)
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
      const unsigned long long v = squeeze_row(rows.raw[k][r].x, rows.raw[k][r].y, sh, b, m4, mPair);
      acc |= (unsigned long long)(uint32_t)v << (8u * fill);
      fill += len0;
      if (fill >= 4u) { *dst++ = (uint32_t)acc; acc >>= 32; fill -= 4u; }
      acc |= (unsigned long long)(uint32_t)(v >> 32) << (8u * fill);
      fill += len1;
      if (fill >= 4u) { *dst++ = (uint32_t)acc; acc >>= 32; fill -= 4u; }
    }
    field += 2u * b;
  }
}
wave_lds_fence();
{
  uint2 *edst = reinterpret_cast<uint2 *>(p.stream + sizeof(limg_hip_stream_header) + ((size_t)by * p.blocksX + sx * 32u) * kEntry);
  const uint2 *esrc = reinterpret_cast<const uint2 *>(sEnt);
  for (uint32_t i = lane; i < inStrip * (kEntry / 8); i += 64) edst[i] = esrc[i];
  // the run in 16-byte stores: the payload area is 8-byte aligned, so a run that starts on an odd word sends that word ahead (the LDS side is then read at
  // 8-byte alignment, which ds_read_b128 does not allow: two ds_read_b64)
  uint2 *pdst = payload + (size_t)cur.base;
  const uint2 *psrc = reinterpret_cast<const uint2 *>(sRun);
  const uint32_t odd = (uint32_t)((reinterpret_cast<uintptr_t>(pdst) >> 3) & 1u) & (total ? 1u : 0u);
  if (odd && lane == 0) pdst[0] = psrc[0];
  const uint32_t pairs = (total - odd) >> 1;
  uint4 *p4 = reinterpret_cast<uint4 *>(pdst + odd);
  for (uint32_t i = lane; i < pairs; i += 64)
  {
    const uint2 a = psrc[odd + 2u * i], b2 = psrc[odd + 2u * i + 1u];
    p4[i] = make_uint4(a.x, a.y, b2.x, b2.y);
  }
  if (((total - odd) & 1u) && lane == 0) pdst[total - 1u] = psrc[total - 1u];
}
wave_lds_fence(); // the run is read: the next strip may overwrite it
