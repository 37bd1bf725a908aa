// limg_hip_list_plan.h -- the layout of a stream-encode list whose images differ in shape (limg_hip_encode_stream_list*), stated ONCE for the host route and the
// kernels that walk it: which items may share the launches, where an image's blocks, strips and float-stage units start in the chunk's concatenated arrays, the
// 16-byte access flags and the dither-chain partition of THAT image, a chunk's totals and its noise need, and where a chunk ends.  A host compiler builds it on
// its own (tests/helpers/list_plan_check.cpp).  Plain C++: no HIP types, no library.
#ifndef LIMG_HIP_LIST_PLAN_H
#define LIMG_HIP_LIST_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "limg_hip_encode_plan.h"

namespace limg_hip
{
  // ---- eligibility: what k_encode_list_rated asks of its list, per item -- whole blocks, the default search, the persistent path behind k_fit_tpb ----
  inline bool list_item_eligible(size_t sizeX, size_t sizeY, int fastBitCrushing, const limg_hip_options &o)
  {
    const EncodeShape sh(sizeX, sizeY);
    return sh.valid && list_in_one_pair(sh, o) && fastBitCrushing != 0;
  }

  constexpr uint32_t kListUnitBlocks = 64; // a float-stage unit: up to 64 adjacent blocks of one block row of ONE image (a wave of k_fit_tpb_list)

  // ---- one image of a chunk: its own geometry and where its slices start ----
  // The device table entry (64 bytes, next to the ImageIO / RatedImage / StreamImage entries of the same index): read with scalar loads, once per work item.
  struct ListImage
  {
    uint64_t firstBlock;  // of its slice of the records, invN (x 4 floats) and shift words
    uint32_t firstStrip;  // its first work strip id: look-back descriptors and payload words are indexed by firstStrip + local strip
    uint32_t strips;      // stripsX * blocksY
    uint32_t firstUnit;   // its first float-stage unit; it has ceil(blocksX / 64) * blocksY of them
    uint32_t sizeX, sizeY, blocksX, blocksY, stripsX;
    uint32_t nBlocks;     // blocksX * blocksY (a stream's table has 32-bit indices: limg_hip_stream_bound)
    uint32_t chainCount, chainRows; // partition(sizeY, poolThreads): every image starts its own chains
    uint32_t vec;         // kListVec*: the 16-byte access flags of THIS image (not the & over the list: widths differ)
    uint32_t pad[2];
  };
  static_assert(sizeof(ListImage) == 64, "one entry of the list table");
  enum { kListVecIn = 1u, kListVecPlanes = 2u, kListVecFactors8 = 4u, kListVecDecoded = 8u, kListVecFactors = 16u };

  inline uint32_t list_vec_bits(const VecAccess &v)
  {
    return (v.in ? kListVecIn : 0u) | (v.planes ? kListVecPlanes : 0u) | (v.factors8 ? kListVecFactors8 : 0u) | (v.decoded ? kListVecDecoded : 0u) | (v.factors ? kListVecFactors : 0u);
  }
  inline uint32_t list_units(const EncodeShape &sh) { return (uint32_t)(((sh.blocksX + kListUnitBlocks - 1) / kListUnitBlocks) * sh.blocksY); }
  // dither calls the longest chain of an image can make: every block at most 3; the last chain takes the remainder, never fewer rows than the others
  inline uint64_t list_chain_calls(const EncodeShape &sh, const Partition &pt)
  {
    uint64_t maxRows = sh.blocksY;
    if (pt.chainCount > 1 && (uint64_t)(pt.chainCount - 1) * pt.chainRows < sh.blocksY) maxRows = sh.blocksY - (uint64_t)(pt.chainCount - 1) * pt.chainRows;
    return maxRows * sh.blocksX * 3;
  }

  // ---- a chunk: the images [i0, i0 + n) of the eligible list, concatenated ----
  struct ListChunkTotals
  {
    uint64_t blocks;     // records / invN / shift words of the chunk
    uint32_t strips;     // work strips (32-bit ids)
    uint32_t units;      // float-stage units
    uint64_t noiseCalls; // the noise table's need: the LARGEST per-chain call count of any image (every image starts its own chains at the seed), not their sum
    bool vecInAll;       // every image's rows may be read 16 bytes per lane: the float stage's DIRECT instances
  };

  // Where the chunk that starts at image i0 ends: the plane batch's rule (1 GiB of block records, 32-bit strip ids, the test build's batch_chunk = images per
  // chunk) counted in blocks and strips SUMMED over the images; at least one image.  blocks[i], strips[i]: of image i, both > 0.
  inline size_t list_chunk_end(const uint64_t *blocks, const uint64_t *strips, size_t count, size_t i0, size_t hook)
  {
    const uint64_t maxBlocks = (1ull << 30) / sizeof(limg_hip_block_record), maxStrips = 0x7FFFFFFFull;
    uint64_t b = 0, s = 0;
    size_t i = i0;
    for (; i < count; i++)
    {
      if (hook > 0 && i - i0 >= hook) break;
      if (i > i0 && (b + blocks[i] > maxBlocks || s + strips[i] > maxStrips)) break;
      b += blocks[i]; s += strips[i];
    }
    return i > i0 ? i : (i0 < count ? i0 + 1 : i0);
  }

  // entry i of a chunk, given the totals of the images in front of it (which it then advances).  in / facs: the image's input and its three factor planes.
  inline ListImage list_image(ListChunkTotals &t, size_t sizeX, size_t sizeY, int poolThreads, const uint32_t *in, uint8_t *const fac[3])
  {
    const EncodeShape sh(sizeX, sizeY);
    const Partition pt = partition(sizeY, poolThreads);
    limg_hip_encode3d_info info = {};
    info.pFactorsA = fac[0]; info.pFactorsB = fac[1]; info.pFactorsC = fac[2];
    const VecAccess v = vec_access(in, &info, sizeX, false);
    ListImage e = {};
    e.firstBlock = t.blocks; e.firstStrip = t.strips; e.firstUnit = t.units;
    e.strips = (uint32_t)sh.strips;
    e.sizeX = (uint32_t)sizeX; e.sizeY = (uint32_t)sizeY; e.blocksX = (uint32_t)sh.blocksX; e.blocksY = (uint32_t)sh.blocksY; e.stripsX = (uint32_t)sh.stripsX;
    e.nBlocks = (uint32_t)sh.blocks;
    e.chainCount = pt.chainCount; e.chainRows = pt.chainRows;
    e.vec = list_vec_bits(v);
    const uint64_t calls = list_chain_calls(sh, pt);
    if (t.blocks == 0 && t.strips == 0) t.vecInAll = true;
    t.vecInAll = t.vecInAll && v.in;
    if (calls > t.noiseCalls) t.noiseCalls = calls;
    t.blocks += sh.blocks; t.strips += (uint32_t)sh.strips; t.units += list_units(sh);
    return e;
  }

  // one of an image's three factor planes in the chunk's scratch: 256-byte aligned slices
  inline size_t list_plane_stride(size_t sizeX, size_t sizeY) { return (sizeX * sizeY + 255) & ~(size_t)255; }

  // ---- the tables of one chunk of n images, side by side in one device block: where each part starts (16-byte aligned), given the bytes of one entry of each part:
  // the image's view (RatedListParams), its ListImage, ImageIO, RatedImage, StreamImage and its two prefix words ----
  struct ChunkEntrySizes { size_t view, image, io, rated, stream, firstStrip, firstUnit; };
  struct ChunkTables
  {
    size_t views, images, io, rated, streams, firstStrip, firstUnit, bytes;
    ChunkTables(size_t n, const ChunkEntrySizes &e)
    {
      auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
      views = 0; images = up(views + n * e.view); io = up(images + n * e.image); rated = up(io + n * e.io);
      streams = up(rated + n * e.rated); firstStrip = up(streams + n * e.stream); firstUnit = up(firstStrip + n * e.firstStrip); bytes = up(firstUnit + n * e.firstUnit);
    }
  };

  // ---- what the largest chunk of a list asks of the scratch: the chunks of more than one image (list_chunk_end; one image alone takes the single call), each
  // member the maximum over them -- everything is grown once, before the first launch.  facBytes[i]: image i's three factor planes ----
  struct ListNeeds { size_t images; uint64_t blocks, strips; size_t facBytes; };
  inline ListNeeds list_needs(const uint64_t *blocks, const uint64_t *strips, const size_t *facBytes, size_t count, size_t hook)
  {
    ListNeeds most = {};
    for (size_t i0 = 0; i0 < count;)
    {
      const size_t i1 = list_chunk_end(blocks, strips, count, i0, hook);
      if (i1 - i0 > 1)
      {
        ListNeeds n = { i1 - i0, 0, 0, 0 };
        for (size_t i = i0; i < i1; i++) { n.blocks += blocks[i]; n.strips += strips[i]; n.facBytes += facBytes[i]; }
        if (n.images > most.images) most.images = n.images;
        if (n.blocks > most.blocks) most.blocks = n.blocks;
        if (n.strips > most.strips) most.strips = n.strips;
        if (n.facBytes > most.facBytes) most.facBytes = n.facBytes;
      }
      i0 = i1;
    }
    return most;
  }
}

#endif
