// limg_hip_splice_plan.h -- what the host decides about a stream splice (limg_hip_stream_splice*, include/limg_hip.h) before anything is launched: whether the pieces
// obey the rules, and the runs the kernels of limg_hip_stream_splice.hip work through.  A piece is a rectangle of 8x8 blocks of one version 1 source stream and the
// place of its first block in the output's block grid; a RUN is one block row of one piece.  Inside a block row the table entries of consecutive blocks are
// consecutive and -- the table's payloadWord being the exclusive prefix of the blocks' words in raster order -- so is their payload, in the source and in the
// output alike: a run is copied as one range of entries and one range of payload words.
// Host-only C++ without HIP types: tests/helpers/splice_plan_check.cpp builds it with the host compiler (tests/test_splice_plan_cpu.py).
#ifndef LIMG_HIP_SPLICE_PLAN_H
#define LIMG_HIP_SPLICE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace limg_hip
{
  // a piece without its stream: the geometry of limg_hip_splice_piece
  struct SplicePiece
  {
    uint32_t srcSizeX, srcSizeY; // the source image
    uint32_t srcBx, srcBy;       // first source block
    uint32_t dstBx, dstBy;       // where it lands in the output's block grid
    uint32_t blocksW, blocksH;   // in blocks
  };
  // one block row of one piece: `count` consecutive entries from srcEntry of the piece's source to dstEntry of the output (both raster indices)
  struct SpliceRun
  {
    uint32_t piece, srcEntry, dstEntry, count;
  };
  // the copy kernel's work item: up to this many blocks of one run, one wave's work (long runs spread over many waves and workgroups)
  constexpr uint32_t kSpliceItemBlocks = 64;

  inline uint64_t splice_blocks(uint64_t size) { return (size + 7u) / 8u; }

  // One axis of the edge rule.  size / srcSize: the output's and the source's extent in pixels; src, dst, n: the piece's first source block, first output block and
  // block count on this axis (inside both grids already).  An output block the output size clips takes the source's own last block, clipped to the same extent;
  // a whole output block takes a whole source block.
  inline bool splice_edge_ok(uint64_t size, uint64_t srcSize, uint64_t src, uint64_t dst, uint64_t n)
  {
    const bool dstLast = dst + n == splice_blocks(size), srcLast = src + n == splice_blocks(srcSize);
    if (dstLast && size % 8u != 0) return srcLast && srcSize % 8u == size % 8u;
    return !(srcLast && srcSize % 8u != 0);
  }

  // The rules of the call that need no stream: sizes, every piece inside its source and the output, the edge rule, and the exact cover.  true: `runs` holds the
  // pieces' block rows in the output's raster order (work and memory proportional to the runs, never to the blocks).  false: a rule is broken; `runs` is unspecified.
  // The caller has bounded sizeX, sizeY and the source sizes so that a block count fits 32 bits (limg_hip_stream_bound).
  inline bool splice_plan(const SplicePiece *pieces, size_t count, uint64_t sizeX, uint64_t sizeY, std::vector<SpliceRun> &runs)
  {
    runs.clear();
    if (!pieces || count == 0 || sizeX == 0 || sizeY == 0) return false;
    const uint64_t blocksX = splice_blocks(sizeX), blocksY = splice_blocks(sizeY), nBlocks = blocksX * blocksY;
    if (blocksX > 0xFFFFFFFFull || blocksY > 0xFFFFFFFFull || nBlocks > 0xFFFFFFFFull || count > nBlocks) return false; // (every piece holds a block at least)
    uint64_t area = 0, rows = 0;
    for (size_t i = 0; i < count; i++)
    {
      const SplicePiece &p = pieces[i];
      if (p.blocksW == 0 || p.blocksH == 0 || p.srcSizeX == 0 || p.srcSizeY == 0) return false;
      const uint64_t sbx = splice_blocks(p.srcSizeX), sby = splice_blocks(p.srcSizeY);
      if (sbx * sby > 0xFFFFFFFFull) return false;
      if ((uint64_t)p.srcBx + p.blocksW > sbx || (uint64_t)p.srcBy + p.blocksH > sby) return false;       // inside its source
      if ((uint64_t)p.dstBx + p.blocksW > blocksX || (uint64_t)p.dstBy + p.blocksH > blocksY) return false; // inside the output
      if (!splice_edge_ok(sizeX, p.srcSizeX, p.srcBx, p.dstBx, p.blocksW) || !splice_edge_ok(sizeY, p.srcSizeY, p.srcBy, p.dstBy, p.blocksH)) return false;
      area += (uint64_t)p.blocksW * p.blocksH;
      rows += p.blocksH;
      if (area > nBlocks) return false; // an overlap for certain: nothing is expanded (rows <= area)
    }
    if (area != nBlocks) return false; // a gap (or an overlap) for certain
    runs.reserve((size_t)rows);
    for (size_t i = 0; i < count; i++)
    {
      const SplicePiece &p = pieces[i];
      const uint64_t sbx = splice_blocks(p.srcSizeX);
      for (uint32_t r = 0; r < p.blocksH; r++)
        runs.push_back({ (uint32_t)i, (uint32_t)(((uint64_t)p.srcBy + r) * sbx + p.srcBx), (uint32_t)(((uint64_t)p.dstBy + r) * blocksX + p.dstBx), p.blocksW });
    }
    std::sort(runs.begin(), runs.end(), [](const SpliceRun &a, const SpliceRun &b) { return a.dstEntry != b.dstEntry ? a.dstEntry < b.dstEntry : a.piece < b.piece; });
    // exact cover: a run lies inside one block row, so runs that abut in raster order from entry 0 to the last start every row at 0 and end it at blocksX
    uint64_t next = 0;
    for (const SpliceRun &r : runs)
    {
      if (r.dstEntry != next) return false; // below: an overlap; above: a gap
      next += r.count;
    }
    return next == nBlocks;
  }

  // the copy kernel's items: itemBase[i] = the first item of run i, itemBase[runs] = their number (0: more than 32 bits hold)
  inline uint32_t splice_items(const std::vector<SpliceRun> &runs, uint32_t *itemBase)
  {
    uint64_t at = 0;
    for (size_t i = 0; i < runs.size(); i++)
    {
      itemBase[i] = (uint32_t)at;
      at += (runs[i].count + kSpliceItemBlocks - 1u) / kSpliceItemBlocks;
    }
    if (at > 0xFFFFFFFFull) return 0;
    itemBase[runs.size()] = (uint32_t)at;
    return (uint32_t)at;
  }
}

#endif
