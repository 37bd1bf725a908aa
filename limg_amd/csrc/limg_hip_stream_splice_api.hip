// limg_hip_stream_splice_api.hip -- the splice entries of the C ABI (limg_hip_stream_splice*, limg_hip_stream_crop*; kernels: limg_hip_stream_splice.hip): a version 1
// stream from rectangles of blocks of version 1 streams.  Every rule about the pieces is decided here, through limg_hip_splice_plan.h, before anything is launched;
// what only the streams' bytes can tell (headers, payload offsets) the kernels check.  The crop entries are the splice entry with one piece.
// No kernel lives here.
#include "limg_hip_context.h"
#include "limg_hip_splice_plan.h"

#include <new>

using namespace limg_hip;

namespace
{
  size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

  // the caller's pieces (pieceSize apart) as the struct this build knows
  limg_hip_result read_pieces(const limg_hip_splice_piece *pPieces, size_t count, size_t pieceSize, std::vector<limg_hip_splice_piece> &pieces)
  {
    if (pieceSize < sizeof(limg_hip_splice_piece) || count == 0 || count > 0xFFFFFFFFull) return limg_hip_error_InvalidParameter;
    pieces.resize(count);
    for (size_t i = 0; i < count; i++) memcpy(&pieces[i], (const uint8_t *)pPieces + i * pieceSize, sizeof(limg_hip_splice_piece));
    for (const limg_hip_splice_piece &p : pieces)
      if (!p.pStream) return limg_hip_error_ArgumentNull;
    return limg_hip_success;
  }

  // Every rule that needs no device: the sizes, each source's extent, and the plan's geometry (inside, edge rule, exact cover) -> the runs.
  // deviceForm: the pointers are the kernels' own, so alignment, capacity and aliasing count as well.
  limg_hip_result check_pieces(const std::vector<limg_hip_splice_piece> &pieces, size_t sizeX, size_t sizeY, bool deviceForm, const uint8_t *pOut, size_t capacity,
                               std::vector<SpliceRun> &runs)
  {
    const size_t bound = limg_hip_stream_bound(sizeX, sizeY);
    if (bound == 0) return limg_hip_error_InvalidParameter;
    if (deviceForm && (capacity < bound || ((uintptr_t)pOut & 15u) != 0)) return limg_hip_error_InvalidParameter;
    std::vector<SplicePiece> geometry(pieces.size());
    for (size_t i = 0; i < pieces.size(); i++)
    {
      const limg_hip_splice_piece &p = pieces[i];
      if (limg_hip_stream_bound(p.srcSizeX, p.srcSizeY) == 0) return limg_hip_error_InvalidParameter;
      const size_t table = sizeof(limg_hip_stream_header) + (size_t)(splice_blocks(p.srcSizeX) * splice_blocks(p.srcSizeY)) * sizeof(limg_hip_stream_block);
      if (p.streamBytes < table) return limg_hip_error_InvalidParameter;
      if (deviceForm)
      {
        if (((uintptr_t)p.pStream & 15u) != 0) return limg_hip_error_InvalidParameter;
        const uintptr_t a = (uintptr_t)p.pStream, b = (uintptr_t)pOut;
        if (a < b + capacity && b < a + p.streamBytes) return limg_hip_error_InvalidParameter; // the output would overwrite a source while it is read
      }
      geometry[i] = { p.srcSizeX, p.srcSizeY, p.srcBx, p.srcBy, p.dstBx, p.dstBy, p.blocksW, p.blocksH };
    }
    return splice_plan(geometry.data(), geometry.size(), sizeX, sizeY, runs) ? limg_hip_success : limg_hip_error_InvalidParameter;
  }

  // the checked call on the device: the tables in one upload, the three launches.  pieces[i].pStream: device memory
  limg_hip_result splice_launch(limg_hip_context *c, const std::vector<limg_hip_splice_piece> &pieces, const std::vector<SpliceRun> &runs, size_t sizeX, size_t sizeY, int hasAlpha,
                                uint32_t errorFactor, uint32_t flags, uint8_t *dOut, hipStream_t s)
  {
    const size_t nRuns = runs.size(), nPieces = pieces.size();
    // [fail word | sources | runs | itemBase | totals]: built on the host, zero where the kernels expect zero
    const size_t oSources = 16, oRuns = align16(oSources + nPieces * sizeof(SpliceSource)), oItems = align16(oRuns + nRuns * sizeof(SpliceRun));
    const size_t oTotals = align16(oItems + (nRuns + 1) * 4), total = align16(oTotals + (nRuns + 1) * 4);
    HIP_TRY(hipSetDevice(c->device));
    limg_hip_result r;
    limg_hip_context::Streams &st = c->stream;
    if (st.spliceBusy)
    { // the call before this one: its copy has left the pinned table and its kernels are done with the device copy
      HIP_TRY(hipEventSynchronize(st.spliceDone));
      st.spliceBusy = false;
    }
    if ((r = st.spliceDone.ensure(hipEventDisableTiming)) != limg_hip_success) return r;
    if ((r = ensure_stream_status(c, s)) != limg_hip_success) return r;
    if ((r = st.spliceHost.ensure(total)) != limg_hip_success) return r;
    if ((r = st.splice.ensure(total)) != limg_hip_success) return r;
    uint8_t *hb = (uint8_t *)st.spliceHost.p, *db = (uint8_t *)st.splice.p;
    memset(hb, 0, total);
    SpliceSource *sources = (SpliceSource *)(hb + oSources);
    for (size_t i = 0; i < nPieces; i++)
    {
      const limg_hip_splice_piece &p = pieces[i];
      sources[i].stream = p.pStream; sources[i].streamBytes = p.streamBytes;
      sources[i].sizeX = p.srcSizeX; sources[i].sizeY = p.srcSizeY;
      sources[i].blocksX = (uint32_t)splice_blocks(p.srcSizeX); sources[i].blocksY = (uint32_t)splice_blocks(p.srcSizeY);
      sources[i].nBlocks = sources[i].blocksX * sources[i].blocksY;
    }
    memcpy(hb + oRuns, runs.data(), nRuns * sizeof(SpliceRun));
    const uint32_t nItems = splice_items(runs, (uint32_t *)(hb + oItems));
    if (nItems == 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipMemcpyAsync(db, hb, total, hipMemcpyHostToDevice, s));
    st.spliceBusy = true; // from here on the table is in flight, whatever fails below
    SpliceParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.sources = (const SpliceSource *)(db + oSources); sp.runs = (const SpliceRun *)(db + oRuns); sp.itemBase = (const uint32_t *)(db + oItems);
    sp.totals = (uint32_t *)(db + oTotals); sp.fail = (uint32_t *)db; sp.status = (uint32_t *)c->stream.status.p; sp.out = dOut;
    sp.nRuns = (uint32_t)nRuns; sp.nItems = nItems;
    sp.sizeX = (uint32_t)sizeX; sp.sizeY = (uint32_t)sizeY; sp.blocksX = (uint32_t)splice_blocks(sizeX); sp.blocksY = (uint32_t)splice_blocks(sizeY);
    sp.nBlocks = sp.blocksX * sp.blocksY; sp.channels = hasAlpha ? 4u : 3u; sp.errorFactor = errorFactor; sp.flags = flags;
    launch_stream_splice(sp, device_cus(c), s);
    const hipError_t launched = hipGetLastError();
    HIP_TRY(hipEventRecord(st.spliceDone, s));
    HIP_TRY(launched);
    return limg_hip_success;
  }

  limg_hip_result splice_device(limg_hip_context *c, const limg_hip_splice_piece *pPieces, size_t count, size_t pieceSize, size_t sizeX, size_t sizeY, int hasAlpha,
                                uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes, hipStream_t s)
  {
    if (!c || !pPieces || !pOut) return limg_hip_error_ArgumentNull;
    std::vector<limg_hip_splice_piece> pieces;
    std::vector<SpliceRun> runs;
    limg_hip_result r;
    if ((r = read_pieces(pPieces, count, pieceSize, pieces)) != limg_hip_success) return r;
    if ((r = check_pieces(pieces, sizeX, sizeY, true, pOut, capacity, runs)) != limg_hip_success) return r;
    if ((r = splice_launch(c, pieces, runs, sizeX, sizeY, hasAlpha, errorFactor, flags, pOut, s)) != limg_hip_success) return r;
    return pBytes ? stream_total_bytes(pOut, s, pBytes) : limg_hip_success;
  }

  // host pointers: every distinct source up once, the device form's launches on the null stream, the status, the finished stream down
  limg_hip_result splice_host(limg_hip_context *c, const limg_hip_splice_piece *pPieces, size_t count, size_t pieceSize, size_t sizeX, size_t sizeY, int hasAlpha,
                              uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes)
  {
    if (!c || !pPieces || !pOut || !pBytes) return limg_hip_error_ArgumentNull;
    std::lock_guard<std::recursive_mutex> hostLock(c->hostEntry);
    std::vector<limg_hip_splice_piece> pieces;
    std::vector<SpliceRun> runs;
    limg_hip_result r;
    if ((r = read_pieces(pPieces, count, pieceSize, pieces)) != limg_hip_success) return r;
    if ((r = check_pieces(pieces, sizeX, sizeY, false, pOut, capacity, runs)) != limg_hip_success) return r;
    // the distinct sources (same pointer, same size), each at a 16-byte boundary of the staging buffer
    std::vector<size_t> order(count), offset(count);
    for (size_t i = 0; i < count; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      if (pieces[a].pStream != pieces[b].pStream) return (uintptr_t)pieces[a].pStream < (uintptr_t)pieces[b].pStream;
      return pieces[a].streamBytes != pieces[b].streamBytes ? pieces[a].streamBytes < pieces[b].streamBytes : a < b;
    });
    size_t staged = 0;
    for (size_t k = 0; k < count; k++)
    {
      const limg_hip_splice_piece &p = pieces[order[k]];
      if (k > 0 && p.pStream == pieces[order[k - 1]].pStream && p.streamBytes == pieces[order[k - 1]].streamBytes) { offset[order[k]] = offset[order[k - 1]]; continue; }
      size_t total = 0;
      if ((r = limg_hip_stream_info(p.pStream, p.streamBytes, nullptr, nullptr, nullptr, &total)) != limg_hip_success) return r;
      if (total > p.streamBytes) return limg_hip_error_OutOfBounds;
      offset[order[k]] = staged;
      staged += align16(p.streamBytes);
    }
    HIP_TRY(hipSetDevice(c->device));
    if ((r = c->host.in.ensure(staged + 16)) != limg_hip_success) return r;
    if ((r = c->stream.buf.ensure(limg_hip_stream_bound(sizeX, sizeY))) != limg_hip_success) return r;
    for (size_t k = 0; k < count; k++)
    {
      limg_hip_splice_piece &p = pieces[order[k]];
      uint8_t *d = (uint8_t *)c->host.in.p + offset[order[k]];
      if (k == 0 || offset[order[k]] != offset[order[k - 1]]) HIP_TRY(hipMemcpy(d, p.pStream, p.streamBytes, hipMemcpyHostToDevice));
      p.pStream = d;
    }
    if ((r = splice_launch(c, pieces, runs, sizeX, sizeY, hasAlpha, errorFactor, flags, (uint8_t *)c->stream.buf.p, nullptr)) != limg_hip_success) return r;
    *pBytes = 0;
    if ((r = limg_hip_check_device_status(c)) != limg_hip_success) return r; // a refused source: nothing reaches pOut
    size_t bytes = 0;
    if ((r = stream_total_bytes((const uint8_t *)c->stream.buf.p, nullptr, &bytes)) != limg_hip_success) return r;
    return download_stream(c, bytes, pOut, capacity, pBytes);
  }

  // a pixel window as one piece; false: not a window the blocks can be copied for
  bool crop_piece(const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, size_t x0, size_t y0, size_t width, size_t height, limg_hip_splice_piece &p)
  {
    if (limg_hip_stream_bound(sizeX, sizeY) == 0 || width == 0 || height == 0 || x0 >= sizeX || width > sizeX - x0 || y0 >= sizeY || height > sizeY - y0) return false;
    if (x0 % 8 != 0 || y0 % 8 != 0 || ((x0 + width) % 8 != 0 && x0 + width != sizeX) || ((y0 + height) % 8 != 0 && y0 + height != sizeY)) return false;
    p = { pStream, streamBytes, (uint32_t)sizeX, (uint32_t)sizeY, (uint32_t)(x0 / 8), (uint32_t)(y0 / 8), 0u, 0u, (uint32_t)splice_blocks(width), (uint32_t)splice_blocks(height) };
    return true;
  }
}

extern "C"
{
  limg_hip_result limg_hip_stream_splice_device(limg_hip_context *c, const limg_hip_splice_piece *pPieces, size_t count, size_t pieceSize, size_t sizeX, size_t sizeY, int hasAlpha,
                                                uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes, void *stream)
  {
    try { return splice_device(c, pPieces, count, pieceSize, sizeX, sizeY, hasAlpha, errorFactor, flags, pOut, capacity, pBytes, (hipStream_t)stream); }
    catch (const std::bad_alloc &) { return limg_hip_error_MemoryAllocationFailure; }
  }

  limg_hip_result limg_hip_stream_splice(limg_hip_context *c, const limg_hip_splice_piece *pPieces, size_t count, size_t pieceSize, size_t sizeX, size_t sizeY, int hasAlpha,
                                         uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes)
  {
    try { return splice_host(c, pPieces, count, pieceSize, sizeX, sizeY, hasAlpha, errorFactor, flags, pOut, capacity, pBytes); }
    catch (const std::bad_alloc &) { return limg_hip_error_MemoryAllocationFailure; }
  }

  limg_hip_result limg_hip_stream_crop_device(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t sizeX, size_t sizeY, int hasAlpha, size_t x0, size_t y0,
                                              size_t width, size_t height, uint32_t errorFactor, uint32_t flags, uint8_t *pOut, size_t capacity, size_t *pBytes, void *stream)
  {
    if (!c || !pStream || !pOut) return limg_hip_error_ArgumentNull;
    limg_hip_splice_piece piece;
    if (!crop_piece(pStream, streamBytes, sizeX, sizeY, x0, y0, width, height, piece)) return limg_hip_error_InvalidParameter;
    return limg_hip_stream_splice_device(c, &piece, 1, sizeof(piece), width, height, hasAlpha, errorFactor, flags, pOut, capacity, pBytes, stream);
  }

  limg_hip_result limg_hip_stream_crop(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, size_t x0, size_t y0, size_t width, size_t height, uint8_t *pOut,
                                       size_t capacity, size_t *pBytes)
  {
    if (!c || !pStream || !pOut || !pBytes) return limg_hip_error_ArgumentNull;
    size_t sizeX = 0, sizeY = 0;
    int hasAlpha = 0;
    const limg_hip_result r = limg_hip_stream_info(pStream, streamBytes, &sizeX, &sizeY, &hasAlpha, nullptr);
    if (r != limg_hip_success) return r;
    limg_hip_stream_header h;
    memcpy(&h, pStream, sizeof(h));
    limg_hip_splice_piece piece;
    if (!crop_piece(pStream, streamBytes, sizeX, sizeY, x0, y0, width, height, piece)) return limg_hip_error_InvalidParameter;
    return limg_hip_stream_splice(c, &piece, 1, sizeof(piece), width, height, hasAlpha, h.errorFactor, h.flags, pOut, capacity, pBytes);
  }
}
