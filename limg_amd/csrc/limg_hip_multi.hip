// limg_hip_multi.hip -- multi-GPU: RCCL behind the C ABI: the communicator, the variable-size gather of compact streams, and the 8x8 encode
// whose one dither chain runs through the strips of all ranks.
#include "limg_hip_context.h"

using namespace limg_hip;

#define NCCL_TRY(expr)                                                                                                    \
  do                                                                                                                      \
  {                                                                                                                       \
    const ncclResult_t e_ = (expr);                                                                                       \
    if (e_ != ncclSuccess)                                                                                                \
    {                                                                                                                     \
      fprintf(stderr, "limg_hip: %s failed: %s (%s:%d)\n", #expr, rccl().GetErrorString(e_), __FILE__, __LINE__);        \
      return limg_hip_error_Generic;                                                                                      \
    }                                                                                                                     \
  } while (0)

extern "C"
{
  limg_hip_result limg_hip_comm_unique_id(uint8_t *pId)
  {
    if (!pId) return limg_hip_error_ArgumentNull;
    static_assert(sizeof(ncclUniqueId) == LIMG_HIP_COMM_ID_BYTES, "ncclUniqueId size");
    if (!rccl().ok) return limg_hip_error_Generic;
    ncclUniqueId id;
    NCCL_TRY(rccl().GetUniqueId(&id));
    memcpy(pId, &id, sizeof(id));
    return limg_hip_success;
  }

  limg_hip_result limg_hip_comm_init(limg_hip_context *c, const uint8_t *pId, int rank, int worldSize)
  {
    if (!c || !pId) return limg_hip_error_ArgumentNull;
    if (worldSize < 1 || rank < 0 || rank >= worldSize || c->chain.comm) return limg_hip_error_InvalidParameter;
    if (!rccl().ok) return limg_hip_error_Generic;
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, pId, sizeof(id));
    NCCL_TRY(rccl().CommInitRank(&c->chain.comm, worldSize, id, rank));
    c->chain.rank = rank; c->chain.world = worldSize;
    limg_hip_result r2 = c->chain.words.ensure((8 + 2 * (size_t)worldSize) * 8); // [0] own value, [1] chain base, [2..3] own (size, capacity), [8 ...] gathered
    if (r2 != limg_hip_success) return r2;
    // the sticky status words (look-back timeout, aborted chain) exist from here on: the single-chain entry must not have to allocate on its error path.  On the
    // null stream, in front of the blocking memset: both are done when this returns
    if ((r2 = ensure_device_status(c, nullptr)) != limg_hip_success) return r2;
    HIP_TRY(hipMemset(c->chain.words.p, 0, (8 + 2 * (size_t)worldSize) * 8));
    return limg_hip_success;
  }

  // What RCCL itself says about the context's communicator: ncclCommCount / ncclCommUserRank / ncclGetVersion.  For bench lines and logs -- a record that names
  // the ranks RCCL saw cannot be produced by a job that silently ran on fewer.
  limg_hip_result limg_hip_comm_info(limg_hip_context *c, int *pRank, int *pRanks, int *pRcclVersion)
  {
    if (!c) return limg_hip_error_ArgumentNull;
    if (!c->chain.comm) return limg_hip_error_InvalidParameter;
    if (!rccl().ok || !rccl().CommCount || !rccl().CommUserRank || !rccl().GetVersion) return limg_hip_error_Generic;
    int v = 0;
    if (pRanks) NCCL_TRY(rccl().CommCount(c->chain.comm, pRanks));
    if (pRank) NCCL_TRY(rccl().CommUserRank(c->chain.comm, pRank));
    if (pRcclVersion) { NCCL_TRY(rccl().GetVersion(&v)); *pRcclVersion = v; }
    return limg_hip_success;
  }

  limg_hip_result limg_hip_comm_destroy(limg_hip_context *c)
  {
    if (!c) return limg_hip_error_ArgumentNull;
    if (c->chain.comm)
    {
      HIP_TRY(hipSetDevice(c->device));
      HIP_TRY(hipDeviceSynchronize());
      NCCL_TRY(rccl().CommDestroy(c->chain.comm));
      c->chain.comm = nullptr; c->chain.rank = 0; c->chain.world = 1;
    }
    return limg_hip_success;
  }

  // Offsets of a variable-size gather: piece r starts at the sum of the earlier sizes, each rounded up to 16 bytes (the decoder wants 16-byte aligned streams).
  limg_hip_result limg_hip_host_gather_offsets(const uint64_t *pSizes, int count, uint64_t *pOffsets)
  {
    if (!pSizes || !pOffsets) return limg_hip_error_ArgumentNull;
    if (count < 1) return limg_hip_error_InvalidParameter;
    uint64_t off = 0;
    for (int r = 0; r < count; r++)
    {
      pOffsets[r] = off;
      off += (pSizes[r] + 15ull) & ~15ull;
    }
    pOffsets[count] = off;
    return limg_hip_success;
  }

  // Exclusive prefix of the per-rank dither-call totals = every rank's first call index in the one chain that runs through all strips (rank order = strip order).
  limg_hip_result limg_hip_host_chain_bases(const uint64_t *pCalls, int count, uint64_t *pBases)
  {
    if (!pCalls || !pBases) return limg_hip_error_ArgumentNull;
    if (count < 1) return limg_hip_error_InvalidParameter;
    uint64_t run = 0;
    for (int r = 0; r < count; r++) { pBases[r] = run; run += pCalls[r]; }
    return limg_hip_success;
  }

  limg_hip_result limg_hip_gather_stream(limg_hip_context *c, const uint8_t *pStream, size_t streamBytes, int root, uint8_t *pGathered, size_t capacity, uint64_t *pOffsets,
                                         void *stream)
  {
    if (!c || !pStream) return limg_hip_error_ArgumentNull;
    if (!c->chain.comm) return limg_hip_error_InvalidParameter;
    if (root < 0 || root >= c->chain.world) return limg_hip_error_InvalidParameter;
    const bool isRoot = c->chain.rank == root;
    if (isRoot && (!pGathered || !pOffsets)) return limg_hip_error_ArgumentNull;
    if (isRoot && ((uintptr_t)pGathered & 15u) != 0) return limg_hip_error_InvalidParameter;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int world = c->chain.world;
    unsigned long long *words = (unsigned long long *)c->chain.words.p;
    // 1. every rank learns every size AND the root's capacity: one 16-byte all-gather.  Whether the pieces fit is then decided by every rank from the same
    //    numbers -- a root that alone found its buffer too small would leave its peers' sends unmatched
    const unsigned long long mine[2] = { (unsigned long long)streamBytes, isRoot ? (unsigned long long)capacity : 0ull };
    HIP_TRY(hipMemcpyAsync(words + 2, mine, 16, hipMemcpyHostToDevice, s));
    NCCL_TRY(rccl().AllGather(words + 2, words + 8, 2, ncclUint64, c->chain.comm, s));
    std::vector<uint64_t> pairs(2 * (size_t)world), sizes(world), offs(world + 1);
    HIP_TRY(hipMemcpyAsync(pairs.data(), words + 8, (size_t)world * 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int r = 0; r < world; r++) sizes[r] = pairs[2 * (size_t)r];
    limg_hip_host_gather_offsets(sizes.data(), world, offs.data());
    if (offs[world] > pairs[2 * (size_t)root + 1]) return limg_hip_error_OutOfBounds; // on EVERY rank: nothing is posted anywhere
    // 2. exactly the used bytes, point to point: each peer -> root transfer rides one xGMI link
    NCCL_TRY(rccl().GroupStart());
    ncclResult_t posted = ncclSuccess; // a failed post must not leave the group open: close it first, report afterwards
    if (isRoot)
    {
      for (int r = 0; r < world && posted == ncclSuccess; r++)
        if (r != root && sizes[r]) posted = rccl().Recv(pGathered + offs[r], sizes[r], ncclUint8, r, c->chain.comm, s);
    }
    else if (streamBytes)
      posted = rccl().Send(pStream, streamBytes, ncclUint8, root, c->chain.comm, s);
    const ncclResult_t closed = rccl().GroupEnd();
    NCCL_TRY(posted);
    NCCL_TRY(closed);
    if (isRoot)
    {
      if (streamBytes) HIP_TRY(hipMemcpyAsync(pGathered + offs[root], pStream, streamBytes, hipMemcpyDeviceToDevice, s));
      memcpy(pOffsets, offs.data(), (size_t)(world + 1) * 8);
      for (int r = 0; r < world; r++) pOffsets[r] = offs[r];
    }
    return limg_hip_success;
  }

  limg_hip_result limg_hip_encode3d_single_chain_device(limg_hip_context *c, const uint32_t *pIn, size_t sizeX, size_t stripRows, int hasAlpha, const limg_hip_encode3d_info *pInfo,
                                                        uint32_t errorFactor, int fastBitCrushing, size_t blocksBefore, void *stream)
  {
    if (!c) return limg_hip_error_ArgumentNull;
    if (!c->chain.comm) return limg_hip_error_InvalidParameter; // no communicator: nobody is waiting for this rank
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *words = (unsigned long long *)c->chain.words.p;
    limg_hip_result r;
    // E step + scan: this strip's dither calls land in words[0] ...  (bad arguments on this rank are a phase-1 failure like any other: see the abort rule)
    if (!pIn || !pInfo) r = limg_hip_error_ArgumentNull;
    else if (TOPT(c, fail_chain_phase1) != 0) r = limg_hip_error_Generic;
    else r = limg_hip_encode3d_chain_device(c, pIn, sizeX, stripRows, hasAlpha, pInfo, errorFactor, fastBitCrushing, 1, (uint64_t *)words, nullptr, blocksBefore, s);
    // Abort rule: a rank whose phase 1 failed must STILL join the exchange -- its peers are (about to be) inside ncclAllGather and would wait for it forever -- and
    // joins it with a poison value instead of a call count.  Every rank's k_chain_base then sees the poison: it hands the F step a poisoned base (k_dither_store
    // returns without storing anything) and raises the context's sticky status word, so that the peers' limg_hip_check_device_status reports the aborted chain;
    // this rank returns its own error.  (The reference's analogue -- row strips on a thread pool, src/limg.cpp:2114-2136 -- cannot half-fail.)
    const limg_hip_result phase1 = r;
    if (phase1 != limg_hip_success) HIP_TRY(hipMemsetAsync(words, 0xFF, 8, s));
    // ... one 8-byte all-gather, the exclusive prefix over the ranks before this one on the device (stream-ordered, no host round trip) ...
    NCCL_TRY(rccl().AllGather(words, words + 8, 1, ncclUint64, c->chain.comm, s));
    launch_chain_base(words + 8, c->chain.rank, c->chain.world, words + 1, (uint32_t *)c->enc.devStatus.p + 1, s);
    if (phase1 != limg_hip_success) return phase1;
    // ... and the F step indexes the noise stream from there: the 8-GPU result equals the single-threaded reference's (src/limg.cpp:1893, :2110)
    return limg_hip_encode3d_chain_device(c, pIn, sizeX, stripRows, hasAlpha, pInfo, errorFactor, fastBitCrushing, 2, nullptr, (const uint64_t *)(words + 1), blocksBefore, s);
  }
}
