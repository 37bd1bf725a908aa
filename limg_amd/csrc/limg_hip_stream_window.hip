// limg_hip_stream_window.hip -- window decode of the "LMG3" stream, both versions: any pixel rectangle of the image into a caller's stride (contract: include/limg_hip.h).
//
// The table gives every 8x8 block (version 1) or rectangle (version 2) its own payloadWord, so a window needs the entries and payload of its own block range
// bx0 .. bx0 + wbx - 1, by0 .. by0 + wby - 1 only.  What is read, stored and kept in context memory scales with that range -- except version 2's table scan.
//   k_stream_window_decode     version 1.  Persistent, lane = (block j = lane & 7, block row r = lane >> 3) over groups of 8 blocks like k_stream_decode, but the work
//                              unit is a run of up to 64 consecutive blocks of ONE block row of the window: raster-consecutive blocks are what the packer lays down
//                              back to back, so a group's payload is still one run that is validated as a run (offsets in 64 bits, inside the payload, no longer than
//                              8 x 24 words) and fetched by the whole wave; across window rows the runs are far apart.  The next group's run is requested before
//                              the current one is decoded.  A group that fails raises the status word and stores nothing.
//   k_bstream_window_map       version 2.  Scans the WHOLE rectangle table (64 B per rectangle), 64 rectangles per wave step: checks every rectangle's geometry, shifts
//                              and payload extent (rect_ok) and claims the blocks of rectangle n window block range in a window-sized block -> rectangle map
//                              (atomicCAS on ~0): a lane claims a small piece itself, the wave claims a large one together; the claimed blocks are counted.
//                              Overlaps wholly outside the window are therefore not seen.
//   k_bstream_window_decode    refuses unless every block of the window was claimed exactly once and nothing was flagged; then units of 8 consecutive blocks of a
//                              window block row: the lane's 8 pixels are the bit run at ((y - 8 oy) * wpx + (x - 8 ox)) * b of each field of the block's rectangle;
//                              a wave's stores are 8 row pieces of 256 contiguous bytes.  Nothing is read through an offset the map kernel has not checked against
//                              the stream's size.
// The full version 2 decode (limg_hip_blocked_decode_stream[_device]) is these two kernels on the window (0, 0, sizeX, sizeY) at stride sizeX: version 2 has no other decoder.
// Both versions decode with a16_constants / a16_pixel (limg_hip_stream_format.h): the reference's decoder in 32-bit terms, exact for every record (any int16 record, every shift triple and
// escape pattern: tests/test_gpu_synthetic_streams.py and tests/test_gpu_synthetic_blocked_streams.py, against the oracle's decode of hand-built streams).  Of the full version 1
// decoder's devices this file uses the next-run prefetch only: no counted wait (and so no store sink), no packed 16-bit decode, no per-block constants in LDS -- every
// lane prepares the constants of its block itself.
// Lanes whose image row or columns fall outside the window store nothing, or only the pixels inside it: nothing but the window's pixels is ever written.
//
// Batched forms (limg_hip_*decode_stream_windows*): many windows of many streams per launch.  The per-unit bodies of the kernels above are __device__ functions
// (window_unit, bwindow_unit, rect_ok, claim_pieces) that both forms call, so a job decodes exactly as its single-window call would.
//   k_stream_windows_decode    version 1.  One persistent launch over the concatenated unit list of all jobs; a wave finds its unit's job by a wave-uniform binary
//                              search over the exclusive prefix of unit counts and reads the job's WindowDecodeParams from the job table through scalar loads.
//   k_bstream_windows_map      version 2.  Work item = (stream group, 64 rectangles): every rectangle is checked ONCE per group and its intersection claimed in the
//                              map slice of every window of the group.  A bad rectangle or header refuses every job of the group, a clash the job it happened in.
//   k_bstream_windows_decode   one launch over the concatenated 8-block units; a unit reads its job's verdict first.
//
// Tensor forms (limg_hip_*decode_stream_windows_tensor*): the batched kernels with another store.  How a lane's 8 decoded pixels leave is a policy of window_unit and
// bwindow_unit: RgbaStore is the packed store of every kernel above; PlanarStore<T> (T = float / _Float16) writes byte c of each pixel as scale[c] * byte + bias[c]
// into plane c, `planes` planes.  k_stream_windows_tensor<T> and k_bstream_windows_tensor<T> are k_stream_windows_decode and k_bstream_windows_decode with it;
// k_bstream_windows_map never touches the output and serves both.  The format is a kernel argument: scale and bias stay in scalar registers.
//
// Scaled forms (limg_hip_*decode_stream_windows_scaled*): the batched kernels with ScaledStore<RgbaStore> / ScaledStore<PlanarStore<T>>, kernels of their own
// (k_stream_windows_scaled[_tensor<T>], k_bstream_windows_scaled[_tensor<T>]).  A job's level L rides in its WindowDecodeParams, whose window is then the SOURCE
// footprint: units, validation and the map kernel see a plain window; only the store differs -- k x k box sums inside the 8x8 block (in the lane along x, across
// the lanes 8, 16 and 32 away along y), rounded and stored by the lane of each box's first row.  Nothing is gathered across blocks (DESIGN.md says why).
//
// Resized forms (limg_hip_*decode_stream_windows_resized*): the one thing a store policy cannot do, a filter whose taps cross 8x8 blocks, as a kernel stage of its own.
// The work item is an output TILE of a job and belongs to a whole workgroup (k_stream_windows_resized[_tensor<T>], k_bstream_windows_resized[_tensor<T>]): its waves
// run the unit bodies above over the tile's level-L footprint with ScaledStore<TileStore> -- into an LDS tile instead of the output --, synchronise, and resample
// bilinearly from LDS by the contract's integer formula.  A second per-job table (ResizeJob) carries what WindowDecodeParams has no room for.
//
// Error forms (limg_hip_*decode_stream_windows_error*): the batched kernels with a policy that stores nothing.  ErrorSink reads the ORIGINAL's 8 pixels where RgbaStore
// would write the decoded ones (p.out / outStride / vecOut then describe the original; the loads are requested before the lane's decode arithmetic) and adds the
// reference's per-pixel colour error -- k_compare's integer sum (limg_hip_synth.hip) -- to the lane's 32-bit partial.  ErrorTotal, the bodies' second policy, reduces
// the partials once per unit into a wave-uniform 64-bit total and adds that to the job's sum with one device-scope atomic when the wave's job changes; where the
// waves' loops end, the four waves of a workgroup hand their totals to one thread through 48 bytes of LDS (ErrorEnd), which adds them with one atomic per job.  k_stream_windows_error / k_bstream_windows_error; k_bstream_windows_map serves them as it is.
#include "limg_hip_stream_format.h"

#include <type_traits>

namespace limg_hip
{
  namespace
  {
    constexpr int kEntry = 56;
    constexpr int kGroupBytes = 8 * 192; // payload of 8 blocks, worst case

    __device__ __forceinline__ uint32_t words_of(uint32_t bits) { return (bits & 0xFF) + ((bits >> 8) & 0xFF) + ((bits >> 16) & 0xFF); }

    // the lane's 8 pixels, columns x .. x + 7 of image row y, into the window: a piece wholly inside it as two 16-byte stores where the caller's buffer allows
    // them, else pixel by pixel; the caller has checked that y is a row of the window
    struct RgbaStore
    {
      __device__ __forceinline__ void operator()(const WindowDecodeParams &p, uint32_t x, uint32_t y, const uint32_t px[8]) const
      {
        uint32_t *row = p.out + (unsigned long long)(y - p.y0) * p.outStride;
        if (p.vecOut && x >= p.x0 && x + 8u <= p.x0 + p.width)
        {
          uint4 *dst = reinterpret_cast<uint4 *>(row + (x - p.x0));
          dst[0] = make_uint4(px[0], px[1], px[2], px[3]);
          dst[1] = make_uint4(px[4], px[5], px[6], px[7]);
          return;
        }
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
          if (x + i >= p.x0 && x + i < p.x0 + p.width) row[x + i - p.x0] = px[i];
      }
    };

    // The same 8 pixels into planes of T: plane c gets byte c of every pixel as (float)byte * scale[c] + bias[c] -- a multiply, then an add, each rounded on its own
    // (the library is built without contraction) -- as it is (float) or rounded to nearest even (_Float16).  The inside / edge rule is RgbaStore's; a piece wholly
    // inside leaves as 16 bytes per store, so the 8 lanes of a block row fill 256 (float, two stores) or 128 (_Float16, one) contiguous bytes of a plane row.
    // The packed pixels are made opaque first: the compiler otherwise sees through the packing, keeps the 8 x 4 channel values of a16_pixel apart instead of the
    // 8 pixels and needs 155 vector registers in version 1's kernel where the RGBA kernel has 99 -- a wave per SIMD less.  f: the call's format, wave-uniform.
    typedef float float4v __attribute__((ext_vector_type(4)));
    typedef _Float16 half8v __attribute__((ext_vector_type(8)));
    template <class T>
    struct PlanarStore
    {
      limg_hip_tensor_format f;
      __device__ __forceinline__ void operator()(const WindowDecodeParams &p, uint32_t x, uint32_t y, const uint32_t px[8]) const
      {
        T *row = reinterpret_cast<T *>(p.out) + (unsigned long long)(y - p.y0) * p.outStride;
        const bool whole = p.vecOut && x >= p.x0 && x + 8u <= p.x0 + p.width;
        uint32_t q[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
        {
          q[i] = px[i];
          asm volatile("" : "+v"(q[i]));
        }
#pragma unroll
        for (uint32_t c = 0; c < 4u; c++)
        {
          if (c >= f.planes) break; // (wave-uniform)
          float v[8];
#pragma unroll
          for (uint32_t i = 0; i < 8u; i++) v[i] = (float)((q[i] >> (8u * c)) & 0xFFu) * f.scale[c] + f.bias[c];
          T *plane = row + (unsigned long long)c * p.planeStride;
          if (whole)
          {
            if constexpr (sizeof(T) == 4)
            {
              float4v *dst = reinterpret_cast<float4v *>(plane + (x - p.x0));
              dst[0] = float4v{ v[0], v[1], v[2], v[3] };
              dst[1] = float4v{ v[4], v[5], v[6], v[7] };
            }
            else
              *reinterpret_cast<half8v *>(plane + (x - p.x0)) = half8v{ (T)v[0], (T)v[1], (T)v[2], (T)v[3], (T)v[4], (T)v[5], (T)v[6], (T)v[7] };
          }
          else
          {
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++)
              if (x + i >= p.x0 && x + i < p.x0 + p.width) plane[x + i - p.x0] = (T)v[i];
          }
        }
      }
    };

    // ---- the error forms: nothing is stored -----------------------------------------------------------------------------------------------
    // What the error bodies keep per wave.  lane: the lane's partial of the current unit -- 8 pixels are below 2^23 (12 x 255^2 x 8), the at most 8 rows a lane decodes
    // in a version 1 unit below 2^26 and a whole unit of 64 blocks below 2^32 (12 x 255^2 x 4096), so 32 bits hold every sum inside a unit.  total, job: the sum of
    // the units since the last flush and the job they belong to, wave-uniform (scalar registers).  alpha: the current job's header says 4 channels.
    // ErrorEnd: where the four waves of a workgroup leave what they hold when their loops end, so that one of them adds it to the sums.  Every atomic of a whole-image
    // call names one address, where they are served one after the other, and the waves' loops end together: left to each wave, thousands of them queue up behind the
    // kernel's last unit (profiles/stream_error.md).
    struct ErrorEnd { unsigned long long total[4]; uint32_t job[4]; };
    struct ErrorTotal
    {
      static constexpr bool kKeepsJob = true; // (version 2's body)
      unsigned long long *sums;
      ErrorEnd &end;
      uint32_t lane = 0, job = 0;
      unsigned long long total = 0;
      bool alpha = false;
      // one 64-bit device-scope atomic for all units of `job` since the last one
      __device__ __forceinline__ void flush()
      {
        if (total != 0ull && lane_id() == 0) atomicAdd(sums + job, total);
        total = 0ull;
      }
      __device__ __forceinline__ void begin_unit(uint32_t unitJob, uint32_t channels)
      {
        if (unitJob != job) flush(); // (wave-uniform)
        job = unitJob; alpha = channels == 4u;
      }
      // every lane is here (the unit bodies' branches have joined): the partials' sum within each row of 16 lanes through DPP, the four rows' through scalar reads
      __device__ __forceinline__ void end_unit()
      {
        uint32_t v = lane;
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm:[1,0,3,2] */, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /* quad_perm:[2,3,0,1] */, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141 /* row_half_mirror */, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140 /* row_mirror */, 0xF, 0xF, false);
        total += (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
                 (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
        lane = 0;
      }
      // the wave's loop has ended, and so will every other wave's of the workgroup (no wave leaves a body early): the four totals, those of one job added up, by
      // thread 0 with at most four atomics -- one where the workgroup ended inside one job
      __device__ __forceinline__ void finish()
      {
        const uint32_t wave = threadIdx.x >> 6;
        if (lane_id() == 0) { end.total[wave] = total; end.job[wave] = job; }
        __syncthreads();
        if (threadIdx.x == 0)
          for (uint32_t w = 0; w < 4u; w++)
          {
            unsigned long long t = end.total[w];
            if (t == 0ull) continue;
            for (uint32_t v = w + 1u; v < 4u; v++)
              if (end.job[v] == end.job[w]) { t += end.total[v]; end.total[v] = 0ull; }
            atomicAdd(sums + end.job[w], t);
          }
        total = 0ull;
      }
    };
    // the bodies' second policy for every kernel that stores: nothing to keep
    struct NoTotal
    {
      static constexpr bool kKeepsJob = false;
      __device__ __forceinline__ void begin_unit(uint32_t, uint32_t) const {}
      __device__ __forceinline__ void end_unit() const {}
      __device__ __forceinline__ void finish() const {}
    };

    // The original's 8 pixels beside the lane's decoded ones, columns x .. x + 7 of image row y; p.out is the ORIGINAL, read only, and the inside / edge rule is
    // RgbaStore's: a piece wholly inside the window arrives as two 16-byte loads where the original's pointer, stride and x0 allow them (vecOut), else pixel by pixel,
    // and only pixels inside the window are read or counted.
    struct ErrorSink
    {
      ErrorTotal &t;
      struct Loaded { uint32_t px[8]; uint32_t inside; }; // inside: bit i = pixel i lies in the window
      // requested before the lane's decode arithmetic, which then runs while the loads are in flight; the caller has checked that y is a row of the window
      __device__ __forceinline__ Loaded load(const WindowDecodeParams &p, uint32_t x, uint32_t y) const
      {
        Loaded o;
        const uint32_t *row = p.out + (unsigned long long)(y - p.y0) * p.outStride;
        if (p.vecOut && x >= p.x0 && x + 8u <= p.x0 + p.width)
        {
          const uint4 *src = reinterpret_cast<const uint4 *>(row + (x - p.x0));
          const uint4 a = src[0], b = src[1];
          o.px[0] = a.x; o.px[1] = a.y; o.px[2] = a.z; o.px[3] = a.w; o.px[4] = b.x; o.px[5] = b.y; o.px[6] = b.z; o.px[7] = b.w;
          o.inside = 0xFFu;
          return o;
        }
        o.inside = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
        {
          const bool in = x + i >= p.x0 && x + i < p.x0 + p.width;
          o.px[i] = in ? row[x + i - p.x0] : 0u;
          o.inside |= in ? 1u << i : 0u;
        }
        return o;
      }
      // k_compare's sum per pixel: red^2 x (2 | 3) + green^2 x 4 + blue^2 x (3 | 2) + alpha^2 x 3, the weights swapped where red^2 >= 0x4000, alpha in 4-channel streams only.
      // Two channels at a time: the even bytes (red, blue) and the odd bytes (green, alpha) of both pixels as pairs of 16-bit values, their differences and the
      // differences' squares (at most 255^2: 16 bits hold them) as packed 16-bit operations, each pair weighted and added by one dot product.  ALL: every pixel lies in
      // the window; else a pixel outside it is compared with itself.
      typedef short short2v __attribute__((ext_vector_type(2)));
      typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));
      template <bool ALL>
      __device__ __forceinline__ uint32_t row_error(const uint32_t dd[8], const Loaded &o) const
      {
        constexpr uint32_t kOdd = 0x0C030C01u; // v_perm_b32: bytes 1 and 3 into bytes 0 and 2, zeros between them
        const ushort2v wOdd = __builtin_bit_cast(ushort2v, t.alpha ? 0x00030004u : 0x00000004u); // (wave-uniform)
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
        {
          const uint32_t d = dd[i], q = ALL || ((o.inside >> i) & 1u) ? o.px[i] : d;
          const short2v even = __builtin_bit_cast(short2v, d & 0x00FF00FFu) - __builtin_bit_cast(short2v, q & 0x00FF00FFu);
          const short2v odd = __builtin_bit_cast(short2v, __builtin_amdgcn_perm(d, d, kOdd)) - __builtin_bit_cast(short2v, __builtin_amdgcn_perm(q, q, kOdd));
          const ushort2v sqEven = __builtin_bit_cast(ushort2v, even * even), sqOdd = __builtin_bit_cast(ushort2v, odd * odd);
          const bool low = (__builtin_bit_cast(uint32_t, sqEven) & 0xC000u) == 0u; // red^2 < 0x4000
          sum = __builtin_amdgcn_udot2(sqEven, __builtin_bit_cast(ushort2v, low ? 0x00030002u : 0x00020003u), sum, false);
          sum = __builtin_amdgcn_udot2(sqOdd, wOdd, sum, false);
        }
        return sum;
      }
      __device__ __forceinline__ void operator()(const WindowDecodeParams &, uint32_t, uint32_t, const uint32_t px[8], const Loaded &o) const
      {
        uint32_t dd[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
        {
          dd[i] = px[i];
          asm volatile("" : "+v"(dd[i])); // (the packed pixels, as in PlanarStore and for its reason)
        }
        t.lane += o.inside == 0xFFu ? row_error<true>(dd, o) : row_error<false>(dd, o);
      }
    };

    // What a unit body does around a lane's decode: before_decode where the lane knows its pixels' place, after_decode with the decoded pixels.  Every store policy has
    // nothing to do before and stores after; ErrorSink requests the original first.
    struct Nothing {};
    template <class STORE>
    __device__ __forceinline__ Nothing before_decode(const STORE &, const WindowDecodeParams &, uint32_t, uint32_t) { return Nothing(); }
    __device__ __forceinline__ ErrorSink::Loaded before_decode(const ErrorSink &s, const WindowDecodeParams &p, uint32_t x, uint32_t y) { return s.load(p, x, y); }
    template <class STORE>
    __device__ __forceinline__ void after_decode(const STORE &store, const WindowDecodeParams &p, uint32_t x, uint32_t y, const uint32_t px[8], const Nothing &) { store(p, x, y, px); }
    __device__ __forceinline__ void after_decode(const ErrorSink &s, const WindowDecodeParams &p, uint32_t x, uint32_t y, const uint32_t px[8], const ErrorSink::Loaded &o) { s(p, x, y, px, o); }

    // ---- reduced scale (the *_scaled entries): the job's level L, k = 1 << L -------------------------------------------------------------
    // p describes the job's source footprint, multiples of k; output pixel (X, Y) is the rounded mean of the k x k box at (k X, k Y), byte by byte.  A box never leaves
    // its 8x8 block: its columns are k of the lane's 8 pixels, its rows the same pixels of the lanes 8, 16 and 32 away (lane = block j + 8 * row).  Two bytes of a
    // pixel travel per dword (bytes 0 / 2 in lo, 1 / 3 in hi): the largest sum, 64 * 255 + 32, fits in 16 bits.
    // Lanes that exchange sums belong to one block and one row of boxes.  Which lanes reach a store is decided per block (its place in the unit and in the window's
    // columns, its group's verdict) and per image row against the footprint's rows, which are whole boxes: such lanes are inside or outside together, so no read
    // below names a lane that is not here.
    // The partners: lane ^ 8 through DPP row_ror:8 (a rotation by 8 within the row of 16 lanes; it folds into the add: one instruction per dword), lane ^ 16 through
    // __shfl_xor (ds_bpermute_b32, one address for all dwords), lane ^ 32 through v_permlane32_swap of the dword with a copy of itself: one half of each result
    // register is the lane's own sum, the other the partner's (2 instructions per dword where __shfl_xor takes a ds_bpermute_b32, its wait and the add).
    __device__ __forceinline__ uint32_t add_lane_xor8(uint32_t v) { return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /* row_ror:8 */, 0xF, 0xF, false); }
    __device__ __forceinline__ uint32_t add_lane_xor16(uint32_t v) { return v + (uint32_t)__shfl_xor((int)v, 16, 64); }
    __device__ __forceinline__ uint32_t add_lane_xor32(uint32_t v)
    {
      const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
      return (uint32_t)r[0] + (uint32_t)r[1];
    }

    // N = 8 >> L reduced pixels of output row Y, columns X .. X + N - 1, into the window.  Store width: a piece of exactly 16 bytes (level 1, RGBA8 and float) that lies
    // wholly inside the window leaves as one 16-byte store where vecOut allows it (X is a multiple of 4 there); every other piece element by element.
    template <uint32_t L>
    __device__ __forceinline__ void store_reduced(const RgbaStore &, const WindowDecodeParams &p, uint32_t X, uint32_t Y, const uint32_t (&q)[8u >> L])
    {
      constexpr uint32_t N = 8u >> L;
      const uint32_t X0 = p.x0 >> L, W = p.width >> L;
      uint32_t *row = p.out + (unsigned long long)(Y - (p.y0 >> L)) * p.outStride;
      if constexpr (N == 4u)
        if (p.vecOut && X >= X0 && X + 4u <= X0 + W)
        {
          *reinterpret_cast<uint4 *>(row + (X - X0)) = make_uint4(q[0], q[1], q[2], q[3]);
          return;
        }
#pragma unroll
      for (uint32_t i = 0; i < N; i++)
        if (X + i >= X0 && X + i < X0 + W) row[X + i - X0] = q[i];
    }

    template <uint32_t L, class T>
    __device__ __forceinline__ void store_reduced(const PlanarStore<T> &s, const WindowDecodeParams &p, uint32_t X, uint32_t Y, const uint32_t (&q)[8u >> L])
    {
      constexpr uint32_t N = 8u >> L;
      const uint32_t X0 = p.x0 >> L, W = p.width >> L;
      T *row = reinterpret_cast<T *>(p.out) + (unsigned long long)(Y - (p.y0 >> L)) * p.outStride;
      const bool whole = N == 4u && sizeof(T) == 4 && p.vecOut && X >= X0 && X + 4u <= X0 + W;
#pragma unroll
      for (uint32_t c = 0; c < 4u; c++)
      {
        if (c >= s.f.planes) break; // (wave-uniform)
        float v[N];
#pragma unroll
        for (uint32_t i = 0; i < N; i++) v[i] = (float)((q[i] >> (8u * c)) & 0xFFu) * s.f.scale[c] + s.f.bias[c];
        T *plane = row + (unsigned long long)c * p.planeStride;
        if constexpr (N == 4u && sizeof(T) == 4)
          if (whole)
          {
            *reinterpret_cast<float4v *>(plane + (X - X0)) = float4v{ v[0], v[1], v[2], v[3] };
            continue;
          }
#pragma unroll
        for (uint32_t i = 0; i < N; i++)
          if (X + i >= X0 && X + i < X0 + W) plane[X + i - X0] = (T)v[i];
      }
    }

    // The resized entries' base policy: level-L pixels into the workgroup's LDS tile, which holds the level pixels fx0 .. fx0 + fw - 1 of the level rows fy0 .. fy0 + fh - 1
    // at pitch fw.  Pixels outside the tile are dropped (X - fx0 wraps to a large value left of it); the level-0 operator does the same for the lane's 8 pixels.
    struct TileStore
    {
      uint32_t *tile;
      uint32_t fx0, fy0, fw, fh;
      __device__ __forceinline__ void put(uint32_t X, uint32_t Y, uint32_t v) const
      {
        if (X - fx0 < fw && Y - fy0 < fh) tile[(Y - fy0) * fw + (X - fx0)] = v;
      }
      __device__ __forceinline__ void operator()(const WindowDecodeParams &, uint32_t x, uint32_t y, const uint32_t px[8]) const
      {
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) put(x + i, y, px[i]);
      }
    };

    template <uint32_t L>
    __device__ __forceinline__ void store_reduced(const TileStore &s, const WindowDecodeParams &, uint32_t X, uint32_t Y, const uint32_t (&q)[8u >> L])
    {
#pragma unroll
      for (uint32_t i = 0; i < (8u >> L); i++) s.put(X + i, Y, q[i]);
    }

    // the lane's 8 pixels of image row y -> its share of the sums of 8 >> L boxes; after the exchange every lane of a box row holds the whole sums, and the lane of
    // the box's first row rounds (half up) and stores.  The pixels are made opaque first, as in PlanarStore and for its reason.
    template <uint32_t L, class BASE>
    __device__ __forceinline__ void reduce_and_store(const BASE &base, const WindowDecodeParams &p, uint32_t x, uint32_t y, const uint32_t px[8])
    {
      constexpr uint32_t k = 1u << L, N = 8u >> L, kHalf = ((k * k) >> 1) * 0x00010001u;
      uint32_t lo[N], hi[N];
#pragma unroll
      for (uint32_t i = 0; i < N; i++)
      {
        lo[i] = 0; hi[i] = 0;
#pragma unroll
        for (uint32_t j = 0; j < k; j++)
        {
          const uint32_t v = px[i * k + j];
          lo[i] += v & 0x00FF00FFu; hi[i] += (v >> 8) & 0x00FF00FFu;
        }
      }
#pragma unroll
      for (uint32_t i = 0; i < N; i++)
      {
        lo[i] = add_lane_xor8(lo[i]); hi[i] = add_lane_xor8(hi[i]);
        if constexpr (L >= 2u) { lo[i] = add_lane_xor16(lo[i]); hi[i] = add_lane_xor16(hi[i]); }
        if constexpr (L >= 3u) { lo[i] = add_lane_xor32(lo[i]); hi[i] = add_lane_xor32(hi[i]); }
      }
      if (y & (k - 1u)) return; // not the box's first row: its sums have gone to the lane that is
      uint32_t q[N];
#pragma unroll
      for (uint32_t i = 0; i < N; i++) q[i] = (((lo[i] + kHalf) >> (2u * L)) & 0x00FF00FFu) | ((((hi[i] + kHalf) >> (2u * L)) & 0x00FF00FFu) << 8);
      store_reduced<L>(base, p, x >> L, y >> L, q);
    }

    // BASE (RgbaStore / PlanarStore<T>) at the job's level: a wave-uniform switch, level 0 is BASE itself
    template <class BASE>
    struct ScaledStore
    {
      BASE base;
      __device__ __forceinline__ void operator()(const WindowDecodeParams &p, uint32_t x, uint32_t y, const uint32_t px[8]) const
      {
        uint32_t q[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
        {
          q[i] = px[i];
          asm volatile("" : "+v"(q[i]));
        }
        switch (p.log2Scale)
        {
        case 0u: base(p, x, y, q); break;
        case 1u: reduce_and_store<1u>(base, p, x, y, q); break;
        case 2u: reduce_and_store<2u>(base, p, x, y, q); break;
        default: reduce_and_store<3u>(base, p, x, y, q); break; // (3: the host entry has refused everything else)
        }
      }
    };

    __device__ __forceinline__ void decode_row(const A16 &k, const unsigned long long packed[3], const uint32_t bb[3], uint32_t px[8])
    {
#pragma unroll
      for (int i = 0; i < 8; i++)
        px[i] = a16_pixel(k, (uint32_t)(packed[0] >> (i * bb[0])) & ((1u << bb[0]) - 1u), (uint32_t)(packed[1] >> (i * bb[1])) & ((1u << bb[1]) - 1u),
                          (uint32_t)(packed[2] >> (i * bb[2])) & ((1u << bb[2]) - 1u));
    }

    // ---- version 1 -------------------------------------------------------------------------------------------------------------------
    struct WindowWaveLds
    {
      uint32_t entry[64][kEntry / 4]; // the unit's table entries, lane == block of the unit
      uint8_t stage[kGroupBytes + 16]; // the current group's payload run (+ what the 12-byte reads of a row's last field reach beyond it)
    };

    // One unit of version 1: up to 64 consecutive blocks of block row `unit / unitsX` of p's window, by one wave.  S: the wave's LDS; payload, payloadWords, channels:
    // from the (checked) header; raise(bits): how the caller reports a group that fails; store: how a lane's 8 pixels leave.  Everything but `lane` is wave-uniform.
    template <class RAISE, class STORE>
    __device__ __forceinline__ void window_unit(const WindowDecodeParams &p, WindowWaveLds &S, uint32_t unit, uint32_t unitsX, int channels, unsigned long long payloadWords,
                                                const uint2 *payload, int lane, RAISE &&raise, const STORE &store)
    {
      const uint32_t j = (uint32_t)lane & 7u, r = (uint32_t)lane >> 3;
      unsigned long long *stage64 = reinterpret_cast<unsigned long long *>(S.stage);
      const uint32_t urow = unit / unitsX, ucol = unit - urow * unitsX;
      const uint32_t by = p.by0 + urow, bxUnit = p.bx0 + ucol * 64u, inUnit = min(64u, p.wbx - ucol * 64u);
      const uint32_t y = by * 8u + r;
      if ((uint32_t)lane < inUnit)
      { // (block (bxUnit + lane, by) lies inside the block grid: the host has checked the window against the image; the table's extent: stream_header_ok)
        const uint2 *ep = reinterpret_cast<const uint2 *>(p.stream + sizeof(limg_hip_stream_header) + ((size_t)by * p.blocksX + bxUnit + (uint32_t)lane) * kEntry);
#pragma unroll
        for (int i = 0; i < kEntry / 8; i++) { const uint2 v = ep[i]; S.entry[lane][2 * i] = v.x; S.entry[lane][2 * i + 1] = v.y; }
      }
      wave_lds_fence();

      // per group of 8 blocks: where its payload run lies, checked as k_stream_decode checks it
      struct Group { uint32_t t, bw, myOff, off0, n; bool valid, any, ok; };
      auto group_info = [&](uint32_t grp) {
        Group G;
        const uint32_t jb = grp * 8u;
        G.any = jb < inUnit; // wave-uniform
        G.t = jb + j; G.bw = 0; G.myOff = 0; G.off0 = 0; G.n = 0; G.valid = false; G.ok = false;
        if (!G.any) return G;
        const uint32_t nValid = min(8u, inUnit - jb);
        G.valid = j < nValid;
        G.bw = G.valid ? entry_bits(S.entry[G.t][12]) : 0u;
        G.myOff = G.valid ? S.entry[G.t][13] : 0u;
        G.off0 = S.entry[jb][13];
        // all of this in 64 bits: offsets come from the (untrusted) stream, and 32-bit sums such as 0xFFFFFFF0 + 24 wrap to small values that pass
        const unsigned long long myEnd = (unsigned long long)G.myOff + words_of(G.bw);
        const uint32_t lastOff = (uint32_t)__shfl((int)G.myOff, (int)nValid - 1, 64), lastWords = (uint32_t)__shfl((int)words_of(G.bw), (int)nValid - 1, 64);
        const unsigned long long endWord = (unsigned long long)lastOff + lastWords;
        const bool sane = G.myOff >= G.off0 && myEnd <= endWord && endWord >= G.off0 && endWord - G.off0 <= (unsigned long long)(kGroupBytes / 8) && endWord <= payloadWords;
        G.ok = __builtin_amdgcn_ballot_w64(G.valid && !sane) == 0;
        G.n = G.ok ? (uint32_t)(endWord - G.off0) : 0u;
        return G;
      };
      auto fetch = [&](const Group &G, uint2 buf[3]) {
#pragma unroll
        for (uint32_t i = 0; i < 3u; i++)
        {
          const uint32_t w = (uint32_t)lane + 64u * i;
          buf[i] = w < G.n ? payload[(size_t)G.off0 + w] : make_uint2(0u, 0u); // (G.n: validated against the payload's size in group_info)
        }
      };

      Group cur = group_info(0);
      uint2 buf[3];
      fetch(cur, buf);
      for (uint32_t grp = 0; grp < 8u; grp++)
      {
        if (!cur.any) break; // wave-uniform
        const Group G = cur;
#pragma unroll
        for (uint32_t i = 0; i < 3u; i++)
        {
          const uint32_t w = (uint32_t)lane + 64u * i;
          if (w < G.n) stage64[w] = ((unsigned long long)buf[i].y << 32) | buf[i].x;
        }
        wave_lds_fence();
        cur = group_info(grp + 1u);
        fetch(cur, buf); // the next group's run, in flight while this one is decoded
        if (!G.ok && lane == 0) raise(2u); // inconsistent offsets: the stream is refused and the group stores nothing
        const uint32_t x = (bxUnit + G.t) * 8u;
        if (G.valid && G.ok && y >= p.y0 && y < p.y0 + p.height && x + 8u > p.x0 && x < p.x0 + p.width)
        {
          const auto before = before_decode(store, p, x, y);
          const uint32_t *e = S.entry[G.t];
          const uint32_t sw = e[12];
          uint32_t fieldByte = (G.myOff - G.off0) * 8u, bb[3], shift[3];
          unsigned long long packed[3];
#pragma unroll
          for (int k = 0; k < 3; k++)
          {
            const uint32_t b = (G.bw >> (8 * k)) & 0xFFu;
            bb[k] = b; shift[k] = min((sw >> (8 * k)) & 0xFFu, 8u);
            const uint32_t o = fieldByte + r * b; // a block row is b bytes of its field
            const uint32_t *wp = reinterpret_cast<const uint32_t *>(S.stage + (o & ~3u));
            const uint32_t d0 = wp[0], d1 = wp[1], d2 = wp[2];
            const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, o & 3u), hi = __builtin_amdgcn_alignbyte(d2, d1, o & 3u);
            packed[k] = ((unsigned long long)hi << 32) | lo;
            fieldByte += b * 8u;
          }
          const A16 k16 = a16_constants([&](int v, int c) { return (int)(int16_t)(e[2 * v + (c >> 1)] >> (16 * (c & 1))); }, shift, channels);
          uint32_t px[8];
          decode_row(k16, packed, bb, px);
          after_decode(store, p, x, y, px, before);
        }
        wave_lds_fence(); // every lane is done reading this group's run
      }
      wave_lds_fence(); // ... and the unit's entries
    }

    __global__ __launch_bounds__(256) void k_stream_window_decode(const WindowDecodeParams p)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
      WindowWaveLds &S = sW[wave];

      const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(p.stream);
      const unsigned long long payloadWords = h->payloadWords;
      if (!stream_header_ok(h, LIMG_HIP_STREAM_VERSION, kEntry, p.nBlocks, p))
      {
        if (tid == 0 && blockIdx.x == 0) atomicOr(p.status, 1u);
        return;
      }
      const int channels = (int)h->channels;
      const uint2 *payload = reinterpret_cast<const uint2 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)p.nBlocks * kEntry);
      const uint32_t unitsX = (p.wbx + 63u) / 64u, nUnits = unitsX * p.wby;
      for (uint32_t unit = blockIdx.x * 4u + (uint32_t)wave; unit < nUnits; unit += gridDim.x * 4u) // (wave-uniform; nothing below synchronises across waves)
        window_unit(p, S, unit, unitsX, channels, payloadWords, payload, lane, [&](uint32_t bits) { atomicOr(p.status, bits); }, RgbaStore());
    }

    // ---- batch: the job table ---------------------------------------------------------------------------------------------------------
    // The job table is written before the launch and by no kernel: read through the constant address space, an entry at a wave-uniform index arrives by scalar loads in
    // scalar registers, as the single-window kernels' arguments do.  The pointers inside it are device memory (the generic loads the compiler would otherwise emit
    // for pointers it has read from memory are slower than global ones).
    template <class T>
    __device__ __forceinline__ T load_uniform(const T *q)
    {
      T v;
      __builtin_memcpy(&v, (const __attribute__((address_space(4))) T *)(uintptr_t)q, sizeof(T));
      return v;
    }
    template <class T>
    __device__ __forceinline__ T *as_global(T *q) { return (T *)(__attribute__((address_space(1))) T *)q; }
    __device__ __forceinline__ WindowDecodeParams load_job(const WindowBatchParams &b, uint32_t job)
    {
      WindowDecodeParams p = load_uniform(b.jobs + job);
      p.stream = as_global(p.stream); p.out = as_global(p.out); p.map = as_global(p.map); p.state = as_global(p.state); p.status = as_global(p.status);
      return p;
    }

    // The slot of `x` in an exclusive prefix of n + 1 entries: base[i] <= x < base[i + 1] (no slot is empty).  x is wave-uniform, so every load below is a scalar
    // load and the index stays in scalar registers: a per-lane search would cost vector registers for nothing.
    __device__ __forceinline__ uint32_t find_slot(const uint32_t *__restrict__ base, uint32_t n, uint32_t x)
    {
      uint32_t lo = 0, hi = n;
      while (hi - lo > 1u)
      {
        const uint32_t mid = (lo + hi) >> 1;
        if (load_uniform(base + mid) <= x) lo = mid; else hi = mid;
      }
      return (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    }

    // a job's status bits: the context's sticky word and the caller's per-job word
    __device__ __forceinline__ void raise_job(const WindowBatchParams &b, uint32_t job, uint32_t bits)
    {
      atomicOr(b.status, bits);
      if (b.jobStatus) atomicOr(b.jobStatus + job, bits);
    }

    // total: what the body keeps across its units (NoTotal; the error kernel's ErrorTotal, which its ErrorSink adds to)
    template <class STORE, class TOTAL = NoTotal>
    __device__ __forceinline__ void stream_windows_body(const WindowBatchParams &b, WindowWaveLds (&sW)[4], const STORE &store, TOTAL &&total = TOTAL())
    {
      const int lane = lane_id();
      const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      WindowWaveLds &S = sW[wave];
      for (uint32_t unit = blockIdx.x * 4u + wave; unit < b.totalUnits; unit += gridDim.x * 4u) // (wave-uniform; nothing below synchronises across waves)
      {
        const uint32_t job = find_slot(b.unitBase, b.count, unit), first = load_uniform(b.unitBase + job);
        const WindowDecodeParams p = load_job(b, job);
        const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(p.stream);
        if (!stream_header_ok(h, LIMG_HIP_STREAM_VERSION, kEntry, p.nBlocks, p))
        { // every unit of the job takes this way: the job writes nothing; its first unit says so
          if (unit == first && lane == 0) raise_job(b, job, 1u);
          continue;
        }
        const uint2 *payload = reinterpret_cast<const uint2 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)p.nBlocks * kEntry);
        total.begin_unit(job, h->channels);
        window_unit(p, S, unit - first, (p.wbx + 63u) / 64u, (int)h->channels, h->payloadWords, payload, lane, [&](uint32_t bits) { raise_job(b, job, bits); }, store);
        total.end_unit();
      }
      total.finish();
    }

    __global__ __launch_bounds__(256) void k_stream_windows_decode(const WindowBatchParams b)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      stream_windows_body(b, sW, RgbaStore());
    }

    template <class T>
    __global__ __launch_bounds__(256) void k_stream_windows_tensor(const WindowBatchParams b, const limg_hip_tensor_format f)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      stream_windows_body(b, sW, PlanarStore<T>{ f });
    }

    // the *_scaled entries: the same bodies, every job stored at its own level
    __global__ __launch_bounds__(256) void k_stream_windows_scaled(const WindowBatchParams b)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      stream_windows_body(b, sW, ScaledStore<RgbaStore>{ RgbaStore() });
    }

    template <class T>
    __global__ __launch_bounds__(256) void k_stream_windows_scaled_tensor(const WindowBatchParams b, const limg_hip_tensor_format f)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      stream_windows_body(b, sW, ScaledStore<PlanarStore<T>>{ PlanarStore<T>{ f } });
    }

    // the *_error entries: the same body, the jobs' sums instead of their pixels (b.errorSums: zeroed in front of the launch)
    __global__ __launch_bounds__(256) void k_stream_windows_error(const WindowBatchParams b)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      __shared__ ErrorEnd sEnd;
      ErrorTotal t{ as_global(b.errorSums), sEnd };
      stream_windows_body(b, sW, ErrorSink{ t }, t);
    }

    // ---- version 2 -------------------------------------------------------------------------------------------------------------------
    __device__ __forceinline__ void refuse(const WindowDecodeParams &p, uint32_t bit)
    {
      atomicOr(p.state + 1, 1u);
      atomicOr(p.status, bit);
    }

    // Whether a rectangle's geometry, shifts and payload extent are sound.  e3: the entry's last 16 bytes; G: the image (WindowDecodeParams / WindowGroup).
    template <class G>
    __device__ __forceinline__ bool rect_ok(const G &g, const uint4 e3, unsigned long long payloadWords)
    {
      const uint32_t ox = e3.z & 0xFFFFu, oy = e3.z >> 16, rx = e3.w & 0xFFFFu, ry = e3.w >> 16, sw = e3.x;
      bool good = rx >= 1u && ry >= 1u && ox + rx <= g.blocksX && oy + ry <= g.blocksY && (sw & 0xFFu) <= 8u && ((sw >> 8) & 0xFFu) <= 8u && ((sw >> 16) & 0xFFu) <= 8u;
      if (good)
      {
        uint32_t wpx;
        const uint32_t n = rect_pixels(g.sizeX, g.sizeY, g.blocksX, g.blocksY, ox, oy, rx, ry, wpx);
        good = (unsigned long long)e3.y + rect_words(n, entry_bits(sw)) <= payloadWords; // (a field is at most n / 8 + 1 words, three of them far below 2^32)
      }
      return good;
    }

    // rectangle (e3) n p's window block range -> ix0, iy0, iw, ih; iw = ih = 0 where they do not meet
    __device__ __forceinline__ void rect_in_window(const WindowDecodeParams &p, const uint4 e3, uint32_t &ix0, uint32_t &iy0, uint32_t &iw, uint32_t &ih)
    {
      const uint32_t ox = e3.z & 0xFFFFu, oy = e3.z >> 16, rx = e3.w & 0xFFFFu, ry = e3.w >> 16;
      ix0 = max(ox, p.bx0); iy0 = max(oy, p.by0); iw = 0; ih = 0;
      const uint32_t ix1 = min(ox + rx, p.bx0 + p.wbx), iy1 = min(oy + ry, p.by0 + p.wby);
      if (ix1 > ix0 && iy1 > iy0) { iw = ix1 - ix0; ih = iy1 - iy0; }
    }

    // The wave's 64 rectangles base .. base + 63, each lane's piece (rectangle n window block range; iw * ih = 0: none) claimed in p's window-sized map.  Returns whether
    // the lane met a block that was taken already; `claimed` counts the lane's claims.
    __device__ __forceinline__ bool claim_pieces(const WindowDecodeParams &p, uint32_t base, int lane, uint32_t ix0, uint32_t iy0, uint32_t iw, uint32_t ih, uint32_t &claimed)
    {
      const uint32_t rect = base + (uint32_t)lane, nb = iw * ih;
      bool clash = false;
      if (nb >= 1u && nb <= 4u)
      { // a small piece: its lane claims it
        for (uint32_t i = 0; i < nb; i++)
        {
          const uint32_t dy = i / iw, dx = i - dy * iw;
          if (atomicCAS(p.map + (size_t)(iy0 - p.by0 + dy) * p.wbx + (ix0 - p.bx0 + dx), kNoRect, rect) != kNoRect) { clash = true; break; }
          claimed++;
        }
      }
      // the large ones, one after the other, by the whole wave; a block that is taken already ends the rectangle (and the stream): the work is bounded by the window's blocks
      unsigned long long big = __builtin_amdgcn_ballot_w64(nb > 4u);
      while (big != 0ull && __builtin_amdgcn_ballot_w64(clash) == 0ull)
      {
        const int src = __builtin_ctzll(big);
        big &= big - 1ull;
        const uint32_t bx = (uint32_t)__shfl((int)ix0, src, 64), by = (uint32_t)__shfl((int)iy0, src, 64), bw = (uint32_t)__shfl((int)iw, src, 64),
                       bnb = (uint32_t)__shfl((int)nb, src, 64);
        for (uint32_t i0 = 0; i0 < bnb && __builtin_amdgcn_ballot_w64(clash) == 0ull; i0 += 64u)
        {
          const uint32_t i = i0 + (uint32_t)lane;
          if (i < bnb)
          {
            const uint32_t dy = i / bw, dx = i - dy * bw;
            if (atomicCAS(p.map + (size_t)(by - p.by0 + dy) * p.wbx + (bx - p.bx0 + dx), kNoRect, base + (uint32_t)src) != kNoRect) clash = true;
            else claimed++;
          }
        }
      }
      return clash;
    }

    __device__ __forceinline__ uint32_t wave_sum(uint32_t v)
    {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
      return v;
    }

    __global__ __launch_bounds__(256) void k_bstream_window_map(const WindowDecodeParams p)
    {
      const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
      const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(p.stream);
      const unsigned long long payloadWords = h->payloadWords;
      const uint32_t nRects = h->reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES];
      if (!(nRects >= 1u && nRects <= p.nBlocks && stream_header_ok(h, LIMG_HIP_STREAM_VERSION_BLOCKED, kRectEntry, nRects, p)))
      {
        if (tid == 0 && blockIdx.x == 0) refuse(p, 1u);
        return;
      }
      uint32_t claimed = 0;
      for (uint32_t base = (blockIdx.x * 4u + (uint32_t)wave) * 64u; base < nRects; base += gridDim.x * 256u)
      {
        if (ld_volatile(p.state + 1) != 0u) break; // refused already (all lanes read the same word: wave-uniform)
        const uint32_t rect = base + (uint32_t)lane;
        uint32_t ix0 = 0, iy0 = 0, iw = 0, ih = 0; // rectangle n window block range
        if (rect < nRects)
        {
          const uint4 e3 = reinterpret_cast<const uint4 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)rect * kRectEntry)[3];
          if (!rect_ok(p, e3, payloadWords)) refuse(p, 2u);
          else rect_in_window(p, e3, ix0, iy0, iw, ih);
        }
        if (claim_pieces(p, base, lane, ix0, iy0, iw, ih, claimed)) refuse(p, 2u);
      }
      claimed = wave_sum(claimed);
      if (lane == 0 && claimed) atomicAdd(p.state, claimed);
    }

    // One unit of version 2: 8 consecutive blocks of block row `unit / unitsX` of p's window, lane = (block j = lane & 7, row = lane >> 3).  nRects, channels, tableEnd,
    // total: from the header the map kernel has checked; the caller has read the verdict.  store: how a lane's 8 pixels leave.
    template <class STORE>
    __device__ __forceinline__ void bwindow_unit(const WindowDecodeParams &p, uint32_t unit, uint32_t unitsX, uint32_t nRects, uint32_t channels, unsigned long long tableEnd,
                                                 unsigned long long total, int lane, const STORE &store)
    {
      const uint32_t j = (uint32_t)lane & 7u, row = (uint32_t)lane >> 3;
      const uint32_t urow = unit / unitsX, wbxi = (unit - urow * unitsX) * 8u + j; // the block's place in the window's block range
      const uint32_t y = (p.by0 + urow) * 8u + row, x = (p.bx0 + wbxi) * 8u;
      if (wbxi >= p.wbx || y < p.y0 || y >= p.y0 + p.height) return;
      const uint32_t rect = p.map[(size_t)urow * p.wbx + wbxi];
      if (rect >= nRects) return; // (cannot happen after the verdict; a lane never indexes the table with anything else)
      const uint4 *ep = reinterpret_cast<const uint4 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)rect * kRectEntry);
      const uint4 e0 = ep[0], e1 = ep[1], e2 = ep[2], e3 = ep[3];
      const uint32_t ev[12] = { e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x, e2.y, e2.z, e2.w };
      const uint32_t sw = e3.x, ox = e3.z & 0xFFFFu, oy = e3.z >> 16, rx = e3.w & 0xFFFFu, ry = e3.w >> 16;
      uint32_t wpx;
      const uint32_t n = rect_pixels(p.sizeX, p.sizeY, p.blocksX, p.blocksY, ox, oy, rx, ry, wpx);
      const unsigned long long i0 = (unsigned long long)(y - oy * 8u) * wpx + (x - ox * 8u);
      const uint32_t bits = entry_bits(sw);
      // the lane's 8 values of each field: the bit run at i0 * b
      unsigned long long packed[3];
      uint32_t bb[3], shift[3];
      unsigned long long fieldByte = tableEnd + (unsigned long long)e3.y * 8ull;
#pragma unroll
      for (int k = 0; k < 3; k++)
      {
        const uint32_t b = (bits >> (8 * k)) & 0xFFu;
        bb[k] = b; shift[k] = (sw >> (8 * k)) & 0xFFu;
        packed[k] = 0;
        if (b)
        {
          const unsigned long long bit = i0 * b, byte = fieldByte + (bit >> 3), at = byte & ~3ull;
          const uint32_t sh = (uint32_t)(byte & 3ull) * 8u + (uint32_t)(bit & 7ull); // < 32
          // three aligned dwords hold the run's 64 bits wherever it starts; the last may lie beyond the stream's end (never beyond the field's: it is not used then)
          const uint32_t *wp = reinterpret_cast<const uint32_t *>(p.stream + at);
          const uint32_t d0 = at + 4ull <= total ? wp[0] : 0u, d1 = at + 8ull <= total ? wp[1] : 0u, d2 = at + 12ull <= total ? wp[2] : 0u;
          const unsigned long long lo = ((unsigned long long)d1 << 32) | d0;
          packed[k] = sh ? ((lo >> sh) | ((unsigned long long)d2 << (64u - sh))) : lo;
          fieldByte += (unsigned long long)field_words(n, b) * 8ull;
        }
      }
      // (behind the last load of the chain map -> entry -> payload: loads return in order, so anything requested ahead of the chain would have to arrive before its
      // next link could be read, and the chain's links come from the cache where the original comes from memory)
      const auto before = before_decode(store, p, x, y);
      const A16 k16 = a16_constants([&](int v, int c) { return (int)(int16_t)(ev[2 * v + (c >> 1)] >> (16 * (c & 1))); }, shift, (int)channels);
      uint32_t px[8];
      decode_row(k16, packed, bb, px);
      after_decode(store, p, x, y, px, before); // (columns beyond a partial last block column lie outside the image, so outside the window)
    }

    __global__ __launch_bounds__(256) void k_bstream_window_decode(const WindowDecodeParams p)
    {
      const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
      // the verdict of k_bstream_window_map: nothing flagged and every block of the window claimed exactly once (claims never overlap, so the count says it)
      if (ld_volatile(p.state + 1) != 0u || ld_volatile(p.state) != p.wbx * p.wby)
      {
        if (tid == 0 && blockIdx.x == 0) atomicOr(p.status, 2u);
        return;
      }
      // the header by scalar loads (no kernel of this call writes the stream): nRects, channels, tableEnd and total then stay in scalar registers through the loop.  As
      // plain loads they came out as vector loads: 8 vector registers more, 71 in all, and 7 waves per SIMD where the launch counts on 8
      const limg_hip_stream_header h = load_uniform(reinterpret_cast<const limg_hip_stream_header *>(p.stream));
      const uint32_t nRects = h.reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES], channels = h.channels;
      const unsigned long long tableEnd = sizeof(limg_hip_stream_header) + (unsigned long long)nRects * kRectEntry, total = tableEnd + h.payloadWords * 8ull;
      const uint32_t unitsX = (p.wbx + 7u) / 8u, nUnits = unitsX * p.wby;
      for (uint32_t unit = blockIdx.x * 4u + (uint32_t)wave; unit < nUnits; unit += gridDim.x * 4u) bwindow_unit(p, unit, unitsX, nRects, channels, tableEnd, total, lane, RgbaStore());
    }

    // ---- version 2, batch ------------------------------------------------------------------------------------------------------------
    // every job of the group is refused: a header that does not match or a rectangle that is malformed concerns all windows of the stream
    __device__ __forceinline__ void refuse_group(const WindowBatchParams &b, const WindowGroup &g, uint32_t bit, int lane)
    {
      for (uint32_t jj = (uint32_t)lane; jj < g.nJobs; jj += 64u)
      {
        const uint32_t job = b.groupJobs[g.firstJob + jj];
        atomicOr(b.jobs[job].state + 1, 1u);
        if (b.jobStatus) atomicOr(b.jobStatus + job, bit);
      }
      if (lane == 0) atomicOr(b.status, bit);
    }

    __global__ __launch_bounds__(256) void k_bstream_windows_map(const WindowBatchParams b)
    {
      const int lane = lane_id();
      const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      for (uint32_t item = blockIdx.x * 4u + wave; item < b.totalItems; item += gridDim.x * 4u) // (wave-uniform)
      {
        const uint32_t gi = find_slot(b.groupItemBase, b.nGroups, item);
        WindowGroup g = load_uniform(b.groups + gi);
        g.stream = as_global(g.stream);
        const uint32_t base = (item - load_uniform(b.groupItemBase + gi)) * 64u;
        const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(g.stream);
        const unsigned long long payloadWords = h->payloadWords;
        const uint32_t nRects = h->reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES];
        if (!(nRects >= 1u && nRects <= g.nBlocks && stream_header_ok(h, LIMG_HIP_STREAM_VERSION_BLOCKED, kRectEntry, nRects, g)))
        { // every item of the group takes this way: nothing of the table is read; the first item refuses the group's jobs
          if (base == 0u) refuse_group(b, g, 1u, lane);
          continue;
        }
        if (base >= nRects) continue; // (the items cover nBlocks rectangles, the most a table may hold)
        // the rectangle, checked once for the whole group
        const uint32_t rect = base + (uint32_t)lane;
        uint4 e3 = make_uint4(0u, 0u, 0u, 0u);
        bool good = true;
        if (rect < nRects)
        {
          e3 = reinterpret_cast<const uint4 *>(g.stream + sizeof(limg_hip_stream_header) + (size_t)rect * kRectEntry)[3];
          good = rect_ok(g, e3, payloadWords);
        }
        if (__builtin_amdgcn_ballot_w64(!good) != 0ull)
        {
          refuse_group(b, g, 2u, lane);
          continue;
        }
        // ... and offered to every window of the group (lanes beyond the table: e3 = 0 is a rectangle of no blocks)
        for (uint32_t jj = 0; jj < g.nJobs; jj++)
        {
          const uint32_t job = load_uniform(b.groupJobs + g.firstJob + jj);
          const WindowDecodeParams p = load_job(b, job);
          if (ld_volatile(p.state + 1) != 0u) continue; // refused already: nothing of it will be decoded (wave-uniform)
          uint32_t ix0, iy0, iw, ih;
          rect_in_window(p, e3, ix0, iy0, iw, ih);
          if (__builtin_amdgcn_ballot_w64(iw * ih != 0u) == 0ull) continue; // none of the 64 meets this window
          uint32_t claimed = 0;
          if (__builtin_amdgcn_ballot_w64(claim_pieces(p, base, lane, ix0, iy0, iw, ih, claimed)) != 0ull && lane == 0)
          { // a clash refuses the job whose map it happened in
            atomicOr(p.state + 1, 1u);
            raise_job(b, job, 2u);
          }
          claimed = wave_sum(claimed);
          if (lane == 0 && claimed) atomicAdd(p.state, claimed);
        }
      }
    }

    // TOTAL::kKeepsJob (the error kernel): a job is typically a whole image, thousands of consecutive units, so what a unit needs to know about its job -- the table
    // entry, the verdict, the header -- is kept in scalar registers while the wave's units stay inside the job's range first .. end - 1 and read once per run of them
    // (the header by scalar loads, as k_bstream_window_decode reads it); the kernels that store look everything up per unit, as they did.  (GPU time of
    // k_bstream_windows_error with the per-unit lookup instead: profiles/stream_error.md, "Version 2's error kernel".)
    template <class STORE, class TOTAL = NoTotal>
    __device__ __forceinline__ void bstream_windows_body(const WindowBatchParams &b, const STORE &store, TOTAL &&total = TOTAL())
    {
      constexpr bool keeps = std::remove_reference_t<TOTAL>::kKeepsJob;
      const int lane = lane_id();
      const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      uint32_t job = 0, first = 0, end = 0, nRects = 0, channels = 0;
      unsigned long long tableEnd = 0, streamEnd = 0;
      bool refused = false;
      WindowDecodeParams p;
      for (uint32_t unit = blockIdx.x * 4u + wave; unit < b.totalUnits; unit += gridDim.x * 4u) // (wave-uniform)
      {
        if (!keeps || unit < first || unit >= end)
        {
          job = find_slot(b.unitBase, b.count, unit); first = load_uniform(b.unitBase + job);
          if constexpr (keeps) end = load_uniform(b.unitBase + job + 1u);
          p = load_job(b, job);
          // the job's verdict from k_bstream_windows_map: nothing flagged and every block of its window claimed exactly once
          refused = ld_volatile(p.state + 1) != 0u || ld_volatile(p.state) != p.wbx * p.wby;
          if constexpr (keeps)
            if (!refused)
            {
              const limg_hip_stream_header h = load_uniform(reinterpret_cast<const limg_hip_stream_header *>(p.stream));
              nRects = h.reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES]; channels = h.channels;
              tableEnd = sizeof(limg_hip_stream_header) + (unsigned long long)nRects * kRectEntry; streamEnd = tableEnd + h.payloadWords * 8ull;
            }
        }
        if (refused)
        {
          if (unit == first && lane == 0) raise_job(b, job, 2u);
          continue;
        }
        if constexpr (!keeps)
        {
          const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(p.stream);
          nRects = h->reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES]; channels = h->channels;
          tableEnd = sizeof(limg_hip_stream_header) + (unsigned long long)nRects * kRectEntry; streamEnd = tableEnd + h->payloadWords * 8ull;
        }
        total.begin_unit(job, channels);
        bwindow_unit(p, unit - first, (p.wbx + 7u) / 8u, nRects, channels, tableEnd, streamEnd, lane, store);
        total.end_unit();
      }
      total.finish();
    }

    __global__ __launch_bounds__(256) void k_bstream_windows_decode(const WindowBatchParams b) { bstream_windows_body(b, RgbaStore()); }

    template <class T>
    __global__ __launch_bounds__(256) void k_bstream_windows_tensor(const WindowBatchParams b, const limg_hip_tensor_format f) { bstream_windows_body(b, PlanarStore<T>{ f }); }

    // (8 workgroups per CU asked for: left alone the allocator takes 65 vector registers and 7 waves per SIMD; held to 64 it needs no scratch and runs the 8 the launch counts on)
    __global__ __launch_bounds__(256, 8) void k_bstream_windows_scaled(const WindowBatchParams b) { bstream_windows_body(b, ScaledStore<RgbaStore>{ RgbaStore() }); }

    template <class T>
    __global__ __launch_bounds__(256, 8) void k_bstream_windows_scaled_tensor(const WindowBatchParams b, const limg_hip_tensor_format f)
    {
      bstream_windows_body(b, ScaledStore<PlanarStore<T>>{ PlanarStore<T>{ f } });
    }

    // (70 vector registers, 7 waves per SIMD as k_bstream_windows_decode's 66; held to 64 for the eighth it would spill two of them to scratch)
    __global__ __launch_bounds__(256) void k_bstream_windows_error(const WindowBatchParams b)
    {
      __shared__ ErrorEnd sEnd;
      ErrorTotal t{ as_global(b.errorSums), sEnd };
      bstream_windows_body(b, ErrorSink{ t }, t);
    }

    // ---- resized, both versions ------------------------------------------------------------------------------------------------------------
    // Work item = an output tile of a job, by one workgroup: (1) its four waves decode the job's units that meet the tile's level-L footprint with the unit bodies
    // above, stored by ScaledStore<TileStore> into the LDS tile; (2) barrier; (3) lane = output column, wave = every fourth output row: the four taps as dword reads
    // from the tile, bytes two per dword half horizontally (255 * 256 fits 16 bits), one per dword vertically, and one store per output element -- a wave's store is
    // 64 consecutive elements of an output row.  The unit bodies get a LOCAL copy of the job's parameters whose pixel clip is the tile's footprint in whole k x k boxes
    // (so the lane partners of the reduction stay on the same branches); block range, map, state and status stay the job's, and with them the unit numbering, every
    // validation and version 2's map indexing.
    struct RgbaOut
    {
      __device__ __forceinline__ void operator()(const WindowDecodeParams &p, uint32_t X, uint32_t Y, uint32_t px) const { p.out[(unsigned long long)Y * p.outStride + X] = px; }
    };
    template <class T>
    struct PlanarOut
    {
      limg_hip_tensor_format f;
      __device__ __forceinline__ void operator()(const WindowDecodeParams &p, uint32_t X, uint32_t Y, uint32_t px) const
      {
        T *at = reinterpret_cast<T *>(p.out) + (unsigned long long)Y * p.outStride + X;
#pragma unroll
        for (uint32_t c = 0; c < 4u; c++)
        {
          if (c >= f.planes) break; // (wave-uniform)
          at[(unsigned long long)c * p.planeStride] = (T)((float)((px >> (8u * c)) & 0xFFu) * f.scale[c] + f.bias[c]);
        }
      }
    };

    template <bool RECTS, class OUT>
    __device__ __forceinline__ void resized_body(const WindowResizeParams &r, uint32_t *tile, WindowWaveLds *sW, const OUT &out)
    {
      const int lane = lane_id();
      const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      for (uint32_t t = blockIdx.x; t < r.totalTiles; t += gridDim.x) // (workgroup-uniform, and so is every `continue` below: no wave misses a barrier)
      {
        const uint32_t job = find_slot(r.tileBase, r.b.count, t), first = load_uniform(r.tileBase + job);
        const WindowDecodeParams p = load_job(r.b, job);
        const ResizeJob rj = load_uniform(r.resize + job);
        const limg_hip_stream_header *h = reinterpret_cast<const limg_hip_stream_header *>(p.stream);
        if constexpr (!RECTS)
        {
          if (!stream_header_ok(h, LIMG_HIP_STREAM_VERSION, kEntry, p.nBlocks, p))
          { // every tile of the job takes this way: the job writes nothing; its first tile says so
            if (t == first && threadIdx.x == 0) raise_job(r.b, job, 1u);
            continue;
          }
        }
        else if (ld_volatile(p.state + 1) != 0u || ld_volatile(p.state) != p.wbx * p.wby)
        { // the job's verdict from k_bstream_windows_map
          if (t == first && threadIdx.x == 0) raise_job(r.b, job, 2u);
          continue;
        }
        // the tile: output columns X0 .. X0 + tw - 1 of rows Y0 .. Y0 + th - 1, and the level pixels its first and last column and row tap
        const uint32_t L = p.log2Scale, flip = rj.flags & LIMG_HIP_RESIZE_FLIP_X;
        const uint32_t ti = t - first, ty = ti / rj.tilesX, tx = ti - ty * rj.tilesX;
        const uint32_t X0 = tx * rj.tileW, Y0 = ty * rj.tileH, tw = min(rj.tileW, rj.outW - X0), th = min(rj.tileH, rj.outH - Y0);
        const uint32_t lox = p.x0 >> L, hix = lox + (p.width >> L) - 1u, loy = p.y0 >> L, hiy = loy + (p.height >> L) - 1u;
        const ResizeTaps xA = resize_axis(flip ? rj.outW - 1u - X0 : X0, rj.x0, rj.srcW, rj.outW, L, lox, hix);
        const ResizeTaps xB = resize_axis(flip ? rj.outW - X0 - tw : X0 + tw - 1u, rj.x0, rj.srcW, rj.outW, L, lox, hix);
        const ResizeTaps yA = resize_axis(Y0, rj.y0, rj.srcH, rj.outH, L, loy, hiy), yB = resize_axis(Y0 + th - 1u, rj.y0, rj.srcH, rj.outH, L, loy, hiy);
        const uint32_t fx0 = min(xA.a, xB.a), fw = max(xA.b, xB.b) - fx0 + 1u, fy0 = yA.a, fh = yB.b - fy0 + 1u;
        if (fw * fh > kResizeTilePixels || tw > 64u) continue; // (the host has planned the tiles so that this cannot happen; nothing is ever stored beyond the tile)

        WindowDecodeParams lp = p;
        lp.x0 = fx0 << L; lp.width = fw << L; lp.y0 = fy0 << L; lp.height = fh << L;
        const ScaledStore<TileStore> store{ TileStore{ tile, fx0, fy0, fw, fh } };
        constexpr uint32_t kUnit = RECTS ? 3u : 6u; // log2 of a unit's width in blocks
        const uint32_t unitsX = (p.wbx + (1u << kUnit) - 1u) >> kUnit;
        const uint32_t ua = ((lp.x0 >> 3) - p.bx0) >> kUnit, nuc = ((((lp.x0 + lp.width - 1u) >> 3) - p.bx0) >> kUnit) - ua + 1u;
        const uint32_t bya = (lp.y0 >> 3) - p.by0, nU = nuc * (((lp.y0 + lp.height - 1u) >> 3) - p.by0 - bya + 1u);
        if constexpr (!RECTS)
        {
          const uint2 *payload = reinterpret_cast<const uint2 *>(p.stream + sizeof(limg_hip_stream_header) + (size_t)p.nBlocks * kEntry);
          const int channels = (int)h->channels;
          const unsigned long long payloadWords = h->payloadWords;
          for (uint32_t i = wave; i < nU; i += 4u) // (wave-uniform)
          {
            const uint32_t ur = i / nuc;
            window_unit(lp, sW[wave], (bya + ur) * unitsX + ua + (i - ur * nuc), unitsX, channels, payloadWords, payload, lane, [&](uint32_t bits) { raise_job(r.b, job, bits); }, store);
          }
        }
        else
        {
          const uint32_t nRects = h->reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES], channels = h->channels;
          const unsigned long long tableEnd = sizeof(limg_hip_stream_header) + (unsigned long long)nRects * kRectEntry, total = tableEnd + h->payloadWords * 8ull;
          for (uint32_t i = wave; i < nU; i += 4u)
          {
            const uint32_t ur = i / nuc;
            bwindow_unit(lp, (bya + ur) * unitsX + ua + (i - ur * nuc), unitsX, nRects, channels, tableEnd, total, lane, store);
          }
        }
        __syncthreads();

        if ((uint32_t)lane < tw)
        {
          const uint32_t X = X0 + (uint32_t)lane;
          const ResizeTaps cx = resize_axis(flip ? rj.outW - 1u - X : X, rj.x0, rj.srcW, rj.outW, L, lox, hix);
          const uint32_t ca = cx.a - fx0, cb = cx.b - fx0, f = cx.f, nf = 256u - f;
          // the y axis' quotient for the wave's first row, then stepped four rows at a time with the job's (stepQ, stepR)
          const unsigned long long num = ((unsigned long long)(2u * (Y0 + wave) + 1u) * rj.srcH) << 15;
          unsigned long long q = num / rj.outH;
          uint32_t rem = (uint32_t)(num - q * rj.outH);
          for (uint32_t Y = Y0 + wave; Y < Y0 + th; Y += 4u)
          {
            const ResizeTaps cy = resize_taps(((unsigned long long)rj.y0 << 16) + q, L, loy, hiy);
            const uint32_t *ra = tile + (cy.a - fy0) * fw, *rb = tile + (cy.b - fy0) * fw;
            const uint32_t p00 = ra[ca], p01 = ra[cb], p10 = rb[ca], p11 = rb[cb], g = cy.f, ng = 256u - g;
            const uint32_t tlo = (p00 & 0x00FF00FFu) * nf + (p01 & 0x00FF00FFu) * f, thi = ((p00 >> 8) & 0x00FF00FFu) * nf + ((p01 >> 8) & 0x00FF00FFu) * f;
            const uint32_t blo = (p10 & 0x00FF00FFu) * nf + (p11 & 0x00FF00FFu) * f, bhi = ((p10 >> 8) & 0x00FF00FFu) * nf + ((p11 >> 8) & 0x00FF00FFu) * f;
            const uint32_t b0 = ((tlo & 0xFFFFu) * ng + (blo & 0xFFFFu) * g + 32768u) >> 16, b2 = ((tlo >> 16) * ng + (blo >> 16) * g + 32768u) >> 16;
            const uint32_t b1 = ((thi & 0xFFFFu) * ng + (bhi & 0xFFFFu) * g + 32768u) >> 16, b3 = ((thi >> 16) * ng + (bhi >> 16) * g + 32768u) >> 16;
            out(p, X, Y, b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
            q += rj.stepQ; rem += rj.stepR;
            if (rem >= rj.outH) { rem -= rj.outH; q++; }
          }
        }
        __syncthreads(); // the tile is free for the next one
      }
    }

    __global__ __launch_bounds__(256) void k_stream_windows_resized(const WindowResizeParams r)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      __shared__ __align__(16) uint32_t sTile[kResizeTilePixels];
      resized_body<false>(r, sTile, sW, RgbaOut());
    }

    template <class T>
    __global__ __launch_bounds__(256) void k_stream_windows_resized_tensor(const WindowResizeParams r, const limg_hip_tensor_format f)
    {
      __shared__ __align__(16) WindowWaveLds sW[4];
      __shared__ __align__(16) uint32_t sTile[kResizeTilePixels];
      resized_body<false>(r, sTile, sW, PlanarOut<T>{ f });
    }

    __global__ __launch_bounds__(256) void k_bstream_windows_resized(const WindowResizeParams r)
    {
      __shared__ __align__(16) uint32_t sTile[kResizeTilePixels];
      resized_body<true>(r, sTile, nullptr, RgbaOut());
    }

    template <class T>
    __global__ __launch_bounds__(256) void k_bstream_windows_resized_tensor(const WindowResizeParams r, const limg_hip_tensor_format f)
    {
      __shared__ __align__(16) uint32_t sTile[kResizeTilePixels];
      resized_body<true>(r, sTile, nullptr, PlanarOut<T>{ f });
    }
  }

  // persistent launches: a workgroup of four waves per residency slot at most, every wave strides over its units.  slotsPerCu: 4 for version 1 (its 100 vector
  // registers), 8 for version 2
  static dim3 window_grid(uint32_t units, int cus, uint32_t slotsPerCu)
  {
    const uint32_t need = units / 4u + (units % 4u ? 1u : 0u), slots = (uint32_t)cus * slotsPerCu;
    return dim3(need < slots ? need : slots);
  }

  void launch_stream_window_decode(const WindowDecodeParams &p, int cus, hipStream_t s)
  {
    hipLaunchKernelGGL(k_stream_window_decode, window_grid(((p.wbx + 63u) / 64u) * p.wby, cus, 4u), dim3(256), 0, s, p);
  }

  void launch_blocked_stream_window_decode(const WindowDecodeParams &p, int cus, hipStream_t s)
  {
    hipLaunchKernelGGL(k_bstream_window_map, window_grid((p.nBlocks + 63u) / 64u, cus, 8u), dim3(256), 0, s, p); // at most nBlocks rectangles, 64 per wave
    hipLaunchKernelGGL(k_bstream_window_decode, window_grid(((p.wbx + 7u) / 8u) * p.wby, cus, 8u), dim3(256), 0, s, p);
  }

  // the batched forms: the grid comes from the call's totals, so many small windows fill the device that one of them would leave nearly empty.  f: the tensor format
  // (its type checked by the host entry), NULL for packed RGBA8; scaled: the job types with a level, which have kernels of their own whatever the levels are.
  // (Templates are emitted in the order they are first named in: tensor before scaled, version 1 before 2, as the device code has had them so far.)
  static void launch_windows_decode(bool rects, bool scaled, const limg_hip_tensor_format *f, const WindowBatchParams &b, dim3 grid, hipStream_t s)
  {
    const bool half = f && f->type == LIMG_HIP_TENSOR_F16;
    if (!f) hipLaunchKernelGGL(!scaled ? (!rects ? k_stream_windows_decode : k_bstream_windows_decode) : (!rects ? k_stream_windows_scaled : k_bstream_windows_scaled), grid, dim3(256), 0, s, b);
    else if (!scaled)
      hipLaunchKernelGGL(!rects ? (half ? k_stream_windows_tensor<_Float16> : k_stream_windows_tensor<float>) : (half ? k_bstream_windows_tensor<_Float16> : k_bstream_windows_tensor<float>),
                         grid, dim3(256), 0, s, b, *f);
    else
      hipLaunchKernelGGL(!rects ? (half ? k_stream_windows_scaled_tensor<_Float16> : k_stream_windows_scaled_tensor<float>)
                                : (half ? k_bstream_windows_scaled_tensor<_Float16> : k_bstream_windows_scaled_tensor<float>),
                         grid, dim3(256), 0, s, b, *f);
  }

  void launch_stream_windows(const WindowBatchParams &b, bool scaled, const limg_hip_tensor_format *f, int cus, hipStream_t s)
  {
    launch_windows_decode(false, scaled, f, b, window_grid(b.totalUnits, cus, 4u), s);
  }

  // version 2: the map kernel first; it never touches the output, works on the footprints and so serves every form as it is
  void launch_blocked_stream_windows(const WindowBatchParams &b, bool scaled, const limg_hip_tensor_format *f, int cus, hipStream_t s)
  {
    hipLaunchKernelGGL(k_bstream_windows_map, window_grid(b.totalItems, cus, 8u), dim3(256), 0, s, b);
    launch_windows_decode(true, scaled, f, b, window_grid(b.totalUnits, cus, 8u), s);
  }

  // the error forms: the batched launches with the error kernels (b.errorSums set, zeroed on `s` in front of this)
  void launch_stream_windows_error(const WindowBatchParams &b, int cus, hipStream_t s)
  {
    hipLaunchKernelGGL(k_stream_windows_error, window_grid(b.totalUnits, cus, 4u), dim3(256), 0, s, b);
  }

  void launch_blocked_stream_windows_error(const WindowBatchParams &b, int cus, hipStream_t s)
  {
    hipLaunchKernelGGL(k_bstream_windows_map, window_grid(b.totalItems, cus, 8u), dim3(256), 0, s, b);
    // 7 residency slots per CU, what the kernel's 70 vector registers allow: an eighth workgroup per CU would start only when one of the seven has ended and run its
    // units as a second round behind them
    hipLaunchKernelGGL(k_bstream_windows_error, window_grid(b.totalUnits, cus, 7u), dim3(256), 0, s, b);
  }

  // the resized forms: a workgroup per output tile, persistent over the call's tiles.  Residency slots per CU: 4 for version 1 (111 vector registers; 4 x (4
  // WindowWaveLds + the 16 KiB tile) = 144 KiB of the CU's 160), 6 for version 2 (73 vector registers; 6 x 16 KiB)
  static void launch_windows_resized(bool rects, const limg_hip_tensor_format *f, const WindowResizeParams &r, int cus, hipStream_t s)
  {
    const uint32_t slots = (uint32_t)cus * (rects ? 6u : 4u);
    const dim3 grid(r.totalTiles < slots ? r.totalTiles : slots);
    const bool half = f && f->type == LIMG_HIP_TENSOR_F16;
    if (!f) hipLaunchKernelGGL(!rects ? k_stream_windows_resized : k_bstream_windows_resized, grid, dim3(256), 0, s, r);
    else
      hipLaunchKernelGGL(!rects ? (half ? k_stream_windows_resized_tensor<_Float16> : k_stream_windows_resized_tensor<float>)
                                : (half ? k_bstream_windows_resized_tensor<_Float16> : k_bstream_windows_resized_tensor<float>),
                         grid, dim3(256), 0, s, r, *f);
  }

  void launch_stream_windows_resized(const WindowResizeParams &r, const limg_hip_tensor_format *f, int cus, hipStream_t s) { launch_windows_resized(false, f, r, cus, s); }

  void launch_blocked_stream_windows_resized(const WindowResizeParams &r, const limg_hip_tensor_format *f, int cus, hipStream_t s)
  {
    hipLaunchKernelGGL(k_bstream_windows_map, window_grid(r.b.totalItems, cus, 8u), dim3(256), 0, s, r.b);
    launch_windows_resized(true, f, r, cus, s);
  }
}
