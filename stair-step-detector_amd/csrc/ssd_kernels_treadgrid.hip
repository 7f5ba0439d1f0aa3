/*
 * ssd_kernels_treadgrid.hip - the tread grid pass (ssd_enqueue_tread_grid, ssd_enqueue_cameras_tread_grid) and its
 * launcher.
 *
 * WHERE on each reported surface the tread was seen and where something stands: per surface a grid of SSD_TG_ROWS x SSD_TG_COLS cells in
 * the surface's own frame, per cell the tread points, the occupants and the tallest occupant (the rule: ssd_treadgrid.h, one text with
 * ssd_tread_grid_host, on the clearance rule of ssd_clearance.h).  The pass reads what k_clearance reads - the frame's RESULT record,
 * K1's cell records, the points - and writes the caller's record alone.  The file is compiled at the end of ssd_kernels_refit.hip, behind
 * ssd_kernels_clearance.hip (clearance_bin is that file's): the passes that run behind a whole enqueue are one translation unit.  The
 * walk is ssd_k_walk.h's (chunk_of, wanted_cells).
 *
 * Accumulation.  Unlike clearance, nearly every point of a stair frame counts (it is a tread point), so the counts are staged in LDS:
 * per surface one word per cell that packs the tread points (low half) and the occupants (high half) - a block's chunk is fewer than
 * 2^16 points, so neither half can carry - and one more word for what falls outside the grid.  17 surfaces: 17.1 KB, 23.6 KB with
 * the prologue's tables, which leaves room for six blocks on a CU (with a plane for the tallest occupant in LDS as well: 41.1 KB, three
 * blocks, and 1.50 ms where this takes 1.04 on the XGA batch: the walk waits for memory, and residency hides that).
 * A lane's four points are consecutive pixels and mostly fall into one cell, so a lane combines its own equal keys first and sends one
 * LDS add per distinct key; combining across the wave instead (a ballot per distinct key) was measured and lost - a point slot's 64
 * lanes are four rows of pixels 4 apart and spread over many cells (profiles/tread_grid_time.txt).
 * Occupants are rare: their count goes to LDS directly and their height to the record with one global atomic maximum each.  At the
 * block's end one global atomic per non-zero count goes to the frame's record, which the caller zeroed on the stream.  Integer adds and
 * maxima: no byte depends on an order.
 */
#include "ssd_k_walk.h"
#include "ssd_launch_rules.h"
#include "ssd_treadgrid.h"

namespace ssd
{

constexpr int kTgSlots = kTgCells + 1;           /* a surface's cells, then what falls outside its grid */
static_assert(kMaxTilesPerBlock * kTile < 65536, "a block's counts of one cell fit a half word");
static_assert(sizeof(ssd_tread_grid) == 4 * (4 + 3 * kTgCells) && sizeof(ssd_frame_tread_grid) == 8 + SSD_MAX_STEPS * sizeof(ssd_tread_grid),
              "ssd_frame_tread_grid is the kernel's record: a header of two int32, then per surface four words and three planes of a word per cell");

struct TreadGridLds
{
  unsigned short cellList[kMaxCellsPerBlock];
  unsigned int listScratch[2 * kWavesPerBlock];
  ClearanceSurface s[SSD_MAX_STEPS];             /* the frame's reported surfaces as the clearance rule reads them */
  TreadGridAxes axes[SSD_MAX_STEPS];             /* ... and each one's own frame */
  unsigned int band[kMaxBins];                   /* height bin -> the surfaces whose band may hold a point of the bin (a superset) */
  unsigned int slab[kMaxBins];                   /* ... and those whose slab may */
  unsigned int wanted;                           /* the bin groups with a candidate of either kind */
  unsigned int counts[SSD_MAX_STEPS * kTgSlots]; /* tread points | occupants << 16 */
};

/* A lane's kPts tread points (keys[j] >= 0: a slot of L.counts; the points are consecutive pixels, so mostly one cell): equal keys are
 * counted once, then one LDS add per distinct key.  (Combining equal keys across the wave per point slot instead - a ballot per distinct
 * key, one LDS add by its first lane - was measured and lost: profiles/tread_grid_time.txt; the code: commit ad9a851.) */
__device__ __forceinline__ void tread_grid_count(unsigned int *counts, int (&keys)[kPts], int lane, int limit)
{
#pragma unroll
  for(int j = 0; j < kPts; j++)
  {
    unsigned int n = 1u;
#pragma unroll
    for(int i = j + 1; i < kPts; i++)
      if(keys[i] == keys[j])
      {
        n++;
        keys[i] = -1;
      }
    if(keys[j] >= 0 && SSD_CHK(35, keys[j], limit))
      atomicAdd(&counts[keys[j]], n);
  }
}

/* Where a block's staircase comes from and where its counts go (tread_grid_block's `where`): index(frame) = which result and which record
 * of the body's `results` and `out` are the block's (below 0: none, the block adds nothing; kEveryFrame: that cannot be), header(..) writes
 * what the pass owes the records' headers, result(..) is the staircase.  The tread grid's own: the frame's result record, the frame's
 * record of the caller's; the record's header as k_clearance writes its own.  The stair map's: ssd_kernels_stairmap.hip */
struct TreadGridOwnFrame
{
  static constexpr bool kEveryFrame = true;
  static constexpr bool kSharedRecord = false;   /* a record is one frame's: its few occupants send their heights as they come */
  const FrameState *__restrict__ st;
  __device__ __forceinline__ int index(int frame) const { return frame; }
  __device__ __forceinline__ void header(int frame, int tid, ssd_frame_tread_grid *__restrict__ out) const
  {
    const FrameState &fs = st[frame];
    const bool live = fs.anyActive != 0u && (fs.status & SSD_ST_THROW) == 0u;
    if(live && tid == 0 && blockIdx.y == 0)
    {
      const int nLive = fs.nLive;
      out[frame].n_surfaces = min(nLive, SSD_MAX_STEPS);
      out[frame].ground = (nLive > 0 && fs.accActive[kGroundAcc]) ? 1 : 0;
    }
  }
  __device__ __forceinline__ const ssd_frame_result &result(const ssd_frame_result *__restrict__ results, int at) const { return results[at]; }
};

/* The body of k_tread_grid and k_tread_grid_cams, and of k_stair_map and k_stair_map_cams (ssd_kernels_stairmap.hip): `where` says whose
 * staircase the block reads and which record of `out` it adds to, and writes the headers.
 * Prologue: clearance's - a thread per reported surface turns its step into the rule's record and its own frame (LDS); a thread per
 * height bin gathers the surfaces whose band, and those whose slab (height - lo .. height + lo), widened by one bin at each end,
 * overlaps the bin - supersets: the per-point rule decides; a surface whose height is a NaN holds every point in its slab (the rule's
 * comparison is negated) and is a slab candidate of every bin.
 * Per point, cheapest test first: world_z, the two tables, the slabs, then world_xy, the sides, and last the divisions for the cell. */
template<int SRC, class Where>
__device__ __forceinline__ void tread_grid_block(TreadGridLds &L, const float *__restrict__ xyz, size_t strideFloats, const PointParams &P,
                                                 const ClearanceWorld &X, const Where &where, const uint2 *__restrict__ tileMasks,
                                                 size_t tileMaskStride, int chunkPoints, const DepthSrc &D, const ssd_frame_result *__restrict__ results,
                                                 const ssd_tread_grid_rule &rule, ssd_frame_tread_grid *__restrict__ out)
{
  const int tid = threadIdx.x, lane = tid & 63;
  const int frame = blockIdx.x;
  const int at = where.index(frame);
  const double lo = rule.clearance.lo, hi = rule.clearance.hi;
  where.header(frame, tid, out);
  if(!Where::kEveryFrame && at < 0)
    return;
  const ssd_frame_result &res = where.result(results, at);
  const int nSteps = (res.status & SSD_ST_THROW) ? 0 : min(max(res.n_steps, 0), SSD_MAX_STEPS);
  if(nSteps == 0)
    return;
  const int nSlots = nSteps * kTgSlots;          /* only the frame's surfaces are zeroed and flushed */
  if(tid < nSteps)
  {
    clearance_surface(res.steps[tid], rule.clearance.margin, L.s[tid]);
    tread_grid_axes(L.s[tid], L.axes[tid]);
  }
  for(int i = tid; i < nSlots; i += kThreads)
    L.counts[i] = 0u;
  if(tid == 0)
    L.wanted = 0u;
  __syncthreads();
  if(tid < kMaxBins)
  {
    unsigned int mBand = 0u, mSlab = 0u;
    if(tid < P.nBins)
      for(int k = 0; k < nSteps; k++)
      {
        const double height = L.s[k].height, base = height - X.worldZ;
        const int bLo = clearance_bin(P, base + lo) - 1, bHi = clearance_bin(P, base + hi) + 1;
        if(L.s[k].o != 0.0 && tid >= bLo && tid <= bHi)
          mBand |= 1u << k;
        const int sLo = clearance_bin(P, base - lo) - 1, sHi = bLo + 2;       /* the bin of base + lo, and one */
        if(!(height == height) || (tid >= sLo && tid <= sHi))
          mSlab |= 1u << k;
      }
    L.band[tid] = mBand;
    L.slab[tid] = mSlab;
    if((mBand | mSlab) != 0u)
      atomicOr(&L.wanted, 1u << (tid / kBinsPerGroup));
  }
  __syncthreads();
  const unsigned int wanted = L.wanted;
  if(wanted == 0u)
    return;

  const Chunk c = chunk_of<SRC>(xyz, strideFloats, tileMasks, tileMaskStride, chunkPoints, P.nPoints);
  const CellWalk w = wanted_cells(c, 1, wanted, L.cellList, L.listScratch);
  for(int g = w.g; g < w.gEnd; g++)
  {
    const int entry = 4 * g + (lane >> 4);
    F3 v[kPts];
    load_cell<SRC>(c.base, c.cell0, L.cellList, entry, w.count, lane, P.nPoints, v, D);
    /* (a row past the end of the list holds invalid points, z = 0, which world_z drops) */
    int seenKeys[kPts];
#pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      int seenKey = -1, occKey = -1, topUnits = 0;
      double wz;
      if(world_z(P, v[j], wz))
      {
        const unsigned int bin = min(static_cast<unsigned int>(height_bin(P, wz)), static_cast<unsigned int>(kMaxBins - 1));
        const unsigned int mBand = L.band[bin];
        unsigned int mSlab = L.slab[bin];
        if((mBand | mSlab) != 0u)
        {
          const double ez = wz + X.worldZ;
          /* the slabs that hold the point, exactly: one of them and the point is no occupant */
          unsigned int inSlab = 0u;
          while(mSlab != 0u)
          {
            const int k = __builtin_ctz(mSlab);
            mSlab &= mSlab - 1u;
            if(!(__builtin_fabs(ez - L.s[k].height) > lo))
              inSlab |= 1u << k;
          }
          double wx, wy;
          if((inSlab | mBand) != 0u && world_xy(P, v[j], wx, wy))
          {
            double ex, ey;
            clearance_external(X, wx, wy, ex, ey);
            const bool tread = inSlab != 0u;
            const int k = tread ? tread_grid_lowest(L.s, inSlab, ex, ey, ez, lo) : clearance_lowest(L.s, mBand, ex, ey, ez, lo, hi);
            if(k >= 0)
            {
              int row, col, slot = k * kTgSlots + kTgCells;
              if(tread_grid_cell(L.axes[k], rule.cell, ex, ey, row, col))
                slot = k * kTgSlots + row * SSD_TG_COLS + col;
              if(tread)
                seenKey = slot;
              else
              {
                occKey = slot;
                topUnits = tread_grid_top(ez, L.s[k].height);
              }
            }
          }
        }
      }
      seenKeys[j] = seenKey;
      if(occKey >= 0 && SSD_CHK(35, occKey, nSlots))
      {
        /* the count in LDS beside the tread points'; the maximum straight to the record's word, which lies at the slot's place in the
         * surface's top plane (top_out for the slot behind the cells): occupants are rare */
        const int k = occKey / kTgSlots, cell = occKey - k * kTgSlots;
        ssd_tread_grid &G = out[at].s[k];
        atomicAdd(&L.counts[occKey], 0x10000u);
        int *const top = cell < kTgCells ? &G.top[0][0] + cell : &G.top_out;
        /* a record that many frames' blocks share (the stair map): the word is read first and the atomic sent only for a height above
         * it - a maximum only rises, so a stale read costs a redundant atomic and never a wrong byte */
        if(!Where::kSharedRecord || __hip_atomic_load(top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < topUnits)
          atomicMax(top, topUnits);
      }
    }
    tread_grid_count(L.counts, seenKeys, lane, nSlots);
  }
  __syncthreads();
  /* one global atomic per non-zero count or maximum to the block's record, which the caller zeroed on the stream (the stair map: or adds to) */
  for(int i = tid; i < nSlots; i += kThreads)
  {
    const unsigned int n = L.counts[i];
    if(n == 0u)
      continue;
    const int k = i / kTgSlots, cell = i - k * kTgSlots;
    ssd_tread_grid &G = out[at].s[k];
    const bool in = cell < kTgCells;
    const unsigned int seen = n & 0xffffu, occ = n >> 16;
    if(seen != 0u)
      atomicAdd(in ? &G.seen[0][0] + cell : &G.n_seen_out, seen);
    if(occ != 0u)
      atomicAdd(in ? &G.occ[0][0] + cell : &G.n_occ_out, occ);
  }
}

template<int SRC>
__global__ __launch_bounds__(kThreads) void k_tread_grid(const float *__restrict__ xyz, size_t strideFloats, PointParams P, ClearanceWorld X,
                                                         const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                         size_t tileMaskStride, int chunkPoints, DepthSrc D,
                                                         const ssd_frame_result *__restrict__ results, ssd_tread_grid_rule rule,
                                                         ssd_frame_tread_grid *__restrict__ out)
{
  __shared__ TreadGridLds L;
  tread_grid_block<SRC>(L, xyz, strideFloats, P, X, TreadGridOwnFrame{ st }, tileMasks, tileMaskStride, chunkPoints, D, results, rule, out);
}

/* The cameras batch's entry point, shaped like k_clearance_cams: the frame's record by scalar loads at block start, the same body. */
template<int SRC>
__global__ __launch_bounds__(kThreads) void k_tread_grid_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                              const int *__restrict__ camOf, const FrameState *__restrict__ st,
                                                              const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints,
                                                              const ssd_frame_result *__restrict__ results, ssd_tread_grid_rule rule,
                                                              ssd_frame_tread_grid *__restrict__ out)
{
  __shared__ TreadGridLds L;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const ClearanceWorld X{ { C.P.r2[0], C.P.r2[1], C.P.r2[2], C.P.r2[3] }, { C.P.t2[0], C.P.t2[1] }, C.P.worldZ };
  const DepthSrc D = C.D;
  tread_grid_block<SRC>(L, xyz, strideFloats, P, X, TreadGridOwnFrame{ st }, tileMasks, tileMaskStride, chunkPoints, D, results, rule, out);
}

/* grid and block size are launch_clearance's */
void launch_tread_grid(const Batch &B, int chunkPoints, const ssd_frame_result *results, const ssd_tread_grid_rule &rule, ssd_frame_tread_grid *out)
{
  const Params &P = B.P;
  const ClearanceWorld X{ { P.r2[0], P.r2[1], P.r2[2], P.r2[3] }, { P.t2[0], P.t2[1] }, P.worldZ };
  with_src(B, [&](auto src, const DepthSrc &D)
  {
    constexpr int SRC = decltype(src)::value;
    if(B.cams)
      hipLaunchKernelGGL((k_tread_grid_cams<SRC>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, results, rule, out);
    else
      hipLaunchKernelGGL((k_tread_grid<SRC>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, X, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, D, results, rule, out);
  });
}

} // namespace ssd
