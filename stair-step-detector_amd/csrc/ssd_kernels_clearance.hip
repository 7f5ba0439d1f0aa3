/*
 * ssd_kernels_clearance.hip - the tread clearance pass (ssd_enqueue_clearance, ssd_enqueue_cameras_clearance) and
 * its launcher.
 *
 * What stands ON each reported surface: the points of no plateau - the reference's `remainder`, which it drops - that lie in a band above a
 * surface's height and inside its quadrilateral shrunk by a margin (the rule: ssd_clearance.h, one text with ssd_clearance_host).  The pass
 * reads the frame's RESULT record as k_final wrote it, K1's cell records and the points again; it writes the caller's two buffers alone.
 * The walk is the extension kernels' (chunk_of, wanted_cells, KeyedSums: ssd_k_walk.h; load_cell: ssd_k_cells.h), keyed by the surface.
 * The file includes that header, the launch rules and its own rule, and no kernel of the chain.  The build compiles it at the end of
 * ssd_kernels_refit.hip: the passes that run behind a whole enqueue are one translation unit, and what they share is parsed once.
 */
#include "ssd_k_walk.h"
#include "ssd_launch_rules.h"
#include "ssd_clearance.h"

namespace ssd
{

static_assert(SSD_MAX_STEPS <= 32, "a bin's candidate surfaces are a 32-bit mask");

struct ClearanceLds
{
  unsigned short cellList[kMaxCellsPerBlock];
  unsigned int listScratch[2 * kWavesPerBlock];
  ClearanceSurface s[SSD_MAX_STEPS];             /* the frame's reported surfaces as the rule reads them */
  unsigned int cand[kMaxBins];                   /* height bin -> the surfaces whose band may hold a point of the bin (a superset) */
  unsigned int wanted;                           /* the bin groups with a candidate */
  unsigned long long sums[SSD_MAX_STEPS][kSurfaceSums];
};

/* the bin of a camera-dependent world height, clamped into the histogram (a NaN: bin 0) */
__device__ __forceinline__ int clearance_bin(const PointParams &P, double wz)
{
  const double t = (wz - P.zMin) * P.recip;
  return !(t >= 0.0) ? 0 : t >= static_cast<double>(P.nBins - 1) ? P.nBins - 1 : static_cast<int>(t);
}

/* The body of k_clearance and k_clearance_cams, for one calibration and for camera batches alike.
 * Prologue: a thread per reported surface turns its step into the rule's record (LDS); a thread per height bin gathers the surfaces whose
 * band (height + lo, height + hi), widened by one bin at each end, overlaps the bin - a superset: the per-point rule decides - and the
 * bin groups of those bins make the block's `wanted` mask against K1's cell records.
 * Per point, cheapest test first: world_z (validity, the z row, the z range), the table, the slabs, then world_xy and the sides.
 * MASK: one byte store per occupant, k + 1, at the index k_labels gives the point; the caller zeroed the mask, every other byte stays. */
template<int SRC, bool MASK>
__device__ __forceinline__ void clearance_block(ClearanceLds &L, const float *__restrict__ xyz, size_t strideFloats, const PointParams &P,
                                                const ClearanceWorld &X, const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                size_t tileMaskStride, int chunkPoints, const DepthSrc &D, const ssd_frame_result *__restrict__ results,
                                                const ssd_clearance_rule &rule, ssd_frame_moments *__restrict__ out, unsigned char *__restrict__ mask,
                                                size_t maskStride)
{
  const int tid = threadIdx.x, lane = tid & 63;
  const int frame = blockIdx.x;
  const FrameState &fs = st[frame];
  const ssd_frame_result &res = results[frame];
  /* the record's header as k_surface_moments writes it, from the same FrameState, by the frame's first block */
  const bool live = fs.anyActive != 0u && (fs.status & SSD_ST_THROW) == 0u;
  if(live && tid == 0 && blockIdx.y == 0)
  {
    const int nLive = fs.nLive;
    out[frame].n_surfaces = min(nLive, SSD_MAX_STEPS);
    out[frame].ground = (nLive > 0 && fs.accActive[kGroundAcc]) ? 1 : 0;
  }
  /* a frame the reference would have thrown on, or without a surface, has no occupant (block-uniform) */
  const int nSteps = (res.status & SSD_ST_THROW) ? 0 : min(max(res.n_steps, 0), SSD_MAX_STEPS);
  if(nSteps == 0)
    return;
  if(tid < nSteps)
    clearance_surface(res.steps[tid], rule.margin, L.s[tid]);
  if(tid < SSD_MAX_STEPS * kSurfaceSums)
    (&L.sums[0][0])[tid] = 0ull;
  if(tid == 0)
    L.wanted = 0u;
  __syncthreads();
  if(tid < kMaxBins)
  {
    unsigned int m = 0u;
    if(tid < P.nBins)
      for(int k = 0; k < nSteps; k++)
      {
        /* the band in camera-dependent world heights (ez = wz + world_z), one bin wider at each end: rounding cannot lose a point */
        const double base = L.s[k].height - X.worldZ;
        const int bLo = clearance_bin(P, base + rule.lo) - 1, bHi = clearance_bin(P, base + rule.hi) + 1;
        if(L.s[k].o != 0.0 && tid >= bLo && tid <= bHi)
          m |= 1u << k;
      }
    L.cand[tid] = m;
    if(m != 0u)
      atomicOr(&L.wanted, 1u << (tid / kBinsPerGroup));
  }
  __syncthreads();
  const unsigned int wanted = L.wanted;
  if(wanted == 0u)
    return;

  const Chunk c = chunk_of<SRC>(xyz, strideFloats, tileMasks, tileMaskStride, chunkPoints, P.nPoints);
  const CellWalk w = wanted_cells(c, 1, wanted, L.cellList, L.listScratch);
  unsigned char *row = MASK ? mask + static_cast<size_t>(frame) * maskStride : nullptr;
  KeyedSums<kSurfaceSums> sums;                  /* keyed by the surface */
  for(int g = w.g; g < w.gEnd; g++)
  {
    const int entry = 4 * g + (lane >> 4);
    F3 v[kPts];
    load_cell<SRC>(c.base, c.cell0, L.cellList, entry, w.count, lane, P.nPoints, v, D);
    /* (a row past the end of the list holds invalid points, z = 0, which world_z drops: its cell index is never used) */
    const int idx = entry < w.count ? (c.cell0 + static_cast<int>(L.cellList[entry])) * kCell + kPts * (lane & 15) : 0;
#pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      int k = -1;                                /* the surface the point occupies, -1: none */
      double wz;
      if(world_z(P, v[j], wz))
      {
        const unsigned int m = L.cand[min(static_cast<unsigned int>(height_bin(P, wz)), static_cast<unsigned int>(kMaxBins - 1))];
        const double ez = wz + X.worldZ;
        double wx, wy;
        if(m != 0u && !clearance_in_slab(L.s, nSteps, ez, rule.lo) && world_xy(P, v[j], wx, wy))
        {
          double ex, ey;
          clearance_external(X, wx, wy, ex, ey);
          k = clearance_lowest(L.s, m, ex, ey, ez, rule.lo, rule.hi);
        }
      }
      const unsigned long long mKeyed = __ballot(k >= 0);
      if(mKeyed == 0ull)                         /* wave-uniform: a slot none of whose points is an occupant */
        continue;
      sums.changeover(k, mKeyed, L.sums, lane);
      sums.add(k, v[j], L.sums);
      if constexpr(MASK)
      {
        if(k >= 0 && SSD_CHK(34, idx + j, P.nPoints))
          row[idx + j] = static_cast<unsigned char>(k + 1);
      }
    }
  }
  sums.flush(L.sums, lane);
  __syncthreads();
  /* one 64-bit atomicAdd per non-zero entry to the frame's record, which the caller zeroed on the stream */
  keyed_sums_give<kSurfaceSums>(L.sums, SSD_MAX_STEPS, [&](int k, int i, unsigned long long t)
  {
    atomicAdd(reinterpret_cast<unsigned long long *>(out + frame) + 1 + k * kSurfaceSums + i, t);
  });
}

template<int SRC, bool MASK>
__global__ __launch_bounds__(kThreads) void k_clearance(const float *__restrict__ xyz, size_t strideFloats, PointParams P, ClearanceWorld X,
                                                        const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                        size_t tileMaskStride, int chunkPoints, DepthSrc D,
                                                        const ssd_frame_result *__restrict__ results, ssd_clearance_rule rule,
                                                        ssd_frame_moments *__restrict__ out, unsigned char *__restrict__ mask, size_t maskStride)
{
  __shared__ ClearanceLds L;
  clearance_block<SRC, MASK>(L, xyz, strideFloats, P, X, st, tileMasks, tileMaskStride, chunkPoints, D, results, rule, out, mask, maskStride);
}

/* The cameras batch's entry point, shaped like k_surface_refit_cams: the frame's record by scalar loads at block start, the parts the
 * body uses copied, the same body. */
template<int SRC, bool MASK>
__global__ __launch_bounds__(kThreads) void k_clearance_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                             const int *__restrict__ camOf, const FrameState *__restrict__ st,
                                                             const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints,
                                                             const ssd_frame_result *__restrict__ results, ssd_clearance_rule rule,
                                                             ssd_frame_moments *__restrict__ out, unsigned char *__restrict__ mask, size_t maskStride)
{
  __shared__ ClearanceLds L;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const ClearanceWorld X{ { C.P.r2[0], C.P.r2[1], C.P.r2[2], C.P.r2[3] }, { C.P.t2[0], C.P.t2[1] }, C.P.worldZ };
  const DepthSrc D = C.D;
  clearance_block<SRC, MASK>(L, xyz, strideFloats, P, X, st, tileMasks, tileMaskStride, chunkPoints, D, results, rule, out, mask, maskStride);
}

/* grid and block size are launch_surface_refit's; the pass has no pre-filter, so no CHECKS instantiations.  A cameras batch: B.depthInput
 * only says that the source is 16-bit depth - each frame's DepthSrc is its camera's */
void launch_clearance(const Batch &B, int chunkPoints, const ssd_frame_result *results, const ssd_clearance_rule &rule, ssd_frame_moments *out,
                      unsigned char *mask, size_t maskStride)
{
  const Params &P = B.P;
  const ClearanceWorld X{ { P.r2[0], P.r2[1], P.r2[2], P.r2[3] }, { P.t2[0], P.t2[1] }, P.worldZ };
  with_src(B, [&](auto src, const DepthSrc &D)
  {
    with_bool(mask != nullptr, [&](auto withMask)
    {
      constexpr int SRC = decltype(src)::value;
      constexpr bool MASK = decltype(withMask)::value;
      if(B.cams)
        hipLaunchKernelGGL((k_clearance_cams<SRC, MASK>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, results, rule, out, mask, maskStride);
      else
        hipLaunchKernelGGL((k_clearance<SRC, MASK>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, X, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, D, results, rule, out, mask, maskStride);
    });
  });
}

} // namespace ssd
