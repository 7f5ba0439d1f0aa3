/* ssd_k_risers.h - stage K6 of the per-frame path, an extension: the three riser passes (k_risers, k_riser_moments, k_riser_labels) and
 * k_riser_results.  k_riser_results is no template: where this header is included decides its place among the unit's kernels, which
 * ssd_kernels.hip keeps last (the ordering rule). */
#ifndef SSD_K_RISERS_H_
#define SSD_K_RISERS_H_
#include "ssd_k_walk.h"
#include "ssd_k_windows.h"

namespace ssd
{

/* ========================================================================= */
/* K6 (extension): evidence of the vertical faces                              */

/* What the three riser passes share: the block's copy of the frame's riser state with the cell list, the way into the walk, and the
 * evidence rule.  Each kernel's own table lies beside or behind the record. */
struct RiserLds
{
  unsigned short cellList[kMaxCellsPerBlock];
  unsigned int listScratch[2 * kWavesPerBlock];
  RiserState rs[kMaxRisers];
  signed char riserOfBin[kMaxBins];
};

/* false for a frame without risers (block-uniform: wantedRisers is set by k_final); else the frame's riser state in L, behind a barrier
 * (what the caller zeroed in front of the call is zero behind it), and the chunk's cells that hold a bin of a riser, which alone are
 * walked (as k_raster / k_inquad).  fs.nRisers is k_final's count of emitted surfaces less one: at most kMaxRisers. */
template<int SRC>
__device__ __forceinline__ bool riser_walk(RiserLds &L, const FrameState &fs, const float *__restrict__ xyz, size_t strideFloats, int nPoints,
                                           const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints, int cellCols, Chunk &c, CellWalk &w)
{
  const int tid = threadIdx.x;
  const unsigned int wanted = fs.wantedRisers;
  if(wanted == 0u)
    return false;
  if(tid < kMaxBins)
    L.riserOfBin[tid] = fs.riserOfBin[tid];
  if(tid < fs.nRisers)
    L.rs[tid] = fs.riser[tid];
  __syncthreads();
  c = chunk_of<SRC>(xyz, strideFloats, tileMasks, tileMaskStride, chunkPoints, nPoints);
  w = wanted_cells(c, cellCols, wanted, L.cellList, L.listScratch);
  return true;
}

/* The evidence rule: then(r, sd) for a point that is evidence of riser r, sd its signed distance from the riser's edge line; nothing
 * for any other point.  The point's height lies in a bin of the riser (a bin of no plateau between the two surfaces) and strictly inside
 * its band, the point within tol of the edge line and along the edge.  (load_points gives a point beyond nPoints z = 0, and world_z
 * drops it: an evidence point lies inside the frame.)  The caller's continuation and not a returned index: returned, the 16-bit depth
 * k_risers spills 42 scalar registers to lanes for 27 and runs a third longer (profiles/extension_kernels_shared.txt). */
template<typename Then>
__device__ __forceinline__ void riser_evidence(const PointParams &P, const F3 &p, const RiserLds &L, double tol, Then then)
{
  double wx, wy, wz;
  if(!world_z(P, p, wz))
    return;
  const int r = L.riserOfBin[height_bin(P, wz)];
  if(r < 0)
    return;
  const RiserState &R = L.rs[r];
  if(!(wz > R.zLo && wz < R.zHi))
    return;
  if(!world_xy(P, p, wx, wy))
    return;
  const double a = wx - R.ox, b = wy - R.oy;
  const double sd = b * R.ux - a * R.uy;                 /* signed distance from the edge line */
  const double t = a * R.ux + b * R.uy;                  /* position along the edge */
  if(fabs(sd) <= tol && t >= 0.0 && t <= R.len)
    then(r, sd);
}

template<int SRC>
SSD_ENTRY(__launch_bounds__(kThreads, 8), k_risers, risers_block)(const float *__restrict__ xyz, size_t strideFloats, SSD_BYVAL(PointParams) P, double tol,
                                                        FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                        size_t tileMaskStride, int chunkPoints, int cellCols, SSD_BYVAL(DepthSrc) D)
{
  __shared__ RiserLds L;
  __shared__ unsigned long long lsum[kMaxRisers][8];
  __shared__ unsigned int lcnt[kMaxRisers][8];

  const int tid = threadIdx.x, lane = tid & 63;
  FrameState &fs = st[blockIdx.x];
  for(int i = tid; i < kMaxRisers * 8; i += kThreads)
  {
    (&lsum[0][0])[i] = 0ull;
    (&lcnt[0][0])[i] = 0u;
  }
  Chunk c;
  CellWalk w;
  if(!riser_walk<SRC>(L, fs, xyz, strideFloats, P.nPoints, tileMasks, tileMaskStride, chunkPoints, cellCols, c, w))
    return;

  const int copy = lane & 7;
  int curR = -1;
  long long accS = 0;
  unsigned int accN = 0;
  auto flushAcc = [&]()
  {
    if(curR >= 0 && accN)
    {
      atomicAdd(&lsum[curR][copy], static_cast<unsigned long long>(accS));
      atomicAdd(&lcnt[curR][copy], accN);
    }
  };
  for(int g = w.g; g < w.gEnd; g++)
  {
    F3 v[kPts];
    load_cell<SRC>(c.base, c.cell0, L.cellList, 4 * g + (lane >> 4), w.count, lane, P.nPoints, v, D);
    #pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      riser_evidence(P, v[j], L, tol, [&](int r, double sd)
      {
        if(r != curR)
        {
          flushAcc();
          curR = r; accS = 0; accN = 0;
        }
        accS += z_to_fixed(sd);
        accN++;
      });
    }
  }
  flushAcc();
  __syncthreads();
  if(tid < fs.nRisers)
  {
    unsigned long long sum = 0;
    unsigned int n = 0;
    for(int k = 0; k < 8; k++)
    {
      sum += lsum[tid][k];
      n += lcnt[tid][k];
    }
    if(n)
    {
      atomicAdd(reinterpret_cast<unsigned long long *>(&fs.rSum[tid]), sum);
      atomicAdd(&fs.rCnt[tid], n);
    }
  }
}

/* k_risers' sibling (the riser fit): the same walk (riser_walk) and the same evidence rule (riser_evidence), walked
 * ONCE, and beside the count and the offset sum of every riser the ten integer sums of ssd_ground_moments (ssd_moments.h) over its evidence
 * points plus n_far, the evidence points the fixed-point rule leaves out - riser i's in record s[i] of the frame's ssd_frame_moments.
 * Accumulation is k_surface_moments' (KeyedSums, keyed by the riser) with one more sum, the offset's.  At the block's end one 64-bit
 * atomicAdd per non-zero entry goes to the frame's record, which the caller zeroed on the stream, and to k_risers' own rSum / rCnt (the
 * count is n + n_far).  Integer addition throughout: no result depends on an order, and rSum / rCnt are what k_risers leaves.
 * Camera batches: k_riser_moments_cams (ssd_kernels_cams.hip) runs this body with the frame's own constants. */
constexpr int kRiserSums = kSurfaceSums + 1;        /* the eleven int64 of ssd_surface_moments, then the offset sum (2^-40 m) */
constexpr int kRiserOffsetSum = kSurfaceSums;
static_assert(kMaxRisers <= SSD_MAX_STEPS, "riser i's sums are record s[i] of an ssd_frame_moments");
static_assert(kMaxRisers * kRiserSums <= kThreads, "one thread per entry of the block's table");

struct RiserMomentsLds
{
  RiserLds r;
  unsigned long long sums[kMaxRisers][kRiserSums];
};

template<int SRC>
SSD_ENTRY(__launch_bounds__(kThreads), k_riser_moments, riser_moments_block)(const float *__restrict__ xyz, size_t strideFloats, SSD_BYVAL(PointParams) P, double tol,
                                                        FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                        size_t tileMaskStride, int chunkPoints, int cellCols, SSD_BYVAL(DepthSrc) D,
                                                        ssd_frame_moments *__restrict__ out)
{
  __shared__ RiserMomentsLds S;

  const int tid = threadIdx.x, lane = tid & 63;
  const int frame = blockIdx.x;
  FrameState &fs = st[frame];
  const int nR = fs.nRisers;
  /* the record's header, by the frame's first block (also of a frame none of whose cells holds a riser's bin) */
  if(blockIdx.y == 0 && tid == 0)
  {
    out[frame].n_surfaces = nR;
    out[frame].ground = 0;
  }
  if(tid < kMaxRisers * kRiserSums)
    (&S.sums[0][0])[tid] = 0ull;
  Chunk c;
  CellWalk w;
  if(!riser_walk<SRC>(S.r, fs, xyz, strideFloats, P.nPoints, tileMasks, tileMaskStride, chunkPoints, cellCols, c, w))
    return;

  KeyedSums<kRiserSums> sums;                    /* keyed by the riser */
  for(int g = w.g; g < w.gEnd; g++)
  {
    F3 v[kPts];
    load_cell<SRC>(c.base, c.cell0, S.r.cellList, 4 * g + (lane >> 4), w.count, lane, P.nPoints, v, D);
#pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      int r = -1;                                /* the point's riser, -1: no evidence */
      long long sdFix = 0;
      riser_evidence(P, v[j], S.r, tol, [&](int rb, double sd) { r = rb; sdFix = z_to_fixed(sd); });
      const unsigned long long mEv = __ballot(r >= 0);
      if(mEv == 0ull)                            /* wave-uniform: a slot none of whose points is evidence */
        continue;
      sums.changeover(r, mEv, S.sums, lane);
      sums.add(r, v[j], S.sums);
      /* the offset sum beside the moments */
      if(r == sums.cur)
        sums.acc[kRiserOffsetSum] += sdFix;
      else if(r >= 0)
        atomicAdd(&S.sums[r][kRiserOffsetSum], static_cast<unsigned long long>(sdFix));
    }
  }
  sums.flush(S.sums, lane);
  __syncthreads();
  /* one 64-bit atomicAdd per non-zero entry to the frame's record, which the caller zeroed on the stream, and to k_risers' own sums */
  keyed_sums_give<kRiserSums>(S.sums, nR, [&](int r, int i, unsigned long long t)
  {
    if(i == kRiserOffsetSum)
      atomicAdd(reinterpret_cast<unsigned long long *>(&fs.rSum[r]), t);
    else
    {
      atomicAdd(reinterpret_cast<unsigned long long *>(out + frame) + 1 + r * kSurfaceSums + i, t);
      if(i == 0 || i == kGroundSums)             /* every evidence point is in n or in n_far */
        atomicAdd(&fs.rCnt[r], static_cast<unsigned int>(t));
    }
  });
}

/* The riser labels (ssd_set_riser_labels): k_risers' cells (riser_walk) and k_risers' evidence rule (riser_evidence),
 * and in place of any sum one byte per evidence point, SSD_LABEL_RISER_BASE + r, at the index k_labels gives the point.  It runs behind
 * k_labels on the same stream, which has written every byte of the frame; an evidence point's bin is a bin of no plateau, so its byte
 * is a zero of k_labels' and belongs to this lane alone: single byte stores, nothing read, nothing else rewritten (the neighbouring
 * bytes are other lanes').  No sums, no atomics, no LDS beyond the frame's riser state and the cell list.  Camera batches:
 * k_riser_labels_cams (ssd_kernels_cams.hip) runs this body with the frame's own constants. */
static_assert(SSD_LABEL_RISER_BASE > SSD_MAX_STEPS && SSD_LABEL_RISER_BASE + kMaxRisers - 1 <= 0xff, "surface and riser labels share a byte");

template<int SRC>
SSD_ENTRY(__launch_bounds__(kThreads, 8), k_riser_labels, riser_labels_block)(const float *__restrict__ xyz, size_t strideFloats, SSD_BYVAL(PointParams) P, double tol,
                                                        const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                        size_t tileMaskStride, int chunkPoints, int cellCols, SSD_BYVAL(DepthSrc) D,
                                                        unsigned char *__restrict__ labels, size_t labelStride)
{
  __shared__ RiserLds L;

  const int lane = threadIdx.x & 63;
  const int frame = blockIdx.x;
  Chunk c;
  CellWalk w;
  if(!riser_walk<SRC>(L, st[frame], xyz, strideFloats, P.nPoints, tileMasks, tileMaskStride, chunkPoints, cellCols, c, w))
    return;
  unsigned char *row = labels + static_cast<size_t>(frame) * labelStride;
  for(int g = w.g; g < w.gEnd; g++)
  {
    const int entry = 4 * g + (lane >> 4);
    F3 v[kPts];
    load_cell<SRC>(c.base, c.cell0, L.cellList, entry, w.count, lane, P.nPoints, v, D);
    if(entry >= w.count)                                    /* a row past the end of the list: its points are invalid, its cell is nobody's */
      continue;
    const int idx = (c.cell0 + static_cast<int>(L.cellList[entry])) * kCell + kPts * (lane & 15);
    #pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      riser_evidence(P, v[j], L, tol, [&](int r, double)
      {
        if(SSD_CHK(33, idx + j, P.nPoints))
          row[idx + j] = static_cast<unsigned char>(SSD_LABEL_RISER_BASE + r);
      });
    }
  }
}

/* one thread per frame: the riser records in external world coordinates (ToExternalWorld as in k_final) */
SSD_ENTRY(, k_riser_results, riser_results_block)(SSD_BYVAL(Params) P, const FrameState *__restrict__ st, ssd_frame_risers *__restrict__ out, int nframes)
{
  const int frame = blockIdx.x * blockDim.x + threadIdx.x;
  if(frame >= nframes)
    return;
  const FrameState &fs = st[frame];
  ssd_frame_risers &o = out[frame];
  const int nR = fs.nRisers;
  o.n_risers = nR;
  o.reserved = 0;
  for(int i = 0; i < kMaxRisers; i++)
  {
    ssd_riser &q = o.risers[i];
    if(i >= nR)
    {
      q.n_points = 0; q.detected = 0; q.height_bottom = 0.0; q.height_top = 0.0;
      q.left[0] = q.left[1] = q.right[0] = q.right[1] = 0.0; q.mean_offset = 0.0;
      continue;
    }
    const RiserState &R = fs.riser[i];
    const unsigned int c = fs.rCnt[i];
    q.n_points = static_cast<int>(c);
    q.detected = c >= static_cast<unsigned int>(P.riserMinSupport) ? 1 : 0;
    q.height_bottom = P.worldZ + R.zBottom;
    q.height_top = P.worldZ + R.zTop;
    double ex = P.r2[0] * R.leftX + P.r2[1] * R.leftY, ey = P.r2[2] * R.leftX + P.r2[3] * R.leftY;
    q.left[0] = ex + P.t2[0]; q.left[1] = ey + P.t2[1];
    ex = P.r2[0] * R.rightX + P.r2[1] * R.rightY; ey = P.r2[2] * R.rightX + P.r2[3] * R.rightY;
    q.right[0] = ex + P.t2[0]; q.right[1] = ey + P.t2[1];
    q.mean_offset = c ? (static_cast<double>(fs.rSum[i]) / static_cast<double>(1ll << kZFixShift)) / c : 0.0;
  }
}

} // namespace ssd

#endif /* SSD_K_RISERS_H_ */
