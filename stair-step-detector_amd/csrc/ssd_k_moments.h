/* ssd_k_moments.h - stage K8 of the per-frame path, an extension: labelled_moments_block, the body of k_surface_moments (ssd_kernels.hip,
 * ssd_kernels_cams.hip) and of k_surface_refit (ssd_kernels_refit.hip).  kSurfaceSums and KeyedSums, which the riser moments and the
 * passes behind a whole enqueue use as well, stand in ssd_k_walk.h.  DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_MOMENTS_H_
#define SSD_K_MOMENTS_H_
#include "ssd_k_labels.h"

namespace ssd
{

/* ========================================================================= */
/* K8 (extension): per-surface integer moments (the surface fit)                */

/* k_labels' sibling: the same cells, the same decision (quad_decide<.., true>), and in place of a byte per point the ten integer sums
 * of ssd_ground_moments (ssd_moments.h) per surface - surface k's over exactly the points k_labels gives label k + 1 - plus n_far, the
 * labelled points the fixed-point rule leaves out.  A cell holding no bin of a live quadrilateral is neither read nor touched.
 * A lane keeps the sums of ONE surface in registers, the wave's current one (wave-uniform; rows of the camera image mostly lie on one
 * surface).  When no lane of a point slot has the current surface and some have another, the wave's sums go to the block's LDS table
 * (shuffles, then 64-bit LDS adds by lane 0) and the wave changes over; the lanes of a mixed slot that hold another surface than the
 * current one add their point to the LDS table directly.  At the block's end one 64-bit atomicAdd per non-zero entry of the table goes
 * to the frame's record, which the caller zeroed on the stream.  Integer addition throughout: no result depends on an order.
 * Camera batches: k_surface_moments_cams (ssd_kernels_cams.hip) runs this body with the frame's own constants. */
struct SurfaceLds
{
  LabelsLds l;
  unsigned long long sums[SSD_MAX_STEPS][kSurfaceSums];
};

/* The body of k_surface_moments and, GATED, of k_surface_refit (ssd_kernels_refit.hip), for one calibration and for
 * camera batches alike.  GATED: `gates` is the batch's, G the block's copy of the frame's in LDS, and on the lane's own label the gate
 * test of ssd_refit.h - a labelled point outside its surface's gate becomes an unlabelled one BEHIND the wave-uniform skip of the slots
 * that label nothing, so the three double products are spent only where some lane has a label; a point trimmed so is counted nowhere. */
template<int SRC, bool CHECKS, bool GATED>
__device__ __forceinline__ void labelled_moments_block(SurfaceLds &S, ssd_frame_gates *G, const float *__restrict__ xyz, size_t strideFloats,
                                                       const PointParams &P, const PreXY &Q, const FrameState *__restrict__ st,
                                                       const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints, const DepthSrc &D,
                                                       const ssd_frame_gates *__restrict__ gates, ssd_frame_moments *__restrict__ out)
{
  LabelsLds &L = S.l;
  const int tid = threadIdx.x, lane = tid & 63;
  const int frame = blockIdx.x;
  const LiveFrame f = labels_stage(L, st[frame], P, Q);
  if(f.live)
  {
    if constexpr(GATED)
    {
      /* the frame's gates: 86 words, once per block */
      static_assert(sizeof(ssd_frame_gates) % 8 == 0 && sizeof(ssd_frame_gates) / 8 <= kThreads, "one thread per 64-bit word of the frame's gates");
      if(tid < static_cast<int>(sizeof(ssd_frame_gates) / 8))
        reinterpret_cast<unsigned long long *>(G)[tid] = reinterpret_cast<const unsigned long long *>(gates + frame)[tid];
    }
    /* the record's header, by the frame's first block: the surfaces labels can name, and whether the first is the ground */
    if(tid == 0 && blockIdx.y == 0)
    {
      out[frame].n_surfaces = min(f.nLive, SSD_MAX_STEPS);
      out[frame].ground = f.gSlot >= 0 ? 1 : 0;
    }
  }
  if(tid < SSD_MAX_STEPS * kSurfaceSums)
    (&S.sums[0][0])[tid] = 0ull;
  __syncthreads();
  if(f.wanted == 0u)
    return;

  const Chunk c = chunk_of<SRC>(xyz, strideFloats, tileMasks, tileMaskStride, chunkPoints, P.nPoints);
  const CellWalk w = wanted_cells(c, 1, f.wanted, L.cellList, L.listScratch);
  const PreLane lc(Q);
  KeyedSums<kSurfaceSums> sums;                  /* keyed by the surface: the label - 1 */
  for(int g = w.g; g < w.gEnd; g++)
  {
    const int entry = 4 * g + (lane >> 4);
    F3 v[kPts];
    load_cell<SRC>(c.base, c.cell0, L.cellList, entry, w.count, lane, P.nPoints, v, D);
#pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      const unsigned int lab = label_of<CHECKS>(v[j], Q, lc, L);
      int k = entry < w.count ? static_cast<int>(lab) - 1 : -1;
      if(__ballot(k >= 0) == 0ull)               /* wave-uniform: a slot none of whose points is labelled */
        continue;
      if constexpr(GATED)
        k = (k >= 0 && refit_keeps(*G, k, v[j].x, v[j].y, v[j].z)) ? k : -1;
      const unsigned long long mKeyed = __ballot(k >= 0);
      if(mKeyed == 0ull)                         /* wave-uniform: every labelled point of the slot was trimmed */
        continue;
      sums.changeover(k, mKeyed, S.sums, lane);
      sums.add(k, v[j], S.sums);
    }
  }
  sums.flush(S.sums, lane);
  __syncthreads();
  /* one 64-bit atomicAdd per non-zero entry to the frame's record, which the caller zeroed on the stream */
  keyed_sums_give<kSurfaceSums>(S.sums, SSD_MAX_STEPS, [&](int k, int i, unsigned long long t)
  {
    atomicAdd(reinterpret_cast<unsigned long long *>(out + frame) + 1 + k * kSurfaceSums + i, t);
  });
}

} // namespace ssd

#endif /* SSD_K_MOMENTS_H_ */
