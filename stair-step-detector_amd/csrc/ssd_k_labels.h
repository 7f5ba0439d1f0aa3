/* ssd_k_labels.h - stage K7 of the per-frame path, an extension: k_labels / labels_block, and the staging of a frame's live state
 * (LabelsLds, labels_stage, label_of) that K8 and the refit take from it.  DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_LABELS_H_
#define SSD_K_LABELS_H_
#include "ssd_k_decide.h"
#include "ssd_k_walk.h"

namespace ssd
{

/* ========================================================================= */
/* K7 (extension): per-pixel surface labels                                    */

/* Label of point i of a frame (= camera pixel v W + u): k + 1 if the point is one of those whose mean is surface k of the frame's
 * result (ground first, then the valid steps ascending: k_final's order), else 0 (include/ssd_hip.h, SSD_LABEL_NONE).  That is
 * k_inquad's decision taken for every point of a live quadrilateral's bins: quad_decide<.., true>.  Runs after k_final (it reads
 * the frame's status) on the same FrameState; writes every byte of [0, W H) of the frame's row once, nothing else. */
struct LabelsLds
{
  QuadTest qts[kMaxLive];                       /* as InquadLds */
  QuadEdgesF edges[kMaxLive + 1];
  K1Consts kc;
  unsigned char lut[kMaxBins];                  /* bin -> live slot, kMaxLive = none */
  unsigned char label[kMaxLive + 1];            /* live slot -> label (the surface's place in the result + 1); row kMaxLive: 0 */
  unsigned short cellList[kMaxCellsPerBlock];
  unsigned int listScratch[2 * kWavesPerBlock];
};

/* four labels of the points idx .. idx + 3 (idx a multiple of 4): one 32-bit store where the row is 4-byte aligned and whole */
__device__ __forceinline__ void store_labels4(unsigned char *__restrict__ row, bool aligned4, int idx, int nPoints, unsigned int word)
{
  if(aligned4 && idx + 4 <= nPoints)
    *reinterpret_cast<unsigned int *>(row + idx) = word;
  else
  {
#pragma unroll
    for(int k = 0; k < 4; k++)
      if(idx + k < nPoints)
        row[idx + k] = static_cast<unsigned char>(word >> (8 * k));
  }
}

/* The frame's live state into the block's LabelsLds, for every kernel that takes k_inquad's decision once more (quad_decide<.., true>);
 * the caller's barrier follows.  Nothing of a frame k_quads found no live quadrilateral in, or whose quadrilaterals the reference would
 * have thrown on, is labelled: wanted = 0 then (block-uniform), and nothing is staged. */
struct LiveFrame
{
  bool live;
  unsigned int wanted;                          /* the bin groups of the live quadrilaterals */
  int nLive, gSlot;                             /* the live slots, and the ground's among them (-1: none) */
};
__device__ __forceinline__ LiveFrame labels_stage(LabelsLds &L, const FrameState &fs, const PointParams &P, const PreXY &Q)
{
  const int tid = threadIdx.x;
  LiveFrame f;
  f.live = fs.anyActive != 0u && (fs.status & SSD_ST_THROW) == 0u;
  f.wanted = f.live ? fs.wantedQuads : 0u;
  f.nLive = 0;
  f.gSlot = -1;
  if(f.live)
  {
    f.nLive = fs.nLive;
    f.gSlot = (f.nLive > 0 && fs.accActive[kGroundAcc]) ? f.nLive - 1 : -1;           /* the ground is the last live slot */
    if(tid < kMaxBins)
    {
      const unsigned char s = fs.lutLive[tid];
      L.lut[tid] = s == 0xff ? static_cast<unsigned char>(kMaxLive) : s;
    }
    if(tid <= kMaxLive)
    {
      /* slot order = accumulator order (treads ascending, the ground last); the result has the ground first */
      int lab = 0;
      if(tid < f.nLive)
        lab = tid == f.gSlot ? 1 : tid + 1 + (f.gSlot >= 0 ? 1 : 0);
      L.label[tid] = static_cast<unsigned char>(lab <= SSD_MAX_STEPS ? lab : 0);
    }
    constexpr int qtWords = kMaxLive * static_cast<int>(sizeof(QuadTest) / 4);
    constexpr int egWords = kMaxLive * static_cast<int>(sizeof(QuadEdgesF) / 4);
    for(int w = tid; w < qtWords; w += kThreads)
      reinterpret_cast<unsigned int *>(L.qts)[w] = reinterpret_cast<const unsigned int *>(fs.qtLive)[w];
    stage_quad_edges(L.edges, fs.edgeLive, egWords, Q.dE0);
    if(tid == 0)
      k1_consts_fill(L.kc, P, nullptr);
  }
  return f;
}

/* the point's label by the decision of quad_decide<.., true>: the live slot's, 0 where the point is in none */
template<bool CHECKS>
__device__ __forceinline__ unsigned int label_of(const F3 &p, const PreXY &Q, const PreLane lc, const LabelsLds &L)
{
  f32x2 d;
  float M, M3;
  unsigned int q;
  unsigned long long mSlow, mIn, mGround;
  quad_decide<CHECKS, true>(p, Q, lc, L.edges, L.lut, L.qts, L.kc, -1, d, M, M3, q, mSlow, mIn, mGround);
  return __builtin_amdgcn_inverse_ballot_w64(mIn) ? L.label[min(q, static_cast<unsigned int>(kMaxLive))] : 0u;
}

template<int SRC, bool CHECKS>
SSD_ENTRY(__launch_bounds__(kThreads), k_labels, labels_block)(const float *__restrict__ xyz, size_t strideFloats, SSD_BYVAL(PointParams) P, SSD_BYVAL(PreXY) Q,
                                                     const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                     size_t tileMaskStride, int chunkPoints, SSD_BYVAL(DepthSrc) D,
                                                     unsigned char *__restrict__ labels, size_t labelStride)
{
  __shared__ LabelsLds L;
  const int tid = threadIdx.x, lane = tid & 63;
  const int frame = blockIdx.x;
  /* labels_stage's text, and not a call of it: staged through the function this kernel takes 95 scalar registers for 71 and its
   * 16-bit depth instantiations 5 to 8 % longer on an MI355X (profiles/extension_kernels_shared.txt) */
  const FrameState &fs = st[frame];
  const bool live = fs.anyActive != 0u && (fs.status & SSD_ST_THROW) == 0u;
  const unsigned int wanted = live ? fs.wantedQuads : 0u;
  if(live)
  {
    const int nLive = fs.nLive;
    const int gSlot = (nLive > 0 && fs.accActive[kGroundAcc]) ? nLive - 1 : -1;
    if(tid < kMaxBins)
    {
      const unsigned char s = fs.lutLive[tid];
      L.lut[tid] = s == 0xff ? static_cast<unsigned char>(kMaxLive) : s;
    }
    if(tid <= kMaxLive)
    {
      int lab = 0;
      if(tid < nLive)
        lab = tid == gSlot ? 1 : tid + 1 + (gSlot >= 0 ? 1 : 0);
      L.label[tid] = static_cast<unsigned char>(lab <= SSD_MAX_STEPS ? lab : 0);
    }
    constexpr int qtWords = kMaxLive * static_cast<int>(sizeof(QuadTest) / 4);
    constexpr int egWords = kMaxLive * static_cast<int>(sizeof(QuadEdgesF) / 4);
    for(int w = tid; w < qtWords; w += kThreads)
      reinterpret_cast<unsigned int *>(L.qts)[w] = reinterpret_cast<const unsigned int *>(fs.qtLive)[w];
    stage_quad_edges(L.edges, fs.edgeLive, egWords, Q.dE0);
    if(tid == 0)
    {
      K1Consts &c = L.kc;
      for(int i = 0; i < 9; i++)
        c.a[i] = P.a[i];
      c.b[0] = P.b[0]; c.b[1] = P.b[1]; c.b[2] = P.b[2];
      c.xMin = P.xMin; c.xMax = P.xMax; c.yMin = P.yMin; c.yMax = P.yMax; c.zMin = P.zMin; c.zMax = P.zMax;
      c.boxX = P.boxX; c.boxY = P.boxY;
      c.recip = P.recip;
      c.xToImage = 0.0; c.yToImage = 0.0;
    }
  }
  __syncthreads();

  const Chunk c = chunk_of<SRC>(xyz, strideFloats, tileMasks, tileMaskStride, chunkPoints, P.nPoints);
  unsigned char *row = labels + static_cast<size_t>(frame) * labelStride;

  /* the cells that hold no bin of a live quadrilateral: zeros, without a look at their points (16 bytes a lane where the row allows) */
  const bool aligned16 = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
  constexpr int kUnits = kCell / 16;
  for(int u = tid; u < c.nCells * kUnits; u += kThreads)
  {
    const int cell = u / kUnits;
    if((c.cells[cell].x & wanted) != 0u)
      continue;
    const int idx = (c.cell0 + cell) * kCell + 16 * (u - cell * kUnits);
    if(aligned16 && idx + 16 <= P.nPoints)
      *reinterpret_cast<uint4 *>(row + idx) = make_uint4(0u, 0u, 0u, 0u);
    else
      for(int k = 0; k < 16 && idx + k < P.nPoints; k++)
        row[idx + k] = 0;
  }
  if(wanted == 0u)
    return;

  /* the others, in order (one column of cells: the list is the chunk's cells ascending), four cells per wave iteration */
  const CellWalk w = wanted_cells(c, 1, wanted, L.cellList, L.listScratch);
  const bool aligned4 = (reinterpret_cast<uintptr_t>(row) & 3u) == 0;
  const PreLane lc(Q);
  for(int g = w.g; g < w.gEnd; g++)
  {
    const int entry = 4 * g + (lane >> 4);
    F3 v[kPts];
    load_cell<SRC>(c.base, c.cell0, L.cellList, entry, w.count, lane, P.nPoints, v, D);
    unsigned int word = 0u;
#pragma unroll
    for(int j = 0; j < kPts; j++)
      word |= label_of<CHECKS>(v[j], Q, lc, L) << (8 * j);
    if(entry < w.count)
      store_labels4(row, aligned4, (c.cell0 + static_cast<int>(L.cellList[entry])) * kCell + kPts * (lane & 15), P.nPoints, word);
  }
}

} // namespace ssd

#endif /* SSD_K_LABELS_H_ */
