/*
 * ssd_kernels_refit.hip - the trimmed surface refit's kernels (ssd_enqueue_surface_refit, DESIGN.md section 7g;
 * ssd_enqueue_cameras_surface_refit, section 7h) and their launchers.
 *
 * k_surface_refit is a sibling body of k_surface_moments: the same cells from K1's records, the same decision
 * (quad_decide<.., true>), the same load, the same accumulation - and a gate test between the label and the sums;
 * k_surface_refit_cams runs the same body with the frame's camera record in place of the handle's by-value constants.  The file
 * includes ssd_kernels.hip with SSD_CAMERAS_TU defined, as ssd_kernels_cams.hip does, which gives that file's device code without its
 * entry points and launchers: a translation unit of its own, so that no kernel of the chain is touched by what is instantiated here.
 */
#define SSD_CAMERAS_TU
#include "ssd_kernels.hip"
#include "ssd_refit.h"

namespace ssd
{

static_assert(sizeof(ssd_plane_gate) == 40 && sizeof(ssd_frame_gates) == 8 + SSD_MAX_STEPS * sizeof(ssd_plane_gate) && sizeof(ssd_frame_gates) % 8 == 0,
              "ssd_frame_gates is staged as 64-bit words: a header of two int32, then five doubles per surface");
constexpr int kGateWords = static_cast<int>(sizeof(ssd_frame_gates) / 8);
static_assert(kGateWords <= kThreads, "one thread per word of the frame's gates");

struct RefitLds
{
  SurfaceLds s;                                  /* k_surface_moments', unchanged */
  ssd_frame_gates gates;                         /* the frame's, fetched once per block */
};

/* k_surface_moments' body (ssd_kernels.hip; the comments there stand for what is the same) with the frame's gates in LDS and, on the
 * lane's own label, the gate test of ssd_refit.h: a labelled point outside its surface's gate becomes an unlabelled one BEHIND the
 * wave-uniform skip of the slots that label nothing, so the three double products are spent only where some lane has a label.  A
 * point trimmed here is counted nowhere.  The header is written as the first pass writes it, from the same FrameState. */
template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_surface_refit(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q,
                                                            const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                            size_t tileMaskStride, int chunkPoints, DepthSrc D,
                                                            const ssd_frame_gates *__restrict__ gates, ssd_frame_moments *__restrict__ out)
{
  __shared__ RefitLds R;
  SurfaceLds &S = R.s;
  LabelsLds &L = S.l;
  const int tid = threadIdx.x, lane = tid & 63;
  const int frame = blockIdx.x;
  const FrameState &fs = st[frame];
  const bool live = fs.anyActive != 0u && (fs.status & SSD_ST_THROW) == 0u;           /* block-uniform */
  const unsigned int wanted = live ? fs.wantedQuads : 0u;
  if(live)
  {
    const int nLive = fs.nLive;
    const int gSlot = (nLive > 0 && fs.accActive[kGroundAcc]) ? nLive - 1 : -1;       /* the ground is the last live slot */
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
    /* the frame's gates: 86 words, once per block */
    if(tid < kGateWords)
      reinterpret_cast<unsigned long long *>(&R.gates)[tid] = reinterpret_cast<const unsigned long long *>(gates + frame)[tid];
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
      /* the record's header is the first pass's */
      if(blockIdx.y == 0)
      {
        out[frame].n_surfaces = min(nLive, SSD_MAX_STEPS);
        out[frame].ground = gSlot >= 0 ? 1 : 0;
      }
    }
  }
  if(tid < SSD_MAX_STEPS * kSurfaceSums)
    (&S.sums[0][0])[tid] = 0ull;
  __syncthreads();
  if(wanted == 0u)
    return;

  const float *base = SRC == kSrcDepth16
    ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(xyz) + static_cast<size_t>(frame) * strideFloats)
    : xyz + static_cast<size_t>(frame) * strideFloats;
  const int begin = blockIdx.y * chunkPoints;
  const int end = min(begin + chunkPoints, P.nPoints);
  const int cell0 = begin / kCell;
  const int nCells = (end - begin + kCell - 1) / kCell;
  const uint2 *cells = tileMasks + static_cast<size_t>(frame) * tileMaskStride + cell0;

  const int count = cell_list_build(cells, nCells, 1, [&](const uint2 info) { return (info.x & wanted) != 0u; }, L.cellList, L.listScratch);
  const PreLane lc(Q);
  const int nGroups = (count + 3) >> 2;
  const int gEnd = ((tid >> 6) + 1) * nGroups / kWavesPerBlock;
  long long acc[kSurfaceSums] = {};
  int cur = 0;                                   /* the label whose sums the wave's registers hold (0: none yet) */
  for(int g = (tid >> 6) * nGroups / kWavesPerBlock; g < gEnd; g++)
  {
    const int entry = 4 * g + (lane >> 4);
    F3 v[kPts];
    load_cell<SRC>(base, cell0, L.cellList, entry, count, lane, P.nPoints, v, D);
#pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      f32x2 d;
      float M, M3;
      unsigned int q;
      unsigned long long mSlow, mIn, mGround;
      quad_decide<CHECKS, true>(v[j], Q, lc, L.edges, L.lut, L.qts, L.kc, -1, d, M, M3, q, mSlow, mIn, mGround);
      const int labelled = (__builtin_amdgcn_inverse_ballot_w64(mIn) && entry < count) ? L.label[min(q, static_cast<unsigned int>(kMaxLive))] : 0;
      if(__ballot(labelled != 0) == 0ull)        /* wave-uniform: a slot none of whose points is labelled */
        continue;
      /* the gate, on the lane's own label (1 .. SSD_MAX_STEPS: L.label holds nothing else) */
      const int lab = (labelled != 0 && refit_keeps(R.gates, labelled - 1, v[j].x, v[j].y, v[j].z)) ? labelled : 0;
      const unsigned long long mLab = __ballot(lab != 0);
      if(mLab == 0ull)                           /* wave-uniform: every labelled point of the slot was trimmed */
        continue;
      if(cur == 0 || __ballot(lab == cur) == 0ull)
      {
        if(cur != 0)
          surface_flush(acc, S.sums, cur - 1, lane);
        cur = __builtin_amdgcn_readlane(lab, __ffsll(static_cast<long long>(mLab)) - 1);
      }
      /* the fixed-point rule (ssd_moments.h) on the float camera coordinates */
      const double rx = moment_round(static_cast<double>(v[j].x)), ry = moment_round(static_cast<double>(v[j].y)), rz = moment_round(static_cast<double>(v[j].z));
      const bool fits = moment_near(rx) && moment_near(ry) && moment_near(rz);
      if(lab == cur)
      {
        if(fits)
          moment_add(rx, ry, rz, acc);
        else
          acc[kGroundSums] += 1;
      }
      else if(lab != 0)
      {
        unsigned long long *t = S.sums[lab - 1];
        if(fits)
        {
          long long one[kGroundSums] = {};
          moment_add(rx, ry, rz, one);
#pragma unroll
          for(int i = 0; i < kGroundSums; i++)
            atomicAdd(&t[i], static_cast<unsigned long long>(one[i]));
        }
        else
          atomicAdd(&t[kGroundSums], 1ull);
      }
    }
  }
  if(cur != 0)
    surface_flush(acc, S.sums, cur - 1, lane);
  __syncthreads();
  if(tid < SSD_MAX_STEPS * kSurfaceSums)
  {
    const unsigned long long t = (&S.sums[0][0])[tid];
    if(t != 0ull)
      atomicAdd(reinterpret_cast<unsigned long long *>(out + frame) + 1 + tid, t);
  }
}

/* The SAME body once more, as a device function for the cameras entry point below.  A copy, not a move: with the body moved out
 * of k_surface_refit and called from it, the compiler laid that kernel out differently (68 bytes of code and, for CHECKS = false on
 * vertices, two scalar registers: profiles/camera_surfaces_refit_kernel_resources.txt), and the one-calibration
 * pass is the yardstick the cameras pass is measured against - so its entry point stays textually what it was.  Whoever changes one of
 * the two changes the other: tests/test_gpu_camera_surfaces_refit.py holds every cameras record to the one-calibration handle's. */
template<int SRC, bool CHECKS>
__device__ __forceinline__ void surface_refit_block(const float *__restrict__ xyz, size_t strideFloats, const PointParams &P, const PreXY &Q,
                                                    const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                    size_t tileMaskStride, int chunkPoints, const DepthSrc &D,
                                                    const ssd_frame_gates *__restrict__ gates, ssd_frame_moments *__restrict__ out)
{
  __shared__ RefitLds R;
  SurfaceLds &S = R.s;
  LabelsLds &L = S.l;
  const int tid = threadIdx.x, lane = tid & 63;
  const int frame = blockIdx.x;
  const FrameState &fs = st[frame];
  const bool live = fs.anyActive != 0u && (fs.status & SSD_ST_THROW) == 0u;           /* block-uniform */
  const unsigned int wanted = live ? fs.wantedQuads : 0u;
  if(live)
  {
    const int nLive = fs.nLive;
    const int gSlot = (nLive > 0 && fs.accActive[kGroundAcc]) ? nLive - 1 : -1;       /* the ground is the last live slot */
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
    /* the frame's gates: 86 words, once per block */
    if(tid < kGateWords)
      reinterpret_cast<unsigned long long *>(&R.gates)[tid] = reinterpret_cast<const unsigned long long *>(gates + frame)[tid];
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
      /* the record's header is the first pass's */
      if(blockIdx.y == 0)
      {
        out[frame].n_surfaces = min(nLive, SSD_MAX_STEPS);
        out[frame].ground = gSlot >= 0 ? 1 : 0;
      }
    }
  }
  if(tid < SSD_MAX_STEPS * kSurfaceSums)
    (&S.sums[0][0])[tid] = 0ull;
  __syncthreads();
  if(wanted == 0u)
    return;

  const float *base = SRC == kSrcDepth16
    ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(xyz) + static_cast<size_t>(frame) * strideFloats)
    : xyz + static_cast<size_t>(frame) * strideFloats;
  const int begin = blockIdx.y * chunkPoints;
  const int end = min(begin + chunkPoints, P.nPoints);
  const int cell0 = begin / kCell;
  const int nCells = (end - begin + kCell - 1) / kCell;
  const uint2 *cells = tileMasks + static_cast<size_t>(frame) * tileMaskStride + cell0;

  const int count = cell_list_build(cells, nCells, 1, [&](const uint2 info) { return (info.x & wanted) != 0u; }, L.cellList, L.listScratch);
  const PreLane lc(Q);
  const int nGroups = (count + 3) >> 2;
  const int gEnd = ((tid >> 6) + 1) * nGroups / kWavesPerBlock;
  long long acc[kSurfaceSums] = {};
  int cur = 0;                                   /* the label whose sums the wave's registers hold (0: none yet) */
  for(int g = (tid >> 6) * nGroups / kWavesPerBlock; g < gEnd; g++)
  {
    const int entry = 4 * g + (lane >> 4);
    F3 v[kPts];
    load_cell<SRC>(base, cell0, L.cellList, entry, count, lane, P.nPoints, v, D);
#pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      f32x2 d;
      float M, M3;
      unsigned int q;
      unsigned long long mSlow, mIn, mGround;
      quad_decide<CHECKS, true>(v[j], Q, lc, L.edges, L.lut, L.qts, L.kc, -1, d, M, M3, q, mSlow, mIn, mGround);
      const int labelled = (__builtin_amdgcn_inverse_ballot_w64(mIn) && entry < count) ? L.label[min(q, static_cast<unsigned int>(kMaxLive))] : 0;
      if(__ballot(labelled != 0) == 0ull)        /* wave-uniform: a slot none of whose points is labelled */
        continue;
      /* the gate, on the lane's own label (1 .. SSD_MAX_STEPS: L.label holds nothing else) */
      const int lab = (labelled != 0 && refit_keeps(R.gates, labelled - 1, v[j].x, v[j].y, v[j].z)) ? labelled : 0;
      const unsigned long long mLab = __ballot(lab != 0);
      if(mLab == 0ull)                           /* wave-uniform: every labelled point of the slot was trimmed */
        continue;
      if(cur == 0 || __ballot(lab == cur) == 0ull)
      {
        if(cur != 0)
          surface_flush(acc, S.sums, cur - 1, lane);
        cur = __builtin_amdgcn_readlane(lab, __ffsll(static_cast<long long>(mLab)) - 1);
      }
      /* the fixed-point rule (ssd_moments.h) on the float camera coordinates */
      const double rx = moment_round(static_cast<double>(v[j].x)), ry = moment_round(static_cast<double>(v[j].y)), rz = moment_round(static_cast<double>(v[j].z));
      const bool fits = moment_near(rx) && moment_near(ry) && moment_near(rz);
      if(lab == cur)
      {
        if(fits)
          moment_add(rx, ry, rz, acc);
        else
          acc[kGroundSums] += 1;
      }
      else if(lab != 0)
      {
        unsigned long long *t = S.sums[lab - 1];
        if(fits)
        {
          long long one[kGroundSums] = {};
          moment_add(rx, ry, rz, one);
#pragma unroll
          for(int i = 0; i < kGroundSums; i++)
            atomicAdd(&t[i], static_cast<unsigned long long>(one[i]));
        }
        else
          atomicAdd(&t[kGroundSums], 1ull);
      }
    }
  }
  if(cur != 0)
    surface_flush(acc, S.sums, cur - 1, lane);
  __syncthreads();
  if(tid < SSD_MAX_STEPS * kSurfaceSums)
  {
    const unsigned long long t = (&S.sums[0][0])[tid];
    if(t != 0ull)
      atomicAdd(reinterpret_cast<unsigned long long *>(out + frame) + 1 + tid, t);
  }
}

/* The cameras batch's entry point, shaped like k_surface_moments_cams: the frame's record by scalar loads at block start, the parts the
 * body uses copied, the same body.  The gates stay the FRAME's (gates + frame): two frames of one camera may carry different ones. */
template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_surface_refit_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                                 const int *__restrict__ camOf, const FrameState *__restrict__ st,
                                                                 const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints,
                                                                 const ssd_frame_gates *__restrict__ gates, ssd_frame_moments *__restrict__ out)
{
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const DepthSrc D = C.D;
  surface_refit_block<SRC, CHECKS>(xyz, strideFloats, P, Q, st, tileMasks, tileMaskStride, chunkPoints, D, gates, out);
}

/* grid, block size and instantiations are launch_surface_moments' (the launch rules of ssd_kernels.hip); a cameras batch: CHECKS by the
 * table, and B.depthInput only says that the source is 16-bit depth - each frame's DepthSrc is its camera's */
void launch_surface_refit(const Batch &B, int chunkPoints, const ssd_frame_gates *gates, ssd_frame_moments *out)
{
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &D)
  {
    constexpr int SRC = decltype(src)::value;
    constexpr bool CHECKS = decltype(checks)::value;
    if(B.cams)
      hipLaunchKernelGGL((k_surface_refit_cams<SRC, CHECKS>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, gates, out);
    else
      hipLaunchKernelGGL((k_surface_refit<SRC, CHECKS>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.P.pt, B.P.pre, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, D, gates, out);
  });
}

} // namespace ssd
