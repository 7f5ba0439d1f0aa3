/*
 * ssd_kernels_pose.hip - k_stair_pose, the stair pose's one kernel (ssd_enqueue_stair_pose), and its launcher.
 * Included at the end of ssd_kernels_ground.hip: the same translation unit, the same skeleton - the grid's second dimension is the
 * frame, the frame's target is block-uniform (its index and its prior come by scalar loads, its tables go through LDS once per block),
 * the wide vertex and depth loads, a depth map per block - and none of k_ground_moments' text is touched.
 *
 * 33 classes x 11 sums are too many for a lane, and neighbouring pixels share a class.  So a block takes a CONTIGUOUS run of the frame
 * and its lanes walk it in steps of the whole block: a lane's next point lies about a row below its last, usually on the same tread or
 * riser.  A lane keeps the eleven sums of ONE class, the class of its last classified point; when the class changes it hands them to the
 * block's table in LDS (eleven 64-bit adds, as often as a lane crosses an edge - not per point) and starts again.  At the end of the
 * walk a wave whose lanes all hold the same class reduces by shuffles and one lane adds; the block's table goes out as one 64-bit global
 * add per touched word.  Integer addition: the result does not depend on any order.  Overflow: ssd_moments.h's argument, per frame.
 */
#include "ssd_pose.h"

namespace ssd
{

constexpr int kPoseThreads = 256;
constexpr int kPoseTargetBytes = (static_cast<int>(sizeof(PoseTarget)) + 15) / 16 * 16;
constexpr int kPoseSumBytes = (kPoseWords * 8 + 15) / 16 * 16;
constexpr int kPoseLds = kPoseTargetBytes + kPoseSumBytes;     /* the depth maps lie behind it: a multiple of 16 */

/* a lane's sums into the block's table, and zero again */
__device__ __forceinline__ void pose_flush(long long (&acc)[kPoseSums], int cls, unsigned long long *sums)
{
  if(cls < 0)
    return;
#pragma unroll
  for(int j = 0; j < kPoseSums; j++)
  {
    if(acc[j] != 0)
      atomicAdd(sums + cls * kPoseSums + j, static_cast<unsigned long long>(acc[j]));
    acc[j] = 0;
  }
}

/* SRC, WIDE: k_ground_moments' (ssd_kernels_ground.hip) */
template<int SRC, bool WIDE>
__global__ __launch_bounds__(kPoseThreads) void k_stair_pose(const unsigned char *__restrict__ frames, size_t strideBytes, int W, int nPoints,
                                                           const PoseTarget *__restrict__ targets, int ntargets, const int *__restrict__ targetOf,
                                                           PoseRange R, ssd_stair_pose_moments *__restrict__ records)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char poseLds[];
  const int frame = blockIdx.y;
  const int t = targetOf[frame];                                               /* block-uniform: a scalar load */
  if(t < 0 || t >= ntargets)
    return;                                                                    /* SSD_STAIR_MAP_NONE: the record stays zero */
  const PoseTarget *target = targets + t;
  const int nSteps = target->nSteps;
  if(nSteps <= 0 || nSteps > kPoseTreads)
    return;                                                                    /* a thrown or empty map: all zero */
  const GroundPrior C = target->cam;                                           /* copies: fetched once, at block start, into SGPRs */
  const ClearanceWorld X = target->world;
  unsigned long long *tgt = reinterpret_cast<unsigned long long *>(poseLds);
  unsigned long long *sums = reinterpret_cast<unsigned long long *>(poseLds + kPoseTargetBytes);
  for(int i = threadIdx.x; i < static_cast<int>(sizeof(PoseTarget) / 8); i += kPoseThreads)
    tgt[i] = reinterpret_cast<const unsigned long long *>(target)[i];
  for(int i = threadIdx.x; i < kPoseWords; i += kPoseThreads)
    sums[i] = 0ull;
  const PoseTarget &T = *reinterpret_cast<const PoseTarget *>(poseLds);
  const unsigned char *base = frames + static_cast<size_t>(frame) * strideBytes;
  long long acc[kPoseSums] = {};
  int cur = -1;
  auto take = [&](float x, float y, float z)
  {
    const int c = pose_class(C, X, T, R, x, y, z);
    if(c < 0)
      return;
    if(c != cur)
    {
      pose_flush(acc, cur, sums);
      cur = c;
    }
    pose_add(x, y, z, acc);
  };
  /* the block's contiguous run of `units` units: [lo, hi) */
  auto run = [&](int units, int &lo, int &hi)
  {
    const int per = (units + static_cast<int>(gridDim.x) - 1) / static_cast<int>(gridDim.x);
    lo = static_cast<int>(blockIdx.x) * per;
    hi = lo + per < units ? lo + per : units;
  };
  const int first = blockIdx.x * kPoseThreads + threadIdx.x, step = gridDim.x * kPoseThreads;
  if constexpr(SRC == kGroundVertices)
  {
    __syncthreads();
    const float *xyz = reinterpret_cast<const float *>(base);
    int lo, hi;
    if constexpr(WIDE)
    {
      const float4 *v = reinterpret_cast<const float4 *>(base);
      const int nUnits = nPoints / 4;
      run(nUnits, lo, hi);
      for(int g = lo + static_cast<int>(threadIdx.x); g < hi; g += kPoseThreads)
      {
        const float4 p0 = v[3 * static_cast<size_t>(g)], p1 = v[3 * static_cast<size_t>(g) + 1], p2 = v[3 * static_cast<size_t>(g) + 2];
        take(p0.x, p0.y, p0.z);
        take(p0.w, p1.x, p1.y);
        take(p1.z, p1.w, p2.x);
        take(p2.y, p2.z, p2.w);
      }
      for(int i = nUnits * 4 + first; i < nPoints; i += step)
        take(xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2]);
    }
    else
    {
      run(nPoints, lo, hi);
      for(int i = lo + static_cast<int>(threadIdx.x); i < hi; i += kPoseThreads)
        take(xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2]);
    }
  }
  else
  {
    /* rs2::pointcloud's maps of the target's camera, xmap[W] then ymap[H], as k_ground_moments makes them */
    float *maps = reinterpret_cast<float *>(poseLds + kPoseLds);
    const int H = nPoints / W;
    for(int i = threadIdx.x; i < W + H; i += kPoseThreads)
      maps[i] = i < W ? ground_map_x(C, i) : ground_map_y(C, i - W);
    __syncthreads();
    const unsigned short *dep = reinterpret_cast<const unsigned short *>(base);
    const float units = C.depthUnits;
    auto one = [&](unsigned int raw, int u, int v)
    {
      const float d = static_cast<float>(raw) * units;          /* raw = 0 gives z = 0: no point */
      take(d * maps[u], d * maps[W + v], d);
    };
    int lo, hi;
    if constexpr(WIDE)
    {
      const uint4 *q = reinterpret_cast<const uint4 *>(base);
      const int nUnits = nPoints / 8;
      run(nUnits, lo, hi);
      for(int g = lo + static_cast<int>(threadIdx.x); g < hi; g += kPoseThreads)
      {
        const uint4 r = q[g];
        const unsigned int w4[4] = { r.x, r.y, r.z, r.w };
        int v = (8 * g) / W, u = 8 * g - v * W;
#pragma unroll
        for(int j = 0; j < 8; j++)
        {
          one((w4[j >> 1] >> (16 * (j & 1))) & 0xffffu, u, v);
          if(++u == W)
          {
            u = 0;
            v++;
          }
        }
      }
      for(int i = nUnits * 8 + first; i < nPoints; i += step)
        one(dep[i], i % W, i / W);
    }
    else
    {
      run(nPoints, lo, hi);
      for(int i = lo + static_cast<int>(threadIdx.x); i < hi; i += kPoseThreads)
        one(dep[i], i % W, i / W);
    }
  }
  /* what the lanes still hold: one class in the whole wave - shuffles, and one lane adds; else each lane for itself */
  const unsigned long long holders = __ballot(cur >= 0);
  if(holders != 0ull)
  {
    const int c0 = __shfl(cur, __ffsll(static_cast<long long>(holders)) - 1);
    if(__all(cur < 0 || cur == c0))
    {
#pragma unroll
      for(int j = 0; j < kPoseSums; j++)
      {
#pragma unroll
        for(int o = 32; o >= 1; o >>= 1)
          acc[j] += __shfl_xor(acc[j], o);
      }
      if((threadIdx.x & 63) == 0)
        pose_flush(acc, c0, sums);
    }
    else
      pose_flush(acc, cur, sums);
  }
  __syncthreads();
  unsigned long long *rec = reinterpret_cast<unsigned long long *>(records + frame);
  for(int i = threadIdx.x; i < kPoseWords; i += kPoseThreads)
  {
    const unsigned long long s = sums[i];
    if(s != 0ull)
      atomicAdd(rec + pose_word(i / kPoseSums) + i % kPoseSums, s);
  }
  if(blockIdx.x == 0 && threadIdx.x == 0)
  {
    int32_t head[4];
    pose_headers(nSteps, T.ground, head);
    int32_t *a = reinterpret_cast<int32_t *>(&records[frame].treads), *b = reinterpret_cast<int32_t *>(&records[frame].risers);
    a[0] = head[0]; a[1] = head[1];
    b[0] = head[2]; b[1] = head[3];
  }
}

void launch_stair_pose(const void *frames, size_t strideBytes, int W, int H, int nframes, bool depthInput, const PoseTarget *targets, int ntargets,
                       const int *targetOf, const PoseRange &R, ssd_stair_pose_moments *records, hipStream_t s)
{
  const int nPoints = W * H;
  const int perLane = depthInput ? 8 : 4;
  const bool wide = aligned_to(frames, strideBytes, 16);
  /* blocks per frame: launch_ground_moments' rule - enough blocks in all to fill the chip when the frames are few, at most 32 steps of
   * the wide loop per lane when they are large, never more blocks than there is work for */
  const int work = (nPoints + perLane * kPoseThreads - 1) / (perLane * kPoseThreads);
  int blocks = (4096 + nframes - 1) / nframes;
  if(blocks < (work + 31) / 32) blocks = (work + 31) / 32;
  if(blocks > work) blocks = work;
  if(blocks < 1) blocks = 1;
  const dim3 grid(blocks, nframes), block(kPoseThreads);
  const unsigned char *f = static_cast<const unsigned char *>(frames);
  if(depthInput)
  {
    const size_t lds = kPoseLds + (static_cast<size_t>(W) + H) * sizeof(float);
    if(wide)
      hipLaunchKernelGGL((k_stair_pose<kGroundDepth16, true>), grid, block, lds, s, f, strideBytes, W, nPoints, targets, ntargets, targetOf, R, records);
    else
      hipLaunchKernelGGL((k_stair_pose<kGroundDepth16, false>), grid, block, lds, s, f, strideBytes, W, nPoints, targets, ntargets, targetOf, R, records);
  }
  else
  {
    if(wide)
      hipLaunchKernelGGL((k_stair_pose<kGroundVertices, true>), grid, block, kPoseLds, s, f, strideBytes, W, nPoints, targets, ntargets, targetOf, R, records);
    else
      hipLaunchKernelGGL((k_stair_pose<kGroundVertices, false>), grid, block, kPoseLds, s, f, strideBytes, W, nPoints, targets, ntargets, targetOf, R, records);
  }
}

} // namespace ssd
