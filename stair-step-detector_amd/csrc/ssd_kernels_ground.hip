/*
 * ssd_kernels_ground.hip - k_ground_moments, the ground fit's one kernel (ssd_enqueue_ground_fit), and its
 * launcher.  A translation unit of its own that includes none of the detection kernels, so that their code is not touched by it.
 *
 * A pure stream: every point of a frame is read once (12 bytes as a vertex, 2 as 16-bit depth) and 80 bytes per frame come out.
 * The grid's second dimension is the frame, so the frame's prior is block-uniform: its address depends on blockIdx.y alone and the
 * loads are scalar loads into SGPRs.  Several blocks share a frame and walk it in strides of the whole row of blocks.  Each lane
 * keeps the ten integer sums of ssd_ground_moments; they are reduced across the wave (shuffles), across the block's waves (LDS),
 * and one set of ten 64-bit atomicAdds per block goes to the frame's record, which the caller zeroed on the stream.  Integer
 * addition: the result does not depend on any order.  Overflow: see ground_point (ssd_ground.h).
 */
#include "ssd_ground.h"
#include "ssd_launch.h"                     /* aligned_to */

namespace ssd
{

constexpr int kGroundThreads = 256;
constexpr int kGroundWaves = kGroundThreads / 64;
enum { kGroundVertices = 0, kGroundDepth16 = 1 };

/* the block's ten sums into the frame's record */
__device__ __forceinline__ void ground_reduce(long long (&acc)[kGroundSums], long long *__restrict__ record)
{
  __shared__ long long part[kGroundWaves][kGroundSums];
#pragma unroll
  for(int i = 0; i < kGroundSums; i++)
  {
#pragma unroll
    for(int o = 32; o >= 1; o >>= 1)
      acc[i] += __shfl_xor(acc[i], o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if(lane == 0)
  {
#pragma unroll
    for(int i = 0; i < kGroundSums; i++)
      part[wave][i] = acc[i];
  }
  __syncthreads();
  if(threadIdx.x < kGroundSums)
  {
    long long t = 0;
#pragma unroll
    for(int w = 0; w < kGroundWaves; w++)
      t += part[w][threadIdx.x];
    if(t != 0)
      atomicAdd(reinterpret_cast<unsigned long long *>(record) + threadIdx.x, static_cast<unsigned long long>(t));
  }
}

/* SRC = kGroundVertices: xyz floats.  WIDE: the frames' addresses are multiples of 16 bytes - four points as three 16-byte loads;
 * the nPoints % 4 points behind them, and everything when !WIDE, one point per lane and step. */
template<int SRC, bool WIDE>
__global__ __launch_bounds__(kGroundThreads) void k_ground_moments(const unsigned char *__restrict__ frames, size_t strideBytes, int W, int nPoints,
                                                                 const GroundPrior *__restrict__ priors, int priorStep, GroundRange R,
                                                                 long long *__restrict__ records)
{
  const int frame = blockIdx.y;
  const GroundPrior C = priors[static_cast<size_t>(frame) * priorStep];      /* a copy: fetched once, at block start, into SGPRs */
  const unsigned char *base = frames + static_cast<size_t>(frame) * strideBytes;
  const int first = blockIdx.x * kGroundThreads + threadIdx.x, step = gridDim.x * kGroundThreads;
  long long acc[kGroundSums] = {};
  if constexpr(SRC == kGroundVertices)
  {
    const float *xyz = reinterpret_cast<const float *>(base);
    int done = 0;
    if constexpr(WIDE)
    {
      const float4 *v = reinterpret_cast<const float4 *>(base);
      const int nUnits = nPoints / 4;
      for(int g = first; g < nUnits; g += step)
      {
        const float4 p0 = v[3 * static_cast<size_t>(g)], p1 = v[3 * static_cast<size_t>(g) + 1], p2 = v[3 * static_cast<size_t>(g) + 2];
        ground_point(C, R, p0.x, p0.y, p0.z, acc);
        ground_point(C, R, p0.w, p1.x, p1.y, acc);
        ground_point(C, R, p1.z, p1.w, p2.x, acc);
        ground_point(C, R, p2.y, p2.z, p2.w, acc);
      }
      done = nUnits * 4;
    }
    for(int i = done + first; i < nPoints; i += step)
      ground_point(C, R, xyz[3 * static_cast<size_t>(i)], xyz[3 * static_cast<size_t>(i) + 1], xyz[3 * static_cast<size_t>(i) + 2], acc);
  }
  else
  {
    /* rs2::pointcloud's maps of this frame's camera, xmap[W] then ymap[H], made by the block with the host's float expressions
     * (ssd_deproject_host: the division is IEEE, correctly rounded, on both sides) */
    extern __shared__ __attribute__((aligned(16))) float maps[];
    const int H = nPoints / W;
    for(int i = threadIdx.x; i < W + H; i += kGroundThreads)
      maps[i] = i < W ? ground_map_x(C, i) : ground_map_y(C, i - W);
    __syncthreads();
    const unsigned short *dep = reinterpret_cast<const unsigned short *>(base);
    const float units = C.depthUnits;
    auto one = [&](unsigned int raw, int u, int v)
    {
      const float d = static_cast<float>(raw) * units;          /* raw = 0 gives z = 0: no point */
      ground_point(C, R, d * maps[u], d * maps[W + v], d, acc);
    };
    int done = 0;
    if constexpr(WIDE)
    {
      const uint4 *q = reinterpret_cast<const uint4 *>(base);
      const int nUnits = nPoints / 8;
      for(int g = first; g < nUnits; g += step)
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
      done = nUnits * 8;
    }
    for(int i = done + first; i < nPoints; i += step)
      one(dep[i], i % W, i / W);
  }
  ground_reduce(acc, records + static_cast<size_t>(frame) * kGroundSums);
}

void launch_ground_moments(const void *frames, size_t strideBytes, int W, int H, int nframes, bool depthInput, const GroundPrior *priors,
                           int priorStep, const GroundRange &R, long long *records, hipStream_t s)
{
  const int nPoints = W * H;
  const int perLane = depthInput ? 8 : 4;
  const bool wide = aligned_to(frames, strideBytes, 16);
  /* blocks per frame: enough blocks in all to fill the chip (256 CUs x 8 blocks) when the frames are few, at most 32 steps of the
   * wide loop per lane when they are large, never more blocks than there is work for */
  const int work = (nPoints + perLane * kGroundThreads - 1) / (perLane * kGroundThreads);
  int blocks = (4096 + nframes - 1) / nframes;
  if(blocks < (work + 31) / 32) blocks = (work + 31) / 32;
  if(blocks > work) blocks = work;
  if(blocks < 1) blocks = 1;
  const dim3 grid(blocks, nframes), block(kGroundThreads);
  const unsigned char *f = static_cast<const unsigned char *>(frames);
  if(depthInput)
  {
    const size_t lds = (static_cast<size_t>(W) + H) * sizeof(float);
    if(wide)
      hipLaunchKernelGGL((k_ground_moments<kGroundDepth16, true>), grid, block, lds, s, f, strideBytes, W, nPoints, priors, priorStep, R, records);
    else
      hipLaunchKernelGGL((k_ground_moments<kGroundDepth16, false>), grid, block, lds, s, f, strideBytes, W, nPoints, priors, priorStep, R, records);
  }
  else
  {
    if(wide)
      hipLaunchKernelGGL((k_ground_moments<kGroundVertices, true>), grid, block, 0, s, f, strideBytes, W, nPoints, priors, priorStep, R, records);
    else
      hipLaunchKernelGGL((k_ground_moments<kGroundVertices, false>), grid, block, 0, s, f, strideBytes, W, nPoints, priors, priorStep, R, records);
  }
}

} // namespace ssd

/* k_stair_pose stands on this kernel's skeleton and shares its translation unit */
#include "ssd_kernels_pose.hip"

/* k_depth_fuse, the third stand-alone frame pass: its body in a header, its launcher here */
#include "ssd_k_fuse.h"

namespace ssd
{

template<int NP>
static void launch_depth_fuse_sized(const FuseArgs &A, bool wide, hipStream_t s)
{
  const dim3 grid(static_cast<unsigned int>(A.blocksPerGroup) * A.ngroups), block(kFuseThreads);
  if(wide)
    hipLaunchKernelGGL((k_depth_fuse<NP, true>), grid, block, kFuseLds, s, A);
  else
    hipLaunchKernelGGL((k_depth_fuse<NP, false>), grid, block, kFuseLds, s, A);
}

void launch_depth_fuse(const void *frames, size_t strideBytes, int nPoints, int n, int hop, int ngroups, const ssd_depth_fuse_rule &rule,
                       void *out, size_t outStride, uint8_t *support, size_t supStride, ssd_depth_fuse_stats *stats, bool groupFastest,
                       hipStream_t s)
{
  /* the wide body: 128-bit loads and stores of eight pixels, 64-bit stores of their support */
  const bool wide = aligned_to(frames, strideBytes, 16) && aligned_to(out, outStride, 16) && (!support || aligned_to(support, supStride, 8));
  /* blocks per group: one step of the loop per lane (a step holds n loads in flight) until the grid passes 32768 blocks */
  const int work = (nPoints + kFusePerLane * kFuseThreads - 1) / (kFusePerLane * kFuseThreads);
  const long long all = static_cast<long long>(work) * ngroups;
  const int steps = static_cast<int>((all + 32767) / 32768);
  int blocks = (work + steps - 1) / steps;
  if(blocks < 1) blocks = 1;
  FuseArgs A;
  A.frames = static_cast<const unsigned char *>(frames);
  A.strideBytes = strideBytes;
  A.out = static_cast<unsigned char *>(out);
  A.outStride = outStride;
  A.support = support;
  A.supStride = supStride;
  A.stats = reinterpret_cast<unsigned long long *>(stats);
  A.nPoints = nPoints; A.n = n; A.hop = hop; A.ngroups = ngroups; A.blocksPerGroup = blocks; A.groupFastest = groupFastest ? 1 : 0;
  A.rule = rule;
  if(n > 8) launch_depth_fuse_sized<16>(A, wide, s);
  else if(n > 4) launch_depth_fuse_sized<8>(A, wide, s);
  else if(n > 2) launch_depth_fuse_sized<4>(A, wide, s);
  else if(n > 1) launch_depth_fuse_sized<2>(A, wide, s);
  else launch_depth_fuse_sized<1>(A, wide, s);
}

} // namespace ssd

/* k_depth_edges, the fourth stand-alone frame pass and the first stencil: its body in a header, its launcher here */
#include "ssd_k_edges.h"

namespace ssd
{

void launch_depth_edges(const void *frames, size_t strideBytes, int W, int H, int nframes, const ssd_depth_edge_rule &rule, void *out,
                        size_t outStride, uint8_t *cls, size_t clsStride, ssd_depth_edge_stats *stats, hipStream_t s)
{
  /* the wide body: 128-bit loads and stores of a strip, 64-bit stores of its classes.  Rows are packed, so a strip lies on a 16-byte
   * boundary only where the width is a multiple of 8 */
  const bool wide = W % kEdgeStrip == 0 && aligned_to(frames, strideBytes, 16) && aligned_to(out, outStride, 16) && (!cls || aligned_to(cls, clsStride, 8));
  EdgeArgs A;
  A.frames = static_cast<const unsigned char *>(frames);
  A.strideBytes = strideBytes;
  A.out = static_cast<unsigned char *>(out);
  A.outStride = outStride;
  A.cls = cls;
  A.clsStride = clsStride;
  A.stats = reinterpret_cast<unsigned long long *>(stats);
  A.W = W; A.H = H; A.nframes = nframes;
  A.spans = (W + kEdgeSpan - 1) / kEdgeSpan;
  A.tasks = A.spans * ((H + kEdgeTile - 1) / kEdgeTile);
  A.blocksPerFrame = (A.tasks + kEdgeWaves - 1) / kEdgeWaves;
  A.rule = rule;
  const dim3 grid(static_cast<unsigned int>(A.blocksPerFrame) * nframes), block(kEdgeThreads);
  if(wide)
    hipLaunchKernelGGL((k_depth_edges<true>), grid, block, kEdgeLds, s, A);
  else
    hipLaunchKernelGGL((k_depth_edges<false>), grid, block, kEdgeLds, s, A);
}

} // namespace ssd

/* k_depth_warp, the fifth stand-alone frame pass and the first scatter: its body in a header, its launcher here */
#include "ssd_k_warp.h"

namespace ssd
{

void launch_depth_warp(const void *frames, size_t strideBytes, int W, int H, int nframes, const ssd_depth_warp_view *views,
                       const ssd_intrinsics &dst, void *out, size_t outStride, ssd_depth_warp_stats *stats, hipStream_t s)
{
  const int nPoints = W * H;
  /* the wide body: 128-bit loads of eight pixels.  The scatter goes word by word whatever the output's alignment */
  const bool wide = aligned_to(frames, strideBytes, 16);
  /* blocks per frame: a block makes the maps (W + H divisions) before its first step, so it takes up to eight steps of the loop per lane
   * where that still leaves 2048 blocks in all (256 CUs x 8), never fewer than one step */
  const int work = (nPoints + kWarpPerLane * kWarpThreads - 1) / (kWarpPerLane * kWarpThreads);
  int steps = static_cast<int>(static_cast<long long>(work) * nframes / 2048);
  if(steps > 8) steps = 8;
  if(steps < 1) steps = 1;
  int blocks = (work + steps - 1) / steps;
  if(blocks < 1) blocks = 1;
  WarpArgs A;
  A.frames = static_cast<const unsigned char *>(frames);
  A.strideBytes = strideBytes;
  A.out = static_cast<unsigned char *>(out);
  A.outStride = outStride;
  A.views = views;
  A.stats = reinterpret_cast<unsigned long long *>(stats);
  A.W = W; A.H = H; A.nframes = nframes; A.blocksPerFrame = blocks;
  A.dst = dst;
  const dim3 grid(static_cast<unsigned int>(blocks) * nframes), block(kWarpThreads);
  const size_t lds = warp_lds_bytes(W, H);
  if(wide)
    hipLaunchKernelGGL((k_depth_warp<true>), grid, block, lds, s, A);
  else
    hipLaunchKernelGGL((k_depth_warp<false>), grid, block, lds, s, A);
}

} // namespace ssd

/* k_depth_fill, the sixth stand-alone frame pass and the second stencil, on the edge filter's row machinery: its
 * body in a header, its launcher here */
#include "ssd_k_fill.h"

namespace ssd
{

void launch_depth_fill(const void *frames, size_t strideBytes, int W, int H, int nframes, const ssd_depth_fill_rule &rule, void *out,
                       size_t outStride, uint8_t *cls, size_t clsStride, ssd_depth_fill_stats *stats, hipStream_t s)
{
  /* the wide body: k_depth_edges' condition, for its loads and stores */
  const bool wide = W % kEdgeStrip == 0 && aligned_to(frames, strideBytes, 16) && aligned_to(out, outStride, 16) && (!cls || aligned_to(cls, clsStride, 8));
  FillArgs A;
  A.frames = static_cast<const unsigned char *>(frames);
  A.strideBytes = strideBytes;
  A.out = static_cast<unsigned char *>(out);
  A.outStride = outStride;
  A.cls = cls;
  A.clsStride = clsStride;
  A.stats = reinterpret_cast<unsigned long long *>(stats);
  A.W = W; A.H = H; A.nframes = nframes;
  A.spans = (W + kEdgeSpan - 1) / kEdgeSpan;
  A.tasks = A.spans * ((H + kEdgeTile - 1) / kEdgeTile);
  A.blocksPerFrame = (A.tasks + kEdgeWaves - 1) / kEdgeWaves;
  A.rule = rule;
  const dim3 grid(static_cast<unsigned int>(A.blocksPerFrame) * nframes), block(kEdgeThreads);
  if(wide)
    hipLaunchKernelGGL((k_depth_fill<true>), grid, block, kFillLds, s, A);
  else
    hipLaunchKernelGGL((k_depth_fill<false>), grid, block, kFillLds, s, A);
}

} // namespace ssd
