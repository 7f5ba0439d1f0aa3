/*
 * ssd_k_warp.h - k_depth_warp, the depth warp's one kernel (ssd_enqueue_depth_warp).  ssd_kernels_ground.hip, the
 * unit of the stand-alone frame passes, includes it and holds its launcher.
 *
 * A stream over the SOURCE and a scatter into the target: every sample of a frame is read once (2 bytes), goes through warp_sample
 * (ssd_warp.h: a float point, three rows of doubles, three double divisions where it lands) and the landed ones go to their target pixel
 * as a minimum.  A lane takes eight neighbouring pixels - one 128-bit load in the wide body, eight 2-byte loads in the narrow one, a
 * block's units interleaved there so that a wave's loads are neighbours (k_depth_fuse's two bodies and its tail handling).  The frame's
 * view is read once per block, from an address that depends on blockIdx alone; the source's maps, xmap[W] then ymap[H], are made by the
 * block in LDS with the host's float expressions (k_ground_moments' scheme).
 *
 * The scatter: gfx950 has no 16-bit global atomic, so the minimum is a compare-and-swap loop on the aligned 32-bit word that holds the
 * pixel; the other half of the word goes back as it was seen.  The enqueue zeroed the frame, 0 is "nothing landed", and a half only
 * ever goes from 0 to a value and from a value to a smaller one.  So a load in front of the loop may skip the swap where the half is
 * already non-zero and <= q - a stale value is one the half held earlier, which is no smaller than what it holds now -, and the lane
 * whose swap takes a half from 0 to non-zero counts the pixel as filled: exactly one per filled pixel, whatever the order.  The swap
 * returns the word, so every turn of the loop waits for memory; lanes of one wave that meet in a word take turns.
 *
 * The record: six sums per lane, reduced across the wave (shuffles), across the block's waves (dynamic LDS, 256 bytes behind the maps)
 * and one 64-bit add per block and non-zero word - k_depth_fuse's scheme.
 */
#ifndef SSD_K_WARP_H_
#define SSD_K_WARP_H_

#include "ssd_warp.h"

namespace ssd
{

constexpr int kWarpThreads = 256;
constexpr int kWarpWaves = kWarpThreads / 64;
constexpr int kWarpPerLane = 8;                                      /* pixels of a lane per step: a unit */
constexpr int kWarpPartBytes = kWarpWaves * kWarpWords * 8;          /* 256 bytes */

/* the dynamic LDS of a block: the waves' partial sums first (a multiple of 16 bytes), the maps behind them */
inline size_t warp_lds_bytes(int W, int H) { return kWarpPartBytes + (static_cast<size_t>(W) + H) * sizeof(float); }

struct WarpArgs
{
  const unsigned char *frames;
  size_t strideBytes;
  unsigned char *out;
  size_t outStride;
  const ssd_depth_warp_view *views;          /* one per frame */
  unsigned long long *stats;                 /* kWarpWords per frame */
  int W, H, nframes, blocksPerFrame;
  ssd_intrinsics dst;
};

/* q onto the 16-bit pixel `pixel` of the frame at `frame` as a minimum; true: this call took the pixel from 0 to non-zero */
__device__ __forceinline__ bool warp_land(unsigned char *frame, int pixel, unsigned int q)
{
  unsigned int *word = reinterpret_cast<unsigned int *>(frame) + (pixel >> 1);
  const unsigned int shift = (pixel & 1) ? 16u : 0u;
  unsigned int old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for(;;)
  {
    const unsigned int cur = (old >> shift) & 0xffffu;
    if(cur != 0u && cur <= q)
      return false;                                                    /* values only fall: nothing to do */
    const unsigned int want = (old & ~(0xffffu << shift)) | (warp_min(cur, q) << shift);
    const unsigned int seen = atomicCAS(word, old, want);
    if(seen == old)
      return cur == 0u;
    old = seen;
  }
}

/* WIDE: the frames lie on 16-byte boundaries - a lane's unit is eight neighbouring pixels and one 128-bit load; the pixels behind the
 * last whole unit, and everything when !WIDE, go element by element, where !WIDE a block's units interleaved */
template<bool WIDE>
__global__ __launch_bounds__(kWarpThreads) void k_depth_warp(const WarpArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char warpLds[];
  unsigned long long *part = reinterpret_cast<unsigned long long *>(warpLds);
  float *maps = reinterpret_cast<float *>(warpLds + kWarpPartBytes);
  const int bid = static_cast<int>(blockIdx.x);
  const int frame = bid / A.blocksPerFrame, chunk = bid % A.blocksPerFrame;
  const int t = static_cast<int>(threadIdx.x);
  const int W = A.W, H = A.H, nPoints = W * H;
  const ssd_depth_warp_view V = A.views[frame];                       /* a copy: fetched once, at block start */
  const WarpTarget T = warp_target(A.dst);
  for(int i = t; i < W + H; i += kWarpThreads)
    maps[i] = i < W ? warp_map_x(V.src, i) : warp_map_y(V.src, i - W);
  __syncthreads();
  const unsigned char *base = A.frames + static_cast<size_t>(frame) * A.strideBytes;
  const unsigned short *dep = reinterpret_cast<const unsigned short *>(base);
  unsigned char *outFrame = A.out + static_cast<size_t>(frame) * A.outStride;
  const int wholeUnits = nPoints / kWarpPerLane, units = (nPoints + kWarpPerLane - 1) / kWarpPerLane;
  unsigned int sums[kWarpSums] = {};
  for(int ub = chunk * kWarpThreads; ub < units; ub += A.blocksPerFrame * kWarpThreads)
  {
    const int u = ub + t;
    const bool whole = WIDE && u < wholeUnits;
    unsigned int v[kWarpPerLane];
    int pix[kWarpPerLane];
#pragma unroll
    for(int e = 0; e < kWarpPerLane; e++)
      pix[e] = WIDE ? u * kWarpPerLane + e : ub * kWarpPerLane + e * kWarpThreads + t;
    if(whole)
    {
      const uint4 r = *reinterpret_cast<const uint4 *>(base + static_cast<size_t>(u) * 16);
      v[0] = r.x & 0xffffu; v[1] = r.x >> 16; v[2] = r.y & 0xffffu; v[3] = r.y >> 16;
      v[4] = r.z & 0xffffu; v[5] = r.z >> 16; v[6] = r.w & 0xffffu; v[7] = r.w >> 16;
    }
    else
    {
#pragma unroll
      for(int e = 0; e < kWarpPerLane; e++)
      {
        const int p = pix[e] < nPoints ? pix[e] : nPoints - 1;         /* the load stays inside the frame */
        v[e] = dep[p];
      }
    }
    int row = 0, col = 0;
#pragma unroll
    for(int e = 0; e < kWarpPerLane; e++)
    {
      const bool live = pix[e] < nPoints;
      const int p = live ? pix[e] : nPoints - 1;                       /* ... and so do the maps' reads */
      if(!WIDE || e == 0 || !live)
      {
        row = p / W;
        col = p - row * W;
      }
      else if(++col == W)                                              /* WIDE: the pixel behind the one before */
      {
        col = 0;
        row++;
      }
      int a, b;
      unsigned int q;
      const int cls = warp_sample(V, T, W, H, v[e], maps[col], maps[W + row], a, b, q);
      if(live)
      {
#pragma unroll
        for(int k = 0; k < kWarpNFilled; k++)
          sums[k] += cls == k ? 1u : 0u;
        if(cls == kWarpNLanded && warp_land(outFrame, b * W + a, q))
          sums[kWarpNFilled]++;
      }
    }
  }
  /* the block's sums into the frame's record */
  unsigned long long acc[kWarpSums];
#pragma unroll
  for(int i = 0; i < kWarpSums; i++)
  {
    acc[i] = sums[i];
#pragma unroll
    for(int o = 32; o >= 1; o >>= 1)
      acc[i] += __shfl_xor(acc[i], o);
  }
  if((t & 63) == 0)
  {
#pragma unroll
    for(int i = 0; i < kWarpSums; i++)
      part[(t >> 6) * kWarpWords + i] = acc[i];
  }
  __syncthreads();
  if(t < kWarpSums)
  {
    unsigned long long sum = 0ull;
#pragma unroll
    for(int w = 0; w < kWarpWaves; w++)
      sum += part[w * kWarpWords + t];
    if(sum != 0ull)
      atomicAdd(A.stats + static_cast<size_t>(frame) * kWarpWords + t, sum);
  }
}

} // namespace ssd

#endif /* SSD_K_WARP_H_ */
