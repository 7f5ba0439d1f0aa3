/* ssd_k_walk.h - what K6 - K8 and the passes behind a whole enqueue share (the labels, the surface moments, the refit, the three riser
 * passes, clearance, the tread grid and the stair map): a block's chunk of a frame, the walk over the chunk's cells that hold a wanted
 * bin (K1's records), and integer sums keyed by a wave-uniform surface or riser.  DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_WALK_H_
#define SSD_K_WALK_H_
#include "ssd_k_cells.h"
#include "ssd_moments.h"

namespace ssd
{

/* A block's chunk of a frame: the frame's points, and K1's records of the chunk's cells. */
struct Chunk
{
  const float *base;
  const uint2 *cells;
  int cell0, nCells;
};
template<int SRC>
__device__ __forceinline__ Chunk chunk_of(const float *__restrict__ xyz, size_t strideFloats, const uint2 *__restrict__ tileMasks, size_t tileMaskStride,
                                          int chunkPoints, int nPoints)
{
  const int frame = blockIdx.x;
  Chunk c;
  c.base = SRC == kSrcDepth16
    ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(xyz) + static_cast<size_t>(frame) * strideFloats)
    : xyz + static_cast<size_t>(frame) * strideFloats;
  const int begin = blockIdx.y * chunkPoints;
  const int end = min(begin + chunkPoints, nPoints);
  c.cell0 = begin / kCell;
  c.nCells = (end - begin + kCell - 1) / kCell;
  c.cells = tileMasks + static_cast<size_t>(frame) * tileMaskStride + c.cell0;
  return c;
}

/* The chunk's cells that hold a bin of `wanted`, listed in order, and the wave's share of the list: groups g .. gEnd - 1 of four cells,
 * entry 4 g + (lane >> 4) of the list for each row of sixteen lanes (load_cell). */
struct CellWalk { int count, g, gEnd; };
__device__ __forceinline__ CellWalk wanted_cells(const Chunk &c, int cols, unsigned int wanted, unsigned short *cellList, unsigned int *listScratch)
{
  CellWalk w;
  w.count = cell_list_build(c.cells, c.nCells, cols, [&](const uint2 info) { return (info.x & wanted) != 0u; }, cellList, listScratch);
  const int nGroups = (w.count + 3) >> 2, wave = threadIdx.x >> 6;
  w.g = wave * nGroups / kWavesPerBlock;
  w.gEnd = (wave + 1) * nGroups / kWavesPerBlock;
  return w;
}

constexpr int kSurfaceSums = kGroundSums + 1;       /* ssd_surface_moments as 11 int64: the ten sums, n_far */
static_assert(sizeof(ssd_surface_moments) == 8 * kSurfaceSums && sizeof(ssd_frame_moments) == 8 + SSD_MAX_STEPS * 8 * kSurfaceSums,
              "ssd_frame_moments is the kernel's record: a header of two int32, then kSurfaceSums int64 per surface");
static_assert(SSD_MAX_STEPS * kSurfaceSums <= kThreads, "one thread per entry of the block's table");

/* Integer sums keyed by a wave-uniform current key (a surface, a riser), for k_surface_moments, k_surface_refit and k_riser_moments: N
 * sums per key, the first kGroundSums those of ssd_ground_moments, then n_far; what lies behind is the caller's.  A lane's key is
 * 0 .. or -1 for a point that counts nowhere. */
template<int N>
struct KeyedSums
{
  long long acc[N] = {};
  int cur = -1;                                  /* the key whose sums the wave's registers hold (-1: none yet) */

  /* the wave's sums into the block's table: shuffles, then lane 0's 64-bit LDS adds */
  __device__ __forceinline__ void flush(unsigned long long (*table)[N], int lane)
  {
    if(cur < 0)
      return;
#pragma unroll
    for(int i = 0; i < N; i++)
    {
#pragma unroll
      for(int o = 32; o >= 1; o >>= 1)
        acc[i] += __shfl_xor(acc[i], o);
    }
    if(lane == 0)
    {
#pragma unroll
      for(int i = 0; i < N; i++)
        if(acc[i] != 0)
          atomicAdd(&table[cur][i], static_cast<unsigned long long>(acc[i]));
    }
#pragma unroll
    for(int i = 0; i < N; i++)
      acc[i] = 0;
  }

  /* a point slot some of whose lanes hold a key (mKeyed, not 0): when none of them holds the current one, the wave changes over */
  __device__ __forceinline__ void changeover(int key, unsigned long long mKeyed, unsigned long long (*table)[N], int lane)
  {
    if(cur < 0 || __ballot(key == cur) == 0ull)
    {
      flush(table, lane);
      cur = __builtin_amdgcn_readlane(key, __ffsll(static_cast<long long>(mKeyed)) - 1);
    }
  }

  /* the lane's point by the fixed-point rule (ssd_moments.h) on the float camera coordinates: to the wave's sums under the current key,
   * straight to the table under another (a cell two keys share: rare), nowhere for key < 0 */
  __device__ __forceinline__ void add(int key, const F3 &p, unsigned long long (*table)[N])
  {
    const double rx = moment_round(static_cast<double>(p.x)), ry = moment_round(static_cast<double>(p.y)), rz = moment_round(static_cast<double>(p.z));
    const bool fits = moment_near(rx) && moment_near(ry) && moment_near(rz);
    if(key == cur)
    {
      if(fits)
        moment_add(rx, ry, rz, acc);
      else
        acc[kGroundSums] += 1;
    }
    else if(key >= 0)
    {
      unsigned long long *t = table[key];
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
};

/* the block's end, behind a barrier: a thread per entry of the table, give(key, i, sum) for every one that is not 0 */
template<int N, typename Give>
__device__ __forceinline__ void keyed_sums_give(const unsigned long long (*table)[N], int nKeys, Give give)
{
  const int tid = threadIdx.x;
  if(tid < nKeys * N)
  {
    const int key = tid / N, i = tid - key * N;
    const unsigned long long t = table[key][i];
    if(t != 0ull)
      give(key, i, t);
  }
}

} // namespace ssd

#endif /* SSD_K_WALK_H_ */
