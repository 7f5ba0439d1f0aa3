/* ssd_k_cells.h - K1's cell records as the later passes read them: row reductions, the cell box, cell_list_build, load_cell.
 * Device code of the per-frame path, cut by stage: DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_CELLS_H_
#define SSD_K_CELLS_H_
#include "ssd_k_point.h"

namespace ssd
{

/* K2 and K4 run after frame-wide decisions (plateau table, outlines) and need only the points of a few
 * height bins.  Camera rows sweep one plateau at a time, so whole runs of consecutive points are irrelevant
 * to them.  K1 therefore leaves one 32-bit mask per CELL — 64 consecutive points = the 4 points of each of
 * the 16 lanes of one DPP row — saying which groups of 4 height bins occur in it (4 B per 768 B of input:
 * no measurable traffic, unlike a byte per point which costs K1 a third of its bandwidth,
 * tools/storebench.hip).  The later passes gather the cells that hold a bin they care about into a compact
 * list per block and walk only those (cell_list_build / SSD_CELL_LOOP below): nothing else is loaded, and
 * every wave iteration works on four wanted cells instead of on 256 consecutive points of which half are
 * somebody else's (wave-tile gating: 52 % of the tiles at 52 % lane use in K2; cells: 34 % at 79 %; tools/cell_analysis.py). */
constexpr int kBinsPerGroup = 4;      /* 128 bins -> 32 groups: one 32-bit mask per cell */
constexpr int kWavesPerBlock = kThreads / 64;
constexpr int kCell = 64;                         /* points per cell */
constexpr int kCellsPerTile = kTile / kCell;      /* 16 */
/* a block's chunk is at most this many tiles (choose_chunk; ssd_launch.h holds the same numbers for the host): K1 keeps the
 * chunk's cell masks in LDS, K2 / K4 / K6 the list of its wanted cells.  K2 gets tall chunks: its waves walk down cell
 * columns and pay a window flush at every column change (measured, XGA batch: 2.5 ms with 8-row chunks, 1.5 with 16,
 * 1.0 with 32) */
#ifndef SSD_MAX_TILES
#define SSD_MAX_TILES 32
#endif
constexpr int kMaxTilesPerBlock = SSD_MAX_TILES;
constexpr int kMaxCellsPerBlock = kMaxTilesPerBlock * kCellsPerTile;
constexpr int kMaxTilesPerBlockRaster = 128;
constexpr int kMaxCellsPerBlockRaster = kMaxTilesPerBlockRaster * kCellsPerTile;
constexpr int kMaxTilesPerBlockInquad = 128;
constexpr int kMaxCellsPerBlockInquad = kMaxTilesPerBlockInquad * kCellsPerTile;

/* OR over the 16 lanes of a DPP row (row_ror 8, 4, 2, 1): every lane of the row gets the row's result */
__device__ __forceinline__ unsigned int row_or_u32(unsigned int v)
{
  v |= static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x128, 0xf, 0xf, false));
  v |= static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x124, 0xf, 0xf, false));
  v |= static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x122, 0xf, 0xf, false));
  v |= static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x121, 0xf, 0xf, false));
  return v;
}

/* K1 also leaves, per cell, the bounding box of its in-range points in world x / y on a 256 x 256 grid over the measuring
 * range (one byte per bound: x0, x1, y0, y1; a cell with no in-range point has an empty mask and a meaningless box).
 * k_inquad decides from it, without loading the cell, that all its points lie outside the ground quadrilateral, or all
 * inside a tread's (its thresholds on this grid carry a margin far above any rounding: InquadLds::liveBox).
 *
 * Round 4: the extremes are tracked per point on the HIGH dwords of d = w - min (doubles, d > 0 for a point in range): for
 * positive doubles the high dword (exponent + 20 mantissa bits) orders like an unsigned integer, so a point costs two
 * subtractions and four 32-bit min / max (round 3: two subtractions, two multiplications, two conversions, a pack and two
 * packed min / max), and the reduction over the 16 lanes of a DPP row is one v_min_u32_dpp / v_max_u32_dpp per step and
 * value.  Only the cell's four results are turned into grid cells (lanes 0, 16, 32, 48): the minimum with the low dword 0
 * (rounded down), the maximum with the high dword + 1 (rounded up) - the box can only grow by that, never lose a point:
 * "a cell's box [x0, x1] x [y0, y1] holds points with xMin + x0 / boxX <= x < xMin + (x1 + 1) / boxX" (live_box_thresholds)
 * stays true. */
__device__ __forceinline__ unsigned int row_min_u32(unsigned int v)
{
  v = min(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x128, 0xf, 0xf, false)));
  v = min(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x124, 0xf, 0xf, false)));
  v = min(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x122, 0xf, 0xf, false)));
  v = min(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x121, 0xf, 0xf, false)));
  return v;
}
__device__ __forceinline__ unsigned int row_max_u32(unsigned int v)
{
  v = max(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x128, 0xf, 0xf, false)));
  v = max(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x124, 0xf, 0xf, false)));
  v = max(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x122, 0xf, 0xf, false)));
  v = max(v, static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x121, 0xf, 0xf, false)));
  return v;
}
/* The box of a cell from the four extremes' high dwords: a minimum with the low dword 0 is the lowest the distance can have
 * been (its cell is below 256: the distance is below the range), a maximum with the NEXT high dword the highest (clamped). */
__device__ __forceinline__ unsigned int cell_box_from_high_dwords(unsigned int x0, unsigned int x1, unsigned int y0, unsigned int y1,
                                                                  double boxX, double boxY)
{
  const unsigned int cx0 = static_cast<unsigned int>(__hiloint2double(static_cast<int>(x0), 0) * boxX);
  const unsigned int cy0 = static_cast<unsigned int>(__hiloint2double(static_cast<int>(y0), 0) * boxY);
  const unsigned int cx1 = min(static_cast<unsigned int>(__hiloint2double(static_cast<int>(x1 + 1u), 0) * boxX), 255u);
  const unsigned int cy1 = min(static_cast<unsigned int>(__hiloint2double(static_cast<int>(y1 + 1u), 0) * boxY), 255u);
  return (cx0 | (cx1 << 8)) | ((cy0 | (cy1 << 8)) << 16);
}

/* The list of the cells of a block's chunk whose mask meets `wanted`, in LDS, COLUMN-major: the cells of one
 * cell column (`cols` cells apart: vertically adjacent in the camera image) follow each other, so a wave that walks
 * the list stays on one patch of the top-down image that creeps down row by row — what its LDS write-combining
 * window needs — and jumps only at a column change.  Entries are cell indices relative to the chunk's first cell.
 * wantCell(record) decides from the cell's record (x = mask of the groups of 4 height bins that occur, y = bounding box,
 * x0 | x1 << 8 | y0 << 16 | y1 << 24 on the 256 x 256 grid) whether the cell is walked.
 * All threads of the block call it; returns the number of entries (block-uniform).  scratch: 2 * kWavesPerBlock words. */
template<typename Want>
__device__ __forceinline__ int cell_list_build(const uint2 *__restrict__ cellInfo, int nCells, int cols, Want wantCell,
                                               unsigned short *list, unsigned int *scratch)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rows = (nCells + cols - 1) / cols;
  constexpr int kFastPasses = 2;                 /* chunks of up to 32 tiles: the product's geometry for batches */
  if(rows * cols <= kFastPasses * kThreads)
  {
    /* All records of the chunk requested at once, every pass's ballot taken, ONE barrier for the counts, one for the list:
     * two barriers and one memory round trip, where the loop below pays two of each per 256 cells (measured: the list was
     * 11 % of a block's life in k_raster and k_inquad). */
    int cidx[kFastPasses];
    uint2 rec[kFastPasses];
#pragma unroll
    for(int p = 0; p < kFastPasses; p++)
    {
      const int i = p * kThreads + tid;
      const int cx = i / rows, r = i - cx * rows;
      const int c = r * cols + cx;
      cidx[p] = (cx < cols && c < nCells) ? c : -1;
      rec[p] = cidx[p] >= 0 ? cellInfo[c] : make_uint2(0u, 0u);
    }
    bool want[kFastPasses];
    int pos[kFastPasses];
#pragma unroll
    for(int p = 0; p < kFastPasses; p++)
    {
      want[p] = cidx[p] >= 0 && wantCell(rec[p]);
      const unsigned long long b = __ballot(want[p]);
      pos[p] = __popcll(b & ((1ull << lane) - 1ull));
      if(lane == 0)
        scratch[p * kWavesPerBlock + wave] = static_cast<unsigned int>(__popcll(b));
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for(int p = 0; p < kFastPasses; p++)
    {
      int before = total;
#pragma unroll
      for(int w = 0; w < kWavesPerBlock; w++)
      {
        const int n = static_cast<int>(scratch[p * kWavesPerBlock + w]);
        before += w < wave ? n : 0;
        total += n;
      }
      if(want[p])
        list[before + pos[p]] = static_cast<unsigned short>(cidx[p]);
    }
    __syncthreads();
    return total;
  }
  int total = 0;
  for(int i0 = 0; i0 < rows * cols; i0 += kThreads)
  {
    const int i = i0 + tid;
    const int cx = i / rows, r = i - cx * rows;
    const int c = r * cols + cx;
    const bool want = cx < cols && c < nCells && wantCell(cellInfo[c]);
    const unsigned long long b = __ballot(want);
    if(lane == 0)
      scratch[wave] = static_cast<unsigned int>(__popcll(b));
    __syncthreads();
    int before = total;
#pragma unroll
    for(int w = 0; w < kWavesPerBlock; w++)
    {
      const int n = static_cast<int>(scratch[w]);
      before += w < wave ? n : 0;
      total += n;
    }
    if(want)
      list[before + __popcll(b & ((1ull << lane) - 1ull))] = static_cast<unsigned short>(c);
    __syncthreads();
  }
  return total;
}

/* A wave takes a contiguous run of GROUPS of four list entries; DPP row q (lanes 16q .. 16q+15) takes entry 4g + q:
 * its 16 lanes read the cell's 768 bytes contiguously, four consecutive points per lane.  Rows beyond the end of the
 * list get invalid points (z = 0), which every consumer drops first. */
template<int SRC>
__device__ __forceinline__ void load_cell(const float *__restrict__ base, int cell0, const unsigned short *list, int entry, int count,
                                          int lane, int nPoints, F3 (&v)[kPts], const DepthSrc &D)
{
  if(entry < count)
    load_points<SRC>(base, (cell0 + static_cast<int>(list[entry])) * kCell + kPts * (lane & 15), nPoints, v, D);
  else
  {
#pragma unroll
    for(int j = 0; j < kPts; j++)
      v[j] = F3{ 0.0f, 0.0f, 0.0f };
  }
}

} // namespace ssd

#endif /* SSD_K_CELLS_H_ */
