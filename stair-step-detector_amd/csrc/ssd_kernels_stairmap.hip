/*
 * ssd_kernels_stairmap.hip - the stair map pass (ssd_enqueue_stair_map, ssd_enqueue_cameras_stair_map) and its
 * launcher.
 *
 * The tread grid's walk (tread_grid_block, ssd_kernels_treadgrid.hip: one text, not a copy) with another `where`: a block's staircase is
 * the caller's map that its frame names, not the frame's own result, and its counts go to that map's record, which the blocks of every
 * frame that names the map share.  The rule, the LDS staging and the flush are the tread grid's: the counts reach memory as one global
 * atomic per non-zero cell per block, not per point, and the occupants' heights as an atomic maximum each - integer adds and maxima,
 * so no byte depends on which frame's block comes first.  The record is shared by many frames' blocks and occupants need not be rare
 * (a frame that does not show the map's staircase), so the word is read first and the atomic sent only for a height above it
 * (kSharedRecord; what an atomic per occupant cost: DESIGN.md section 7p, Time).
 * The bins and the transform are still the frame's own (its camera's in a cameras batch); the candidate tables are built from the
 * map's surfaces against those bins and are supersets as before.
 * The file is compiled at the end of ssd_kernels_refit.hip, behind ssd_kernels_treadgrid.hip.
 */
#include "ssd_k_walk.h"     /* tread_grid_block's walk */
#include "ssd_launch_rules.h"
#include "ssd_treadgrid.h"

namespace ssd
{

static_assert(sizeof(ssd_stair_map) == sizeof(ssd_frame_result) + 8 && sizeof(ssd_stair_map) == 1240, "ssd_stair_map is the kernel's record");
static_assert(SSD_MAX_STAIR_MAPS <= kThreads, "the headers of all maps are written by one block, a thread per map");
static_assert(SSD_STAIR_MAP_NONE >= SSD_MAX_STAIR_MAPS, "the index of no map is no map's index");

/* tread_grid_block's `where` for a stair map: the frame's map index by a scalar load at block start (the address depends on the frame
 * alone); a frame that names no map - SSD_STAIR_MAP_NONE, or anything else that is not below nmaps - adds nothing.  The headers of all
 * nmaps records are written by one block (frame 0, chunk 0; a thread per map), whatever its own map is: what ssd_tread_grid_host writes
 * for the map's staircase, and zeros for one that threw or has no step.  The staircases are the maps', so the body's `results` is null. */
struct TreadGridStairMap
{
  static constexpr bool kEveryFrame = false;
  static constexpr bool kSharedRecord = true;    /* every frame of a map adds to its record: the tops are read before they are raised */
  const ssd_stair_map *__restrict__ maps;
  const int *__restrict__ mapOf;
  int nmaps;
  __device__ __forceinline__ int index(int frame) const
  {
    const int m = mapOf[frame];
    return m < nmaps ? m : -1;
  }
  __device__ __forceinline__ void header(int frame, int tid, ssd_frame_tread_grid *__restrict__ out) const
  {
    if(frame == 0 && blockIdx.y == 0 && tid < nmaps && SSD_CHK(36, tid, SSD_MAX_STAIR_MAPS))
    {
      const ssd_frame_result &r = maps[tid].stairs;
      const int n = (r.status & SSD_ST_THROW) ? 0 : min(max(r.n_steps, 0), SSD_MAX_STEPS);
      out[tid].n_surfaces = n;
      out[tid].ground = (n > 0 && maps[tid].ground != 0) ? 1 : 0;
    }
  }
  __device__ __forceinline__ const ssd_frame_result &result(const ssd_frame_result *, int at) const { return maps[at].stairs; }
};

template<int SRC>
__global__ __launch_bounds__(kThreads) void k_stair_map(const float *__restrict__ xyz, size_t strideFloats, PointParams P, ClearanceWorld X,
                                                        const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints, DepthSrc D,
                                                        const ssd_stair_map *__restrict__ maps, const int *__restrict__ mapOf, int nmaps,
                                                        ssd_tread_grid_rule rule, ssd_frame_tread_grid *__restrict__ out)
{
  __shared__ TreadGridLds L;
  tread_grid_block<SRC>(L, xyz, strideFloats, P, X, TreadGridStairMap{ maps, mapOf, nmaps }, tileMasks, tileMaskStride, chunkPoints, D, nullptr, rule, out);
}

/* The cameras batch's entry point, shaped like k_tread_grid_cams: the frame's camera by scalar loads at block start, the same body. */
template<int SRC>
__global__ __launch_bounds__(kThreads) void k_stair_map_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                             const int *__restrict__ camOf, const uint2 *__restrict__ tileMasks,
                                                             size_t tileMaskStride, int chunkPoints, const ssd_stair_map *__restrict__ maps,
                                                             const int *__restrict__ mapOf, int nmaps, ssd_tread_grid_rule rule,
                                                             ssd_frame_tread_grid *__restrict__ out)
{
  __shared__ TreadGridLds L;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const ClearanceWorld X{ { C.P.r2[0], C.P.r2[1], C.P.r2[2], C.P.r2[3] }, { C.P.t2[0], C.P.t2[1] }, C.P.worldZ };
  const DepthSrc D = C.D;
  tread_grid_block<SRC>(L, xyz, strideFloats, P, X, TreadGridStairMap{ maps, mapOf, nmaps }, tileMasks, tileMaskStride, chunkPoints, D, nullptr, rule, out);
}

/* grid and block size are launch_tread_grid's */
void launch_stair_map(const Batch &B, int chunkPoints, const ssd_stair_map *maps, const int *mapOf, int nmaps, const ssd_tread_grid_rule &rule,
                      ssd_frame_tread_grid *out)
{
  const Params &P = B.P;
  const ClearanceWorld X{ { P.r2[0], P.r2[1], P.r2[2], P.r2[3] }, { P.t2[0], P.t2[1] }, P.worldZ };
  with_src(B, [&](auto src, const DepthSrc &D)
  {
    constexpr int SRC = decltype(src)::value;
    if(B.cams)
      hipLaunchKernelGGL((k_stair_map_cams<SRC>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.tileMasks, B.tileMaskStride, chunkPoints, maps, mapOf, nmaps, rule, out);
    else
      hipLaunchKernelGGL((k_stair_map<SRC>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, X, B.tileMasks, B.tileMaskStride, chunkPoints, D, maps, mapOf, nmaps, rule, out);
  });
}

} // namespace ssd
