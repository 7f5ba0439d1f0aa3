/*
 * ssd_kernels_refit.hip - the trimmed surface refit's kernels (ssd_enqueue_surface_refit, DESIGN.md section 7g;
 * ssd_enqueue_cameras_surface_refit, section 7h) and their launchers.
 *
 * k_surface_refit is k_surface_moments' body, labelled_moments_block (ssd_k_moments.h), with GATED on: the same cells from K1's records,
 * the same decision (quad_decide<.., true>), the same load, the same accumulation - and a gate test between the label and the sums;
 * k_surface_refit_cams runs it with the frame's camera record in place of the handle's by-value constants.  A translation unit of its
 * own, so that no kernel of the chain is touched by what is instantiated here; it includes the stage headers it builds on and the launch
 * rules, and nothing of the chain.  SSD_CAMERAS_TU is defined in front as in ssd_kernels_cams.hip: the unit has _cams entry points, k_labels
 * stays a device function here, and the tools builds' clocks and counters stay off (ssd_k_entry.h).
 */
#define SSD_CAMERAS_TU
#include "ssd_k_moments.h"
#include "ssd_launch_rules.h"

namespace ssd
{

static_assert(sizeof(ssd_plane_gate) == 40 && sizeof(ssd_frame_gates) == 8 + SSD_MAX_STEPS * sizeof(ssd_plane_gate),
              "ssd_frame_gates is staged as 64-bit words: a header of two int32, then five doubles per surface");

struct RefitLds
{
  SurfaceLds s;                                  /* k_surface_moments', unchanged */
  ssd_frame_gates gates;                         /* the frame's, fetched once per block */
};

/* The header is written as the first pass writes it, from the same FrameState. */
template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_surface_refit(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q,
                                                            const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                            size_t tileMaskStride, int chunkPoints, DepthSrc D,
                                                            const ssd_frame_gates *__restrict__ gates, ssd_frame_moments *__restrict__ out)
{
  __shared__ RefitLds R;
  labelled_moments_block<SRC, CHECKS, true>(R.s, &R.gates, xyz, strideFloats, P, Q, st, tileMasks, tileMaskStride, chunkPoints, D, gates, out);
}

/* The cameras batch's entry point, shaped like k_surface_moments_cams: the frame's record by scalar loads at block start, the parts the
 * body uses copied, the same body.  The gates stay the FRAME's (gates + frame): two frames of one camera may carry different ones. */
template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_surface_refit_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                                 const int *__restrict__ camOf, const FrameState *__restrict__ st,
                                                                 const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints,
                                                                 const ssd_frame_gates *__restrict__ gates, ssd_frame_moments *__restrict__ out)
{
  __shared__ RefitLds R;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const DepthSrc D = C.D;
  labelled_moments_block<SRC, CHECKS, true>(R.s, &R.gates, xyz, strideFloats, P, Q, st, tileMasks, tileMaskStride, chunkPoints, D, gates, out);
}

/* grid, block size and instantiations are launch_surface_moments' (ssd_launch_rules.h); a cameras batch: CHECKS by the
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

/* the other pass behind a whole enqueue, the tread clearance, in this translation unit: one parse of the shared headers */
#include "ssd_kernels_clearance.hip"
/* ... and the tread grid (section 7n), which is built on it */
#include "ssd_kernels_treadgrid.hip"
/* ... and the stair map (section 7p), which is the tread grid's walk with another source and destination */
#include "ssd_kernels_stairmap.hip"
