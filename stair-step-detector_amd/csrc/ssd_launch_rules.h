/* ssd_launch_rules.h - the launch rules the translation units' launchers share (grid_*, with_*), and the cameras launchers' declarations.
 * Host code, included by the three units that launch the stage headers' kernels: DESIGN.md section 3b. */
#ifndef SSD_LAUNCH_RULES_H_
#define SSD_LAUNCH_RULES_H_
#include "ssd_launch.h"
#include <type_traits>
#include "ssd_k_point.h"    /* kTile, kSrc*; the image kernels' thread counts: ssd_k_entry.h */

namespace ssd
{
/* What the three translation units' launchers share: every launch rule once, over the Batch.  A launcher in ssd_kernels.hip, in
 * ssd_kernels_cams.hip or in ssd_kernels_refit.hip names its __global__ and that kernel's arguments, nothing else.
 *
 * Grid layout of every per-frame kernel: FRAME on the fast axis (blockIdx.x), chunk / image slot on the slow
 * one.  Workgroups are dealt round-robin over the 8 XCDs in linear-id order; with the chunk (or the image
 * slot) on the fast axis every XCD would always get the same chunk positions of every frame — the stairs
 * for some XCDs, the skipped ground for others (measured: +30 % on K2, and K3 running on half of the XCDs
 * because only slots 0..3 hold images).  Frame-fastest gives each XCD whole frames: balanced, and a frame's
 * state and images stay in one XCD's L2. */
static inline int chunks_for(int nPoints, int chunkPoints) { return (nPoints + chunkPoints - 1) / chunkPoints; }
static inline dim3 grid_frames(const Batch &B) { return dim3(B.nframes); }                          /* a block per frame */
static inline dim3 grid_frame_threads(const Batch &B) { return dim3((B.nframes + 63) / 64); }      /* a thread per frame, blocks of 64 */
static inline dim3 grid_predict(const Batch &B) { return dim3(B.nframes, kPredictParts); }
static inline dim3 grid_images(const Batch &B) { return dim3(B.nframes, B.P.maxStepImages); }
static inline dim3 grid_stream(const Batch &B, int chunkPoints) { return dim3(B.nframes, chunks_for(B.P.nPoints, chunkPoints)); }
/* k_raster with the single pass's list: a block takes every fourth listed frame in turn */
static inline dim3 grid_raster(const Batch &B, int chunkPoints, bool listed)
{
  return dim3(listed ? (B.nframes + 3) / 4 : B.nframes, chunks_for(B.P.nPoints, chunkPoints));
}
/* K1 in the single pass - a tile a whole number of camera rows: the tile loop keeps every wave in its band of columns; else the sorted strips */
static inline bool hist_strips(const Batch &B, const unsigned long long *planeImg) { return planeImg && kTile % B.P.W != 0; }

/* a run-time bool as std::true_type / std::false_type */
template<typename F>
static inline void with_bool(bool b, F f)
{
  if(b)
    f(std::true_type{});
  else
    f(std::false_type{});
}
/* The point source of a launch as a compile-time constant: f(std::integral_constant<int, kSrc...>, the DepthSrc to pass) */
template<typename F>
static inline void with_src(const Batch &B, F f)
{
  if(B.depthInput)
    f(std::integral_constant<int, kSrcDepth16>{}, B.depth);
  else if((reinterpret_cast<uintptr_t>(B.xyz) & 15u) == 0 && (B.strideFloats & 3u) == 0 && (B.P.nPoints & 3) == 0)
    f(std::integral_constant<int, kSrcF3Aligned>{}, DepthSrc{});
  else
    f(std::integral_constant<int, kSrcF3>{}, DepthSrc{});
}
/* ... and CHECKS with it, f(src, checks, DepthSrc): a cameras batch by its table, a one-calibration batch by its constants */
template<typename F>
static inline void with_src_checks(const Batch &B, F f)
{
  with_src(B, [&](auto src, const DepthSrc &D) { with_bool(B.cams ? B.cams->checks : needs_checks(B.P), [&](auto checks) { f(src, checks, D); }); });
}
/* k_predict's: the depth loop has no pre-filter, so it has the one instantiation without CHECKS */
template<typename F>
static inline void with_predict(const Batch &B, F f)
{
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &D)
  {
    if constexpr(decltype(src)::value == kSrcDepth16)
      f(src, std::false_type{}, D);
    else
      f(src, checks, D);
  });
}
/* k_inquad's, f(src, full, checks, DepthSrc): debug capture (the whole ground image: the handle's, so the same for every camera) always
 * takes the instantiation with the rare configurations' tests */
template<typename F>
static inline void with_inquad(const Batch &B, F f)
{
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &D)
  {
    if(B.P.px.groundFull)
      f(src, std::true_type{}, std::true_type{}, D);
    else
      f(src, std::false_type{}, checks, D);
  });
}
/* k_outline's and k_final's threads, f(std::integral_constant<int, T>): while every image has a CU of its own, the block that gets
 * through its phases soonest; beyond that the cheapest */
template<typename F>
static inline void with_img_threads(const Batch &B, F f)
{
  if(B.nframes <= kImgFewFrames)
    f(std::integral_constant<int, kImgThreadsFew>{});
  else
    f(std::integral_constant<int, kImgThreadsBatch>{});
}

/* the launchers of the cameras entry points (ssd_kernels_cams.hip): what launch_*(B, ...) hands a batch with B.cams to */
void launch_predict_cams(const Batch &B, int *fallback, int poolPlanes, int sabotage);
void launch_hist_cams(const Batch &B, int chunkPoints, unsigned long long *planeImg);
void launch_peaks_cams(const Batch &B, DebugFrame *dbg, int *fallback);
void launch_raster_cams(const Batch &B, int chunkPoints, unsigned long long *stepImg, const int *fallback);
void launch_outline_cams(const Batch &B, unsigned long long *stepImg, unsigned long long *planeImg, DebugFrame *dbg, unsigned long long *dbgImg);
void launch_quads_cams(const Batch &B, DebugFrame *dbg);
void launch_inquad_cams(const Batch &B, int chunkPoints, unsigned long long *groundImg);
void launch_final_cams(const Batch &B, unsigned long long *groundImg, ssd_frame_result *results, DebugFrame *dbg, unsigned long long *dbgImg);
void launch_surface_moments_cams(const Batch &B, int chunkPoints, ssd_frame_moments *out);
void launch_labels_cams(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride);
void launch_risers_cams(const Batch &B, int chunkPoints, ssd_frame_risers *out);
void launch_riser_moments_cams(const Batch &B, int chunkPoints, ssd_frame_risers *out, ssd_frame_moments *moments);
void launch_riser_labels_cams(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride);
} // namespace ssd

#endif /* SSD_LAUNCH_RULES_H_ */
