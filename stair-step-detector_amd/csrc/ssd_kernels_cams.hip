/*
 * ssd_kernels_cams.hip - the entry points of cameras batches (ssd_enqueue_cameras) and their launchers.
 *
 * A cameras batch names, frame by frame, the camera each frame comes from.  Every kernel of the chain already sits on one frame
 * per block, so each entry point here takes the handle's camera table and the batch's index (frame -> camera) in place of the
 * by-value constants, fetches the frame's CameraRec at block start and runs the SAME device body as its one-calibration sibling:
 * this file includes ssd_kernels.hip with SSD_CAMERAS_TU defined, which gives the bodies without that file's entry points and
 * launchers (see the note at its top).  A translation unit of its own, so that the one-calibration kernels' code is not touched
 * by what is instantiated here.
 */
#define SSD_CAMERAS_TU
#include "ssd_kernels.hip"

namespace ssd
{

/* camera_of (ssd_device.h) gives the frame's record; the streaming kernels copy the parts they use at block start, as their siblings
 * get them by value. */
template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads, 6) void k_hist_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                        const int *__restrict__ camOf, FrameState *__restrict__ st, uint2 *__restrict__ tileMasks,
                                                        size_t tileMaskStride, int chunkPoints)
{
  __shared__ HistLds L;
  NoSpecLds none;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const DepthSrc D = C.D;
  hist_block<SRC, false, false, CHECKS>(L, none, xyz, strideFloats, P, Q, PixelParams{}, st, tileMasks, nullptr, tileMaskStride, chunkPoints, D, blockIdx.x, blockIdx.y);
}

template<int SRC, bool STRIPS, bool CHECKS>
__global__ __launch_bounds__(kThreads, SSD_K1S_WAVES) void k_hist_planes_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                   const int *__restrict__ camOf, FrameState *__restrict__ st, uint2 *__restrict__ tileMasks,
                                                   unsigned long long *__restrict__ planeImg, size_t tileMaskStride, int chunkPoints)
{
  __shared__ HistLds L;
  __shared__ SpecLds SL;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const PixelParams X = C.P.px;
  const DepthSrc D = C.D;
  hist_block<SRC, true, STRIPS, CHECKS>(L, SL, xyz, strideFloats, P, Q, X, st, tileMasks, planeImg, tileMaskStride, chunkPoints, D, blockIdx.x, blockIdx.y);
}

template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_predict_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                           const int *__restrict__ camOf, FrameState *__restrict__ st, int sabotage, int *__restrict__ fallback, int poolPlanes)
{
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const DepthSrc D = C.D;
  predict_block<SRC, CHECKS>(xyz, strideFloats, P, Q, st, D, C.P.minHeight, sabotage, fallback, poolPlanes);
}

__global__ __launch_bounds__(64) void k_peaks_cams(const CameraRec *__restrict__ cams, const int *__restrict__ camOf, FrameState *__restrict__ st, int nframes,
                                                   DebugFrame *__restrict__ dbg, int spec, int *__restrict__ fallback)
{
  if(static_cast<int>(blockIdx.x) >= nframes)
    return;
  peaks_block(camera_of(cams, camOf, blockIdx.x).P, st, nframes, dbg, spec, fallback);
}

template<int SRC, bool LIST>
__global__ __launch_bounds__(kThreads, LIST ? 5 : SSD_K2_WAVES) void k_raster_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                        const int *__restrict__ camOf, FrameState *__restrict__ st,
                                                        unsigned long long *__restrict__ stepImg,
                                                        const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints,
                                                        const int *__restrict__ fallback)
{
  __shared__ RasterLds L;
  if constexpr(LIST)
  {
    const int n = fallback[0];
    for(int e = blockIdx.x; e < n; e += gridDim.x)
    {
      const int frame = fallback[kFallbackList + e];
      const CameraRec &C = camera_of(cams, camOf, frame);
      const PointParams P = C.P.pt;
      const PixelParams X = C.P.px;
      const DepthSrc D = C.D;
      raster_block<SRC>(L, xyz, strideFloats, P, X, st, stepImg, tileMasks, tileMaskStride, chunkPoints, D, frame, blockIdx.y);
      __syncthreads();
    }
  }
  else
  {
    const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
    const PointParams P = C.P.pt;
    const PixelParams X = C.P.px;
    const DepthSrc D = C.D;
    raster_block<SRC>(L, xyz, strideFloats, P, X, st, stepImg, tileMasks, tileMaskStride, chunkPoints, D, blockIdx.x, blockIdx.y);
  }
}

template<int T>
__global__ __launch_bounds__(T) void k_outline_cams(const CameraRec *__restrict__ cams, const int *__restrict__ camOf, FrameState *__restrict__ st,
                                                    unsigned long long *__restrict__ stepImg,
                                                    unsigned long long *__restrict__ planeImg,
                                                    DebugFrame *__restrict__ dbg,
                                                    unsigned long long *__restrict__ dbgImg)
{
  outline_block<T>(camera_of(cams, camOf, blockIdx.x).P, st, stepImg, planeImg, dbg, dbgImg);
}

__global__ __launch_bounds__(64) void k_quads_cams(const CameraRec *__restrict__ cams, const int *__restrict__ camOf, FrameState *__restrict__ st, int nframes,
                                                   DebugFrame *__restrict__ dbg)
{
  if(static_cast<int>(blockIdx.x) >= nframes)
    return;
  quads_block(camera_of(cams, camOf, blockIdx.x).P, st, nframes, dbg);
}

template<int SRC, bool FULL, bool CHECKS>
__global__ __launch_bounds__(kThreads, FULL ? 4 : SSD_K4_WAVES) void k_inquad_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                        const int *__restrict__ camOf, FrameState *__restrict__ st,
                                                        unsigned long long *__restrict__ groundImg,
                                                        const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints)
{
  __shared__ InquadLds<FULL> L;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const PixelParams X = C.P.px;
  const DepthSrc D = C.D;
  const int nChunks = static_cast<int>(gridDim.y), first = max(1, nChunks / 8), by = static_cast<int>(blockIdx.y);    /* the order of k_inquad */
  const int chunkIdx = by < first ? nChunks - 1 - by : by - first;
  inquad_block<SRC, FULL, CHECKS>(L, xyz, strideFloats, P, Q, X, st, groundImg, tileMasks, tileMaskStride, chunkPoints, D, blockIdx.x, chunkIdx);
}

template<int T>
__global__ __launch_bounds__(T) void k_final_cams(const CameraRec *__restrict__ cams, const int *__restrict__ camOf, FrameState *__restrict__ st,
                                                  unsigned long long *__restrict__ groundImg,
                                                  ssd_frame_result *__restrict__ results,
                                                  DebugFrame *__restrict__ dbg,
                                                  unsigned long long *__restrict__ dbgImg)
{
  final_block<T>(camera_of(cams, camOf, blockIdx.x).P, st, groundImg, results, dbg, dbgImg);
}

template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_labels_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                          const int *__restrict__ camOf, const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                          size_t tileMaskStride, int chunkPoints,
                                                          unsigned char *__restrict__ labels, size_t labelStride)
{
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const DepthSrc D = C.D;
  labels_block<SRC, CHECKS>(xyz, strideFloats, P, Q, st, tileMasks, tileMaskStride, chunkPoints, D, labels, labelStride);
}

template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_surface_moments_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                                   const int *__restrict__ camOf, const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                                   size_t tileMaskStride, int chunkPoints, ssd_frame_moments *__restrict__ out)
{
  __shared__ SurfaceLds S;
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const PreXY Q = C.P.pre;
  const DepthSrc D = C.D;
  labelled_moments_block<SRC, CHECKS, false>(S, nullptr, xyz, strideFloats, P, Q, st, tileMasks, tileMaskStride, chunkPoints, D, nullptr, out);
}

template<int SRC>
__global__ __launch_bounds__(kThreads, 8) void k_risers_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                             const int *__restrict__ camOf, FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                             size_t tileMaskStride, int chunkPoints)
{
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const DepthSrc D = C.D;
  risers_block<SRC>(xyz, strideFloats, P, C.P.riserTol, st, tileMasks, tileMaskStride, chunkPoints, C.P.px.cellCols, D);
}

template<int SRC>
__global__ __launch_bounds__(kThreads) void k_riser_moments_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                                 const int *__restrict__ camOf, FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                                 size_t tileMaskStride, int chunkPoints, ssd_frame_moments *__restrict__ out)
{
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const DepthSrc D = C.D;
  riser_moments_block<SRC>(xyz, strideFloats, P, C.P.riserTol, st, tileMasks, tileMaskStride, chunkPoints, C.P.px.cellCols, D, out);
}

template<int SRC>
__global__ __launch_bounds__(kThreads, 8) void k_riser_labels_cams(const float *__restrict__ xyz, size_t strideFloats, const CameraRec *__restrict__ cams,
                                                                   const int *__restrict__ camOf, const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                                   size_t tileMaskStride, int chunkPoints,
                                                                   unsigned char *__restrict__ labels, size_t labelStride)
{
  const CameraRec &C = camera_of(cams, camOf, blockIdx.x);
  const PointParams P = C.P.pt;
  const DepthSrc D = C.D;
  riser_labels_block<SRC>(xyz, strideFloats, P, C.P.riserTol, st, tileMasks, tileMaskStride, chunkPoints, C.P.px.cellCols, D, labels, labelStride);
}

/* one thread per frame here, so the record is the thread's own (a few constants of it, once per frame) */
__global__ void k_riser_results_cams(const CameraRec *__restrict__ cams, const int *__restrict__ camOf, const FrameState *__restrict__ st,
                                     ssd_frame_risers *__restrict__ out, int nframes)
{
  const int frame = blockIdx.x * blockDim.x + threadIdx.x;
  if(frame >= nframes)
    return;
  riser_results_block(cams[camOf[frame]].P, st, out, nframes);
}


/* ========================================================================= */
/* launchers (declared with the launch rules in ssd_kernels.hip, which the one-calibration launchers share with these: the same grids,
 * block sizes and instantiations by construction) */

void launch_predict_cams(const Batch &B, int *fallback, int poolPlanes, int sabotage)
{
  with_predict(B, [&](auto src, auto checks, const DepthSrc &)
  {
    hipLaunchKernelGGL((k_predict_cams<decltype(src)::value, decltype(checks)::value>), grid_predict(B), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, sabotage, fallback, poolPlanes);
  });
}
void launch_hist_cams(const Batch &B, int chunkPoints, unsigned long long *planeImg)
{
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &)
  {
    constexpr int SRC = decltype(src)::value;
    constexpr bool CHECKS = decltype(checks)::value;
    if(planeImg)
      with_bool(hist_strips(B, planeImg), [&](auto sorted)
      {
        hipLaunchKernelGGL((k_hist_planes_cams<SRC, decltype(sorted)::value, CHECKS>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, planeImg, B.tileMaskStride, chunkPoints);
      });
    else
      hipLaunchKernelGGL((k_hist_cams<SRC, CHECKS>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints);
  });
}
void launch_peaks_cams(const Batch &B, DebugFrame *dbg, int *fallback)
{
  hipLaunchKernelGGL(k_peaks_cams, grid_frames(B), dim3(64), 0, B.s, B.cams->table, B.cams->index, B.st, B.nframes, dbg, fallback ? 1 : 0, fallback);
}
void launch_raster_cams(const Batch &B, int chunkPoints, unsigned long long *stepImg, const int *fallback)
{
  with_src(B, [&](auto src, const DepthSrc &)
  {
    with_bool(fallback != nullptr, [&](auto listed)
    {
      hipLaunchKernelGGL((k_raster_cams<decltype(src)::value, decltype(listed)::value>), grid_raster(B, chunkPoints, fallback != nullptr), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, stepImg, B.tileMasks, B.tileMaskStride, chunkPoints, fallback);
    });
  });
}
void launch_outline_cams(const Batch &B, unsigned long long *stepImg, unsigned long long *planeImg, DebugFrame *dbg, unsigned long long *dbgImg)
{
  with_img_threads(B, [&](auto t)
  {
    hipLaunchKernelGGL(k_outline_cams<decltype(t)::value>, grid_images(B), dim3(decltype(t)::value), 0, B.s, B.cams->table, B.cams->index, B.st, stepImg, planeImg, dbg, dbgImg);
  });
}
void launch_quads_cams(const Batch &B, DebugFrame *dbg)
{
  hipLaunchKernelGGL(k_quads_cams, grid_frames(B), dim3(64), 0, B.s, B.cams->table, B.cams->index, B.st, B.nframes, dbg);
}
void launch_inquad_cams(const Batch &B, int chunkPoints, unsigned long long *groundImg)
{
  with_inquad(B, [&](auto src, auto full, auto checks, const DepthSrc &)
  {
    hipLaunchKernelGGL((k_inquad_cams<decltype(src)::value, decltype(full)::value, decltype(checks)::value>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, groundImg, B.tileMasks, B.tileMaskStride, chunkPoints);
  });
}
void launch_final_cams(const Batch &B, unsigned long long *groundImg, ssd_frame_result *results, DebugFrame *dbg, unsigned long long *dbgImg)
{
  with_img_threads(B, [&](auto t)
  {
    hipLaunchKernelGGL(k_final_cams<decltype(t)::value>, grid_frames(B), dim3(decltype(t)::value), 0, B.s, B.cams->table, B.cams->index, B.st, groundImg, results, dbg, dbgImg);
  });
}
void launch_labels_cams(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride)
{
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &)
  {
    hipLaunchKernelGGL((k_labels_cams<decltype(src)::value, decltype(checks)::value>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, labels, labelStride);
  });
}
void launch_surface_moments_cams(const Batch &B, int chunkPoints, ssd_frame_moments *out)
{
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &)
  {
    hipLaunchKernelGGL((k_surface_moments_cams<decltype(src)::value, decltype(checks)::value>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, out);
  });
}
static void launch_riser_results_cams(const Batch &B, ssd_frame_risers *out)
{
  hipLaunchKernelGGL(k_riser_results_cams, grid_frame_threads(B), dim3(64), 0, B.s, B.cams->table, B.cams->index, B.st, out, B.nframes);
}
void launch_risers_cams(const Batch &B, int chunkPoints, ssd_frame_risers *out)
{
  with_src(B, [&](auto src, const DepthSrc &)
  {
    hipLaunchKernelGGL(k_risers_cams<decltype(src)::value>, grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints);
  });
  launch_riser_results_cams(B, out);
}
void launch_riser_moments_cams(const Batch &B, int chunkPoints, ssd_frame_risers *out, ssd_frame_moments *moments)
{
  with_src(B, [&](auto src, const DepthSrc &)
  {
    hipLaunchKernelGGL(k_riser_moments_cams<decltype(src)::value>, grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, moments);
  });
  launch_riser_results_cams(B, out);
}
void launch_riser_labels_cams(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride)
{
  with_src(B, [&](auto src, const DepthSrc &)
  {
    hipLaunchKernelGGL(k_riser_labels_cams<decltype(src)::value>, grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.cams->table, B.cams->index, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, labels, labelStride);
  });
}

} // namespace ssd
