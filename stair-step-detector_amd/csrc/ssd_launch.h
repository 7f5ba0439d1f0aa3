/* ssd_launch.h — host-callable launchers of the kernels in ssd_kernels.hip */
#ifndef SSD_LAUNCH_H_
#define SSD_LAUNCH_H_

#include "ssd_device.h"
#include "ssd_chunks.h"                     /* kTileHost and the kMaxTilesPerBlock*Host bounds, beside the chunk rules that read them */

namespace ssd
{
constexpr int kCellHost = 64;              /* points per cell (one gating mask each) */
/* The single pass (k_hist rasters the step plateaus itself) pays a kernel (k_predict) that a few frames do
 * not earn back; its keys hold 13 bits of row and its windows must fit the image. */
/* from 64 XGA frames per batch on (tools/sp_frames.py: 48 frames 3 % slower, 64 frames 4 % faster; VGA between 128 and 192
 * frames, FHD around 24-64): by points */
constexpr long long kSinglePassMinPoints = 64ll * 1024 * 768;
inline bool single_pass_batch(int nframes, int nPoints) { return static_cast<long long>(nframes) * nPoints >= kSinglePassMinPoints; }
constexpr int kSinglePassBackoff = 63;      /* batches run in two passes after one the single pass could not pay on (ssd_fetch_back) */
constexpr int kPredictParts = 4;            /* blocks of k_predict per frame */
/* The rare configurations' per-point tests (inputs beyond PreXY::maxInput that could read "inside", a z range that does not end on
 * a bin edge: ssd_prexy.h) live in instantiations of their own: as run-time flags they cost the common one two instructions per point */
inline bool needs_checks(const Params &P) { return P.pre.checkInput != 0 || P.pre.zCheckTop != 0; }
inline bool single_pass_geometry(int W, int H) { return W >= 64 && W <= 8192 && H >= 16 && H <= 4096; }
/* a launcher's test for a wide body: frames at p, strideBytes apart, all lie on k-byte boundaries */
inline bool aligned_to(const void *p, size_t strideBytes, size_t k) { return reinterpret_cast<size_t>(p) % k == 0 && strideBytes % k == 0; }

/* What every launcher of the chain is given: the handle's constants, the batch's frames, the workspace's per-frame state, the stream.
 * cams: a cameras batch - every launcher then hands the batch to its *_cams entry point (ssd_kernels_cams.hip, ssd_kernels_refit.hip)
 * with the table and the batch's index, CHECKS by cams->checks; P then gives only what the cameras share (resolution, points, image
 * slots) and depthInput only says that the source is 16-bit depth (each frame's DepthSrc is its camera's).  The kernels that only read
 * st / tileMasks declare them const; the record holds what the writers need. */
struct Batch
{
  const Params &P;
  const float *xyz;                           /* the frames (16-bit depth: the same pointer, read as unsigned short) */
  size_t strideFloats;                        /* between frames, in elements of the source type */
  bool depthInput;
  DepthSrc depth;                             /* the handle's deprojection; used while depthInput && !cams */
  FrameState *st;
  uint2 *tileMasks;
  size_t tileMaskStride;
  int nframes;
  hipStream_t s;
  const CameraSel *cams;
};

/* The single pass: launch_predict (k_predict; fallback = the batch's list of frames for k_raster - count, then indices: k_predict
 * resets it, k_peaks appends, k_raster reads; sabotage: see k_predict), then launch_hist with planeImg != nullptr (K1 rastering the
 * candidate bins' planes), launch_peaks / launch_raster with the list, launch_outline with the planes. */
void launch_predict(const Batch &B, int *fallback, int poolPlanes, int sabotage);
void launch_hist(const Batch &B, int chunkPoints, unsigned long long *planeImg);
void launch_peaks(const Batch &B, DebugFrame *dbg, int *fallback);
void launch_raster(const Batch &B, int chunkPoints, unsigned long long *stepImg, const int *fallback);
void launch_outline(const Batch &B, unsigned long long *stepImg, unsigned long long *planeImg, DebugFrame *dbg, unsigned long long *dbgImg);
void launch_quads(const Batch &B, DebugFrame *dbg);
void launch_inquad(const Batch &B, int chunkPoints, unsigned long long *groundImg);
void launch_final(const Batch &B, unsigned long long *groundImg, ssd_frame_result *results, DebugFrame *dbg, unsigned long long *dbgImg);
/* per-surface moments (k_surface_moments) after launch_final: frame i's record at out + i, zeroed by the caller on the stream in front of
 * the launch; chunkPoints as launch_labels' */
void launch_surface_moments(const Batch &B, int chunkPoints, ssd_frame_moments *out);
/* per-pixel surface labels (k_labels) after launch_final: frame i's W H labels at labels + i * labelStride; chunkPoints as launch_risers' */
void launch_labels(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride);
void launch_risers(const Batch &B, int chunkPoints, ssd_frame_risers *out);
/* launch_risers with the riser fit's moments (k_riser_moments in place of k_risers: one walk, both results): frame i's record at
 * moments + i, zeroed by the caller on the stream in front of the launch */
void launch_riser_moments(const Batch &B, int chunkPoints, ssd_frame_risers *out, ssd_frame_moments *moments);
/* the riser labels (k_riser_labels) behind launch_labels AND launch_risers / launch_riser_moments of the same batch on the same stream,
 * only while P.risers (k_final refreshes the state it reads only then): SSD_LABEL_RISER_BASE + i into the byte of every evidence point
 * of riser i, labels and labelStride as launch_labels'; grid and chunkPoints as launch_risers' */
void launch_riser_labels(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride);

/* k_surface_gates (ssd_kernels_solve.hip): rec[i] -> out[i] for nframes >= 1 records, both in device memory and not
 * overlapping, on stream s; every byte of out[0 .. nframes) is written, nothing behind them */
void launch_surface_gates(const ssd_frame_moments *rec, int nframes, int min_points, double k_sigma, double gate_min, ssd_frame_gates *out, hipStream_t s);
/* k_camera_fold and k_camera_ground_gates (ssd_kernels_fold.hip), on stream s, everything in device memory:
 * rec[0 .. nframes) under the index camOf (one int per frame) -> out[0 .. ncams), all 104 bytes of each, on top of what they hold when
 * `accumulate`; and the camera's gate from fold[0 .. ncams) over g[0] of gates[0 .. nframes), every other byte left as it is */
void launch_camera_fold(const ssd_frame_moments *rec, const int *camOf, int nframes, int ncams, bool accumulate, ssd_camera_fold *out, hipStream_t s);
void launch_camera_ground_gates(const ssd_frame_moments *rec, const int *camOf, int nframes, const ssd_camera_fold *fold, int ncams, int min_points,
                                double k_sigma, double gate_min, ssd_frame_gates *gates, hipStream_t s);
}

#endif /* SSD_LAUNCH_H_ */
