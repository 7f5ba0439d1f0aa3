/*
 * ssd_hip.h — C ABI of libssd_hip.so: the MI355X (gfx950) implementation of the
 * per-frame point-cloud path of peter-nebe/stair-step-detector.
 *
 * Drop-in boundary (reference file:line each entry point replaces; paths are
 * relative to the reference tree):
 *
 *   ssd_calibration_from_points  GeometricTransformation::GeometricTransformation(worldPoints, cameraPoints)
 *                                transformation.cpp:196-215 (+ :108-157, :94-106)
 *   ssd_create / ssd_destroy     Pointcloud::Pointcloud(window, trans)   pointcloud.cpp:602-606, pointcloud.h:32-42
 *                                + the compile-time Configuration          configuration.h:27-52, pointcloud.cpp:99-106
 *   ssd_process_host             Pointcloud::process(const Camera::DepthFrame&)   pointcloud.cpp:608-626
 *                                (the frame's xyz vertices = rs2::pointcloud::calculate output, pointcloud.cpp:138)
 *   ssd_enqueue / ssd_fetch      the same, for frames already resident in device memory, asynchronous
 *   ssd_serialize                Stairs::serialize()                     stairs.cpp:55-70 (byte-exact text line)
 *   ssd_get_debug                integer intermediates for parity tests (hist, peaks, images, scans, lines)
 *
 * Not in this library: the synthetic frame source that stands in for the camera (include/ssd_source.h,
 * libssd_source.so) and the hooks that let tests run pieces of the kernels in isolation (include/ssd_testhooks.h,
 * libssd_testhooks.so).
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions return
 * 0 on success or a negative SSD_E_* code; nothing throws across the boundary.
 * A handle is bound to one device and is not thread-safe (one host thread per GPU).
 * Streams: see ssd_config::batches_in_flight.  With one workspace a handle's calls execute on the caller's stream in the
 * order they were made; if a call names another stream than the previous one, the library orders it behind the previous
 * call with an event — correct, but the two do not overlap.  With several workspaces the batches run on streams of the
 * handle's own.  ssd_process_host / ssd_process_depth_host always use two non-blocking streams of the handle's own (copy and
 * compute) and return when the results are on the host; they do not synchronise with the legacy default stream.
 * Configuration limits: max(|z_min|, |z_max|) < 2048 m and max|z| * width * height < 2^23 (the mean height of a step
 * is accumulated in 2^-40 m fixed point), 3..SSD_MAX_BINS histogram bins, width <= 3175 ((width - 1) / 25 + 2 scan columns
 * <= SSD_MAX_SCANS), height <= 2560 ((height - 1) / 10 + 1 vertical-edge probe rows <= SSD_MAX_EDGE_PTS).
 */
#ifndef SSD_HIP_H_
#define SSD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSD_MAX_BINS 128          /* histogram bins the kernels support (reference default: 121) */
#define SSD_MAX_PLATEAUS 32       /* filtered histogram peaks per frame */
#define SSD_MAX_STEP_IMAGES 16    /* plateaus at or above minHeight per frame (each owns a bit image) */
#define SSD_MAX_STEPS (SSD_MAX_STEP_IMAGES + 1)
#define SSD_MAX_PLANES 24         /* single-pass batches: bit images of candidate height bins a frame can have */
#define SSD_POOL_PLANES_PER_FRAME 10   /* ... and how many the workspace holds per frame of max_frames_per_batch (a pool: frames draw what they need) */
#define SSD_MAX_SCANS 128
#define SSD_MAX_EDGE_PTS 256
#define SSD_LINE_CAP 4096
#define SSD_BATCHES_IN_FLIGHT_THROUGHPUT 3   /* ssd_config::batches_in_flight of a caller that enqueues ahead of its fetches */

/* error codes */
#define SSD_OK 0
#define SSD_E_ARG (-1)
#define SSD_E_HIP (-2)
#define SSD_E_NOMEM (-3)
#define SSD_E_NODEVICE (-4)
#define SSD_E_CAP (-5)

/* per-frame status bits (ssd_frame_result.status) */
#define SSD_ST_THROW 1         /* reference would have thrown std::invalid_argument (quadrilateralTest.cpp:283-372): no line */
#define SSD_ST_OOB_PIXEL 2     /* a point fell on pixel column W / row H (reference quirk Q5); dropped */
#define SSD_ST_ASSERT 4        /* a reference assert would have fired (segmentation.cpp:549-550, :254) */
#define SSD_ST_OVERFLOW 8      /* more plateaus than SSD_MAX_PLATEAUS / max_step_plateaus: frame truncated */

/* configuration.h:27-52 plus stream resolution and workspace sizing */
typedef struct
{
  int32_t width, height;
  double x_min, x_max, y_min, y_max, z_min, z_max;   /* Configuration::MeasuringRange */
  double height_interval;                            /* 0.01 */
  double min_height_above_ground;                    /* 0.05 */
  double min_step_depth;                             /* 0.1 */
  int32_t max_frames_per_batch;                      /* a workspace is sized for this many frames per call (ssd_workspace_bytes: about 1.75 MB per XGA
                                                        frame; 4.1 MB from 64 XGA frames' worth of points per batch on - such batches, as
                                                        vertices, run K1 and the step plateaus' raster as ONE pass over the input, with
                                                        SSD_MAX_PLANES more bit images per frame; results are the same either way) */
  int32_t max_step_plateaus;                         /* <= SSD_MAX_STEP_IMAGES */
  /* Workspaces of the handle = batches it keeps in flight (1..8; 0 = 1).
   * 1 (the default): every call runs on the caller's stream, strictly in stream order — enqueue, then refill the same frames
   *      on the same stream (or, on the NULL stream, with a plain hipMemcpy) is ordered, nothing to read further.
   * > 1 (opt-in; SSD_BATCHES_IN_FLIGHT_THROUGHPUT = 3 is what bench.py and detect-stairs-amd ask for): successive ssd_enqueue
   *      calls take the workspaces in turn, each on a stream of the handle's own, so that the launches of one batch fill the
   *      gaps the one-block-per-frame kernels of the others leave.  XGA, frames/s with 1 / 2 / 3 / 4 / 6 in flight
   *      (profiles/r03_depths.json): 1024 frames per call 272 k / 290 k / 301 k / 294 k / 307 k, 256: 237 k / 286 k / 306 k /
   *      295 k / 314 k, 64: 188 k / 248 k / 270 k / 251 k / 284 k, 16: 94 k / 165 k / 214 k / 170 k / 228 k (3 and 6 sit better
   *      than 4 and 5) — provided the caller enqueues ahead of its fetches.  Memory = batches_in_flight x 1.75 MB per XGA frame
   *      of max_frames_per_batch (1024 frames, 3 in flight: 5.4 GB beside 9.7 GB of frames; 4.1 MB per frame and 12.6 GB with the
   *      planes of the single pass, ssd_set_single_pass).  Stream contract then: a batch
   *      starts behind the work `stream` holds at the time of the call, but work put on `stream` afterwards is NOT ordered
   *      behind the batch — its frames must stay untouched until its results were fetched, or until a stream was made to wait
   *      for it with ssd_stream_wait.  ssd_process_host / ssd_process_depth_host cut a host batch into slices of at most 32
   *      frames, copied through two staging buffers on a copy stream of the handle's own; with one workspace the slices'
   *      kernels follow each other on the handle's compute stream, with several they take the workspaces in turn like any other
   *      batches and overlap (a staging buffer is refilled only after the kernels of the slice that read it have finished on
   *      THEIR stream).  Both calls return when every slice's results are in `results`; they use no stream of the caller's. */
  int32_t batches_in_flight;
} ssd_config;

/* the constants of GeometricTransformation (transformation.h:102-126) */
typedef struct
{
  double a[9];    /* camera -> camera-dependent world, row-major rotation */
  double b[3];    /* translation */
  double r2[4];   /* ToExternalWorld 2-D rotation, row-major */
  double t2[2];   /* ToExternalWorld 2-D translation */
  double world_z; /* ToExternalWorld::_worldZ */
} ssd_calibration;

/* Stairs::StairStep (stairs.h:32-36), external world coordinates */
typedef struct
{
  double height;    /* mean z of the plateau's points inside its quadrilateral + world_z (pointcloud.cpp:574-581, transformation.cpp:209-211):
                       summed in 2^-40 m fixed point, order-independent — within 3e-14 m of, not bit-equal to, the reference's running double sum */
  double quad[8];   /* quadrilateral[0..3] as x,y pairs: front-left, front-right, back-left, back-right */
} ssd_step;

typedef struct
{
  int32_t n_steps;   /* Stairs::stairSteps.size() */
  int32_t status;    /* SSD_ST_* bits */
  ssd_step steps[SSD_MAX_STEPS];
} ssd_frame_result;

typedef struct ssd_handle ssd_handle;

/* ---- configuration / calibration (host only, no GPU needed) ------------- */
int ssd_default_config(ssd_config *cfg, int width, int height);
int ssd_calibration_from_points(const double world_points[9], const double camera_points[9], ssd_calibration *out);
int ssd_calibration_identity(ssd_calibration *out);   /* GeometricTransformation() default, transformation.h:51-55 */
/* GeometricCalibration::load() (geometricCalibration.cpp:185-203): reads the two text files the calibration
 * step leaves in the working directory — "calibration-triangle" (calibrationTriangle.cpp:97-125: header line
 * `calibration triangle`, `xN = v, yN = v, zN = v` for N = 1..3, `lowerQuadrant = left|right`) and
 * "calibration-points" (geometricCalibration.cpp:73-98: header line `calibration points`, 10 rows of
 * `x, y, z; x, y, z; x, y, z`) — averages the 10 point sets and builds the transformation.
 * Returns SSD_OK and *loaded = 1; if a file is missing or invalid the reference logs an error and carries on
 * with the identity transformation (:199-202): *loaded = 0, identity in *out, still SSD_OK.
 * world_points / camera_points (9 doubles each, may be NULL) receive what was read. */
int ssd_calibration_load(const char *triangle_path, const char *points_path, ssd_calibration *out, int *loaded,
                         double *world_points, double *camera_points);

/* ---- lifetime ------------------------------------------------------------ */
int ssd_create(const ssd_config *cfg, const ssd_calibration *cal, int device, ssd_handle **out);
int ssd_destroy(ssd_handle *h);
const char *ssd_last_error(void);
size_t ssd_workspace_bytes(const ssd_handle *h);
/* Batches of 64 XGA frames' worth of points and more, given as vertices, run K1 and the raster of the step plateaus as ONE pass over
 * the input ("The single pass"): about 10 % more frames/s for 2.4 MB more per XGA frame and workspace
 * (SSD_MAX_PLANES bit images per frame), the results the same bit for bit.  enable = 0 gives that memory back and keeps the
 * handle on two passes; enable != 0 (the default of a handle whose max_frames_per_batch qualifies) takes it again.  Waits for the
 * handle's batches in flight.  No reference counterpart (a deployment knob).
 * The planes are the last thing ssd_create allocates and the one thing it can do without: when they do not fit - or would cross
 * SSD_MAX_PLANE_BYTES, an environment variable that bounds what a handle may take for the planes of all its workspaces together
 * (a GPU shared with other tenants) - the handle is created on two passes, ssd_create returns SSD_OK and ssd_last_error() says why;
 * ssd_set_single_pass(h, 1) under the same shortage fails with SSD_E_NOMEM and leaves the handle whole, on two passes. */
int ssd_set_single_pass(ssd_handle *h, int enable);

/* ---- processing ------------------------------------------------------------
 * A frame is width*height points, AoS float x,y,z (rs2::vertex layout), row-major, invalid = (0,0,0).
 * ssd_process_host:   frames in host memory, contiguous; fills results[n].  Double-buffered: the batch is cut into slices
 *                     of up to 32 frames, the host-to-device copy of a slice overlaps the kernels of the one before.
 *                     Memory from ssd_host_alloc (pinned) is copied by DMA directly; pageable memory goes through the
 *                     runtime's staging.  PCIe-bound either way (9.4 MB per XGA frame, 1.6 MB as 16-bit depth).
 * ssd_enqueue:        frames already in device memory (frame i at d_xyz + i*frame_stride_bytes); enqueues the
 *                     whole pipeline on `stream` (a hipStream_t, NULL = default stream) and returns without
 *                     synchronising. nframes <= max_frames_per_batch.
 * ssd_fetch:          waits for the last ssd_enqueue (whose last step is the copy of its results into pinned host
 *                     memory) and hands its results over.
 */
int ssd_process_host(ssd_handle *h, const float *xyz, int nframes, ssd_frame_result *results);
int ssd_enqueue(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream);
int ssd_fetch(ssd_handle *h, ssd_frame_result *results, int nframes, void *stream);
/* The results of a batch travel to the host as part of its ssd_enqueue (max(2, batches_in_flight) slots, used in turn), so
 * a caller may keep the GPU busy: ssd_enqueue(batch i+1) first, then ssd_fetch_back(.., back = 1) for batch i — with 3
 * batches in flight: two enqueues ahead, back = 2.  back = 0 is ssd_fetch.  Waits only for that batch.  A slot is reused by
 * the enqueue max(2, batches_in_flight) calls later: fetch before that. */
int ssd_fetch_back(ssd_handle *h, ssd_frame_result *results, int nframes, int back);
/* makes `stream` (a hipStream_t, NULL = default stream) wait for the batch `back` enqueues ago (counted like ssd_fetch_back: the
 * enqueues that produced results; a partial ssd_enqueue_stages run without the last stage is not one), without blocking the host:
 * what a producer that overwrites the batch's frames, or a consumer of device-side state, needs when the handle keeps
 * several batches in flight (with one workspace the caller's stream is already ordered) */
int ssd_stream_wait(ssd_handle *h, int back, void *stream);
/* the number of workspaces the handle was created with (ssd_config::batches_in_flight resolved) */
int ssd_batches_in_flight(const ssd_handle *h);

/* ---- batches overlapped across handles ------------------------------------------------------------------------
 * One handle runs a batch as a chain of dependent launches; its small kernels (one block per frame or image) leave the
 * GPU nearly empty for about 0.1 ms per batch, which matters the more the fewer frames a batch has.  A pipeline owns
 * `depth` handles (each with its own workspace: memory = depth x ssd_workspace_bytes) on `depth` streams of its own and
 * deals the submitted batches out round-robin; results come back in submission order.  At most `depth` batches are
 * unfetched at any time (ssd_pipeline_submit returns SSD_E_CAP otherwise); the frames of a submitted batch must stay
 * untouched until its results were fetched.  XGA, frames/s at depth 1 / 2 / 3 / 4: 64 frames per
 * batch 181 k / 235 k / 248 k / 232 k, 256: 230 k / 272 k / 282 k / 274 k, 1024: 257 k / 284 k / 304 k / 295 k. */
typedef struct ssd_pipeline ssd_pipeline;
int ssd_pipeline_create(const ssd_config *cfg, const ssd_calibration *cal, int device, int depth, ssd_pipeline **out);
int ssd_pipeline_destroy(ssd_pipeline *p);
/* The pipeline's streams are its own (non-blocking): ssd_pipeline_submit expects the frames to be complete in device memory
 * (their producer synchronised); ssd_pipeline_submit_after orders the batch behind the work `producer_stream` holds at the
 * time of the call (use_producer != 0; producer_stream NULL = the default stream). */
int ssd_pipeline_submit(ssd_pipeline *p, const void *d_xyz, size_t frame_stride_bytes, int nframes);
int ssd_pipeline_submit_after(ssd_pipeline *p, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *producer_stream, int use_producer);
/* results of the OLDEST unfetched batch (waits for it); *nframes = its frame count; capacity = length of `results` */
int ssd_pipeline_next(ssd_pipeline *p, ssd_frame_result *results, int capacity, int *nframes);
int ssd_pipeline_pending(const ssd_pipeline *p);        /* batches submitted and not yet fetched */
/* per-stage device times for the pipeline's batches (ssd_set_timing on every handle; events between the launches of a batch do
 * not keep the batches of different handles from overlapping: measured, depth 3 at 1024 frames 302 k frames/s with, 297 k
 * without).  ssd_pipeline_stage_times: the 7 stages (ssd_get_stage_times) of the batch ssd_pipeline_next returned last —
 * valid until that batch's handle is given another one, i.e. call it right after ssd_pipeline_next */
int ssd_pipeline_set_timing(ssd_pipeline *p, int enable);
int ssd_pipeline_stage_times(ssd_pipeline *p, float ms[7]);
const char *ssd_pipeline_last_error(void);

/* ---- 16-bit depth input ---------------------------------------------
 * The step before the path in the reference is rs2::pointcloud::calculate (pointcloud.cpp:138): depth image ->
 * xyz vertices.  librealsense2 2.42.0 (third party, not in the reference tree) computes, in float,
 *     d = raw * depth_units;  x = d * ((u - ppx) / fx);  y = d * ((v - ppy) / fy);  z = d;   raw = 0 -> (0,0,0)
 * (src/proc/pointcloud.cpp pre_compute_x_y_map / get_points, rsutil.h rs2_deproject_pixel_to_point; the L515
 * depth stream has no distortion model).  With intrinsics set, the kernels read the 2-byte depth pixel instead
 * of the 12-byte vertex and deproject on the fly — the same results as deprojecting first, 6x less input. */
typedef struct
{
  float fx, fy, ppx, ppy;       /* rs2_intrinsics of the depth stream */
  float depth_units;            /* metres per raw unit (L515: 0.00025) */
} ssd_intrinsics;

int ssd_set_intrinsics(ssd_handle *h, const ssd_intrinsics *intr);
/* frames of width*height uint16 depth values, row-major; same contracts as ssd_process_host / ssd_enqueue */
int ssd_process_depth_host(ssd_handle *h, const uint16_t *depth, int nframes, ssd_frame_result *results);
int ssd_enqueue_depth(ssd_handle *h, const void *d_depth, size_t frame_stride_bytes, int nframes, void *stream);
/* host restatement of the deprojection (no GPU needed): depth image -> width*height xyz floats */
int ssd_deproject_host(const ssd_intrinsics *intr, int width, int height, const uint16_t *depth, float *xyz);

/* ---- vertical faces -------------------------------------------------------
 * EXTENSION: the reference has no counterpart — it discards the points that belong to no plateau (`remainder`)
 * with a TODO to find the vertical faces in them (pointcloud.cpp:285-294).  Nothing here changes the results above.
 * Between two vertically consecutive emitted surfaces (ground, valid steps; in output order) lies one riser: the
 * vertical rectangle under the FRONT edge of the upper surface, from the lower surface's height to the upper's.
 * Its evidence are the in-range points of no plateau whose height lies strictly between the two surfaces (one
 * height interval away from either), within `tolerance` metres (horizontally) of that front edge's line and
 * between its end points.  DESIGN.md section 7 states the arithmetic; oracle/ holds the same on the CPU. */
#define SSD_MAX_RISERS (SSD_MAX_STEPS - 1)
typedef struct
{
  int32_t n_points;          /* evidence points */
  int32_t detected;          /* n_points >= min_support */
  double height_bottom, height_top;   /* heights of the lower / upper surface (as ssd_step.height) */
  double left[2], right[2];  /* the upper surface's front-left / front-right corner, external world x,y */
  double mean_offset;        /* mean signed horizontal distance of the evidence from the edge line, metres
                                (positive: on the left of the direction front-left -> front-right) */
} ssd_riser;

typedef struct
{
  int32_t n_risers;          /* emitted surfaces - 1, or 0 */
  int32_t reserved;
  ssd_riser risers[SSD_MAX_RISERS];
} ssd_frame_risers;

/* enable != 0: every later ssd_enqueue / ssd_process_* also gathers riser evidence (one more pass over the points
 * of the bins between the surfaces).  tolerance in (0, 1] metres, min_support >= 1. */
int ssd_set_risers(ssd_handle *h, int enable, double tolerance, int min_support);
/* risers of the last enqueue (after ssd_fetch, or instead of it: synchronises `stream`), or of the whole batch of the last
 * ssd_process_host / ssd_process_depth_host call (collected slice by slice); nframes <= what that call processed.  While
 * risers are on, a handle with several workspaces runs its batches one after the other (the riser buffer is single). */
int ssd_fetch_risers(ssd_handle *h, ssd_frame_risers *out, int nframes, void *stream);
/* ---- per-pixel surface labels -----------------------------------------------------------------------------------
 * EXTENSION: which camera pixels each reported surface came from.  Frame i's labels are W * H bytes, one per point (camera
 * pixel (u, v) at v * W + u, for vertex and 16-bit depth input alike):
 *   k + 1  the point is one of those whose mean is surface k of the frame's ssd_frame_result (k_final's order: the ground first
 *          when emitted, then the valid steps ascending), i.e. pointsInQuadri of calcGround / calcStairStep
 *          (pointcloud.cpp:528-558): z > 0, strictly inside the measuring range after CameraToWorld (the reference's doubles),
 *          its height bin among those that feed that surface's plateau (ssd_debug_plateau eff_lo .. eff_hi), and
 *          QuadrilateralTest::isPointWithin of that plateau's quadrilateral;
 *   0      otherwise (SSD_LABEL_NONE).  Every label of a frame is 0 when its status has SSD_ST_THROW or n_steps == 0.
 * So the count of label k + 1 is that surface's n_in_quad (the ground: ground_n_in_quad) and the mean of round(z * 2^40) over its
 * pixels is its height less world_z, bit for bit.  Quirk Q6: a ground whose front edge is not found is reported as the all-zero
 * surface (height world_z, quadrilateral zero); label 1 still marks the points the reference averaged for it (those inside the
 * ground quadrilateral it tested them against: their count and mean are ssd_debug_frame's ground_n_in_quad / ground_mean_z).  An SSD_ST_OVERFLOW frame is labelled as its truncated result reports.
 * The contracts are those of ssd_enqueue / ssd_enqueue_depth / ssd_process_host / ssd_process_depth_host.  Labels of frame i go
 * to d_labels + i * label_stride_bytes (label_stride_bytes >= W * H); bytes past W * H of a stride and frames past nframes are
 * not written.  They are complete when ssd_fetch / ssd_fetch_back of the batch returns (and for a stream made to wait with
 * ssd_stream_wait).  The host variants fill labels[nframes * W * H] (pinned or pageable) and return when all of it is there.
 * A handle that never asks for labels allocates and launches nothing for them. */
#define SSD_LABEL_NONE 0   /* label k + 1 = the point counts toward surface k of the frame's ssd_frame_result */
int ssd_enqueue_labels(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream,
                       uint8_t *d_labels, size_t label_stride_bytes);
int ssd_enqueue_depth_labels(ssd_handle *h, const void *d_depth, size_t frame_stride_bytes, int nframes, void *stream,
                             uint8_t *d_labels, size_t label_stride_bytes);
int ssd_process_host_labels(ssd_handle *h, const float *xyz, int nframes, ssd_frame_result *results, uint8_t *labels);
int ssd_process_depth_host_labels(ssd_handle *h, const uint16_t *depth, int nframes, ssd_frame_result *results, uint8_t *labels);
/* ---- riser labels: the evidence pixels of every vertical face, in the same mask ------------------------------------------
 * EXTENSION.  A surface label needs a height bin among a plateau's effective bins, riser evidence a bin of no
 * plateau: no point can be both, so one byte per pixel still suffices and no label value above moves.
 *   ssd_set_riser_labels  waits for the handle's batches in flight.  While it is on AND risers are on (ssd_set_risers), every call that
 *                         writes labels - ssd_enqueue_labels, ssd_enqueue_depth_labels, ssd_enqueue_cameras with d_labels,
 *                         ssd_process_host_labels, ssd_process_depth_host_labels, ssd_process_host_cameras with labels - writes,
 *                         beside the surface labels, SSD_LABEL_RISER_BASE + i into the byte of every evidence point of riser i of the
 *                         frame's ssd_frame_risers: exactly the points ssd_riser.n_points counts (above), of risers with
 *                         detected == 0 too.  So the count of label SSD_LABEL_RISER_BASE + i in a frame is risers[i].n_points, and
 *                         with riser moments also on, ssd_surface_moments_host over the riser half of ssd_labels_split is the frame's
 *                         ssd_fetch_riser_moments record, byte for byte.  It may be set while risers are off and takes effect when they
 *                         come on.  While it is off, or risers are off, or a call writes no labels, nothing more is launched and every
 *                         byte is what it is without this section; results, risers, riser moments, debug records and the surface
 *                         labels never change.  A frame whose status has SSD_ST_THROW or with fewer than two emitted surfaces carries
 *                         no riser label; an SSD_ST_OVERFLOW frame is labelled as its truncated riser record reports.  Bytes past W * H
 *                         of a stride and frames past nframes are not written.  Not part of ssd_enqueue_stages or ssd_pipeline_*.  No
 *                         buffer is allocated: a pair of events per timing slot, on the first enable.
 *   ssd_labels_split      host only, no GPU needed: surfaces[k] = labels[k] where labels[k] <= SSD_MAX_STEPS, else 0; risers[k] =
 *                         labels[k] - SSD_LABEL_RISER_BASE + 1 where the label lies in SSD_LABEL_RISER_BASE .. SSD_LABEL_RISER_BASE +
 *                         SSD_MAX_RISERS - 1, else 0 - each in the form ssd_surface_moments_host and ssd_surface_refit_moments_host
 *                         accept (n_surfaces = the frame's n_steps and n_risers).  Either output may be NULL, either may be `labels`
 *                         itself.  SSD_E_ARG, before anything is written: a label in neither range, null labels with n > 0.
 * Camera batches: frame i's label bytes are byte for byte those of a handle made by ssd_create(cfg, &cams[camera_of_frame[i]].cal)
 * (with its intrinsics for depth input) for that frame alone. */
#define SSD_LABEL_RISER_BASE 32   /* label SSD_LABEL_RISER_BASE + i = the point is evidence of riser i of the frame's ssd_frame_risers */
int ssd_set_riser_labels(ssd_handle *h, int enable);
int ssd_labels_split(const uint8_t *labels, size_t n, uint8_t *surfaces /* may be NULL */, uint8_t *risers /* may be NULL */);

/* ---- per-frame calibration: batches of frames from many cameras ------------------------------------------------------
 * EXTENSION.  A handle may hold a table of cameras beside the calibration ssd_create gave it; a cameras
 * batch names, frame by frame, the camera each frame comes from.  The cameras share the handle's ssd_config (resolution,
 * measuring range, intervals); what a mounting and a sensor decide varies: CameraToWorld, ToExternalWorld, world_z and, for
 * 16-bit depth input, the intrinsics.
 *   ssd_set_cameras     waits for the handle's batches in flight and replaces the table (ncams = 0 frees it).  Each camera's
 *                       constants are derived exactly as ssd_create / ssd_set_intrinsics derive a handle's.
 *   ssd_enqueue_cameras as ssd_enqueue (input = SSD_INPUT_VERTICES) or ssd_enqueue_depth (SSD_INPUT_DEPTH16), with labels when
 *                       d_labels is not NULL; camera_of_frame (HOST memory, nframes entries) is copied during the call.
 *   ssd_process_host_cameras   as ssd_process_host / ssd_process_depth_host (and their _labels forms).
 * Contract: frame i's result, labels, risers and debug record are byte for byte those a handle made by
 * ssd_create(cfg, &cams[camera_of_frame[i]].cal) (with ssd_set_intrinsics(&...intr) for depth input) returns for that frame alone.
 * Fetching (ssd_fetch, ssd_fetch_back, ssd_stream_wait, ssd_fetch_risers, ssd_get_debug*, the timing getters) is that of any
 * other batch.  SSD_E_ARG, before anything is launched or copied: no table, an index >= ssd_camera_count, depth input naming a
 * camera without intrinsics, ncams outside 0 .. SSD_MAX_CAMERAS, a null handle.  ssd_enqueue, ssd_process_host and the rest keep
 * using ssd_create's calibration whatever the table holds; ssd_enqueue_stages and ssd_pipeline_* take no cameras.  A handle that
 * never sets cameras allocates and launches nothing for them. */
#define SSD_MAX_CAMERAS 4096
#define SSD_INPUT_VERTICES 0
#define SSD_INPUT_DEPTH16 1
typedef struct
{
  ssd_calibration cal;
  ssd_intrinsics intr;          /* read when has_intrinsics != 0 */
  int32_t has_intrinsics;
  int32_t reserved;
} ssd_camera;
int ssd_set_cameras(ssd_handle *h, const ssd_camera *cams, int ncams);
int ssd_camera_count(const ssd_handle *h);
int ssd_enqueue_cameras(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                        const uint16_t *camera_of_frame, int input, uint8_t *d_labels, size_t label_stride_bytes);
int ssd_process_host_cameras(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                             ssd_frame_result *results, uint8_t *labels);

/* ---- ground fit: a camera's calibration refined from the floor in its own frames ------------------------------------
 * EXTENSION.  CameraToWorld (a, b) is fully determined by the floor's plane in camera coordinates
 * (ssd_calibration_from_points: z = -n0, y = normalize(0, -z.z / z.y, 1), x = y x z, b = (0, 0, n0 . p0)); only ToExternalWorld
 * (r2, t2, world_z) needs surveyed marks.  Given frames and a rough prior calibration per frame, one streaming pass on the GPU
 * gathers each frame's floor points into exact integer moments, and a small host solve turns the moments into a plane and a
 * refined calibration (r2, t2, world_z carried over from the prior: the fit follows pitch, roll and height, not yaw or the
 * translation over the floor).
 * Floor points of a frame: a point (x, y, z) in float camera coordinates (16-bit depth input is deprojected first, bit-equal to
 * ssd_deproject_host) is a floor point iff
 *   z > 0;
 *   w = A p + b lies strictly inside the handle's x and y measuring range, w in doubles as K1 computes it: each row
 *     (a0 x + a1 y) + a2 z, then + b, no FMA;
 *   -tol <= w.z && w.z <= tol;
 *   each of qx, qy, qz has |q| < 2^20, q = llrint(double(v) * 65536.0): 2^-16 m fixed point, |v| < 16 m.
 * A frame has fewer than 2^23 points and each product is below 2^40, so every sum stays below 2^63: the moments are exact
 * integers, independent of the order of summation, and the device and ssd_ground_moments_host agree bit for bit. */
#define SSD_GF_OK 0
#define SSD_GF_FEW 1          /* fewer than min_points floor points */
#define SSD_GF_DEGENERATE 2   /* points do not determine a plane, or the plane gives no calibration */
#define SSD_GF_PLANARITY 16.0 /* DEGENERATE unless lambda_mid >= SSD_GF_PLANARITY * lambda_min */

typedef struct
{
  int64_t n;          /* floor points */
  int64_t s[3];       /* sum qx, qy, qz */
  int64_t ss[6];      /* sum qx*qx, qx*qy, qx*qz, qy*qy, qy*qz, qz*qz */
} ssd_ground_moments;

typedef struct
{
  ssd_ground_moments m;
  int32_t status, reserved;
  double normal[3];   /* n0: unit, away from the camera (n0 . centroid > 0), camera coordinates */
  double dist;        /* n0 . centroid = camera height above the fitted floor */
  double rms;         /* sqrt(lambda_min): rms distance of the floor points from the plane, metres */
  double tilt;        /* angle between n0 and the prior's (-a[6], -a[7], -a[8]), radians */
  double height_delta;/* dist - prior b[2] */
  ssd_calibration cal;/* a, b from (n0, dist) exactly as ssd_calibration_from_points derives them from n0 and dot(c0, n0);
                         r2, t2, world_z copied from the prior.  status != OK: the prior, unchanged */
} ssd_ground_fit;

/* host only: the a / b half of ssd_calibration_from_points (the same code, shared), r2 / t2 / world_z copied from `prior`;
 * SSD_E_ARG in the degenerate cases ssd_calibration_from_points rejects (dist <= 0, a plane that holds the camera's y axis) */
int ssd_calibration_from_plane(const double n0[3], double dist, const ssd_calibration *prior, ssd_calibration *out);
/* host restatement of the floor-point rule for ONE frame (no GPU needed): input = SSD_INPUT_VERTICES (width * height xyz floats)
 * or SSD_INPUT_DEPTH16 (width * height uint16, prior->has_intrinsics required); tol in (0, 1] */
int ssd_ground_moments_host(const ssd_config *cfg, const ssd_camera *prior, int input, const void *frame, double tol, ssd_ground_moments *out);
/* host only: moments -> plane -> calibration.  The centred scatter N SS - S (x) S is formed exactly in 128-bit integers, converted
 * once to double and scaled to m^2; its eigenvalues lambda_min <= lambda_mid <= lambda_max by cyclic Jacobi; n0 = the eigenvector
 * of lambda_min, signed so that n0 . centroid > 0.  Status in this order: FEW (n < max(min_points, 1)), DEGENERATE (lambda_mid <= 0,
 * or lambda_mid < SSD_GF_PLANARITY * lambda_min, or ssd_calibration_from_plane fails; an eigenvalue not above 64 eps lambda_max
 * counts as 0: the rounding level of the solve), OK.  Unless OK: cal = the prior, the other doubles 0.  Always returns SSD_OK for
 * non-null arguments. */
int ssd_ground_fit_solve(const ssd_ground_moments *m, const ssd_calibration *prior, int min_points, ssd_ground_fit *out);
/* The moments of frames resident in device memory (frame i at d_frames + i * frame_stride_bytes), on the caller's stream, in order,
 * without synchronising - the stream contract of ssd_enqueue with one workspace, whatever batches_in_flight is.  npriors = 0: the
 * handle's calibration (and its ssd_set_intrinsics for depth input); 1: priors[0] for every frame; nframes: one per frame.  Priors
 * are HOST memory, copied during the call.  Uses none of the detection workspaces, neither disturbs nor waits for batches in flight
 * and leaves the state ssd_fetch* read untouched.  SSD_E_ARG before anything is launched: npriors not 0, 1 or nframes, depth input
 * without intrinsics, nframes outside 1 .. max_frames_per_batch, tol outside (0, 1], a null handle.  Its buffers (80 bytes per
 * frame of max_frames_per_batch on the device and pinned, and the priors) are made on the first call and counted in
 * ssd_workspace_bytes from then on; a handle that never fits allocates, creates and launches nothing for it. */
int ssd_enqueue_ground_fit(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                           const ssd_camera *priors, int npriors, double tol);
/* waits for the last ssd_enqueue_ground_fit and runs ssd_ground_fit_solve per frame against that frame's prior; nframes <= its */
int ssd_fetch_ground_fit(ssd_handle *h, ssd_ground_fit *out, int nframes, int min_points, void *stream);
/* frames in host memory (pinned or pageable), any nframes >= 1: in slices through the staging buffers of ssd_process_host, the copy
 * of a slice overlapping the kernel of the one before; returns when out[nframes] is filled */
int ssd_process_host_ground_fit(ssd_handle *h, const void *frames, int nframes, int input, const ssd_camera *priors, int npriors,
                                double tol, int min_points, ssd_ground_fit *out);

/* ---- surface fit: plane, tilt and flatness of every reported surface ----------------------------------------------------
 * EXTENSION.  The per-pixel labels say which points carry each reported surface; the ground fit turns points
 * into exact integer moments and a plane.  Joined: one more pass behind k_final gathers, per frame, the moments of every surface of
 * its ssd_frame_result - about 1.5 KB per frame instead of a byte per point - and a small host solve turns them into a plane each.
 * The moments of surface k of a frame are the ten sums of ssd_ground_moments over exactly the points whose label (above) would be
 * k + 1: q = llrint(double(v) * 65536.0) on the float camera coordinates (16-bit depth input is deprojected first, bit-equal to
 * ssd_deproject_host); a labelled point with some |q| >= 2^20 (|v| >= 16 m) is left out of the sums and counted in n_far.  The
 * overflow argument is the ground fit's: all sums are exact integers, independent of the order of summation, and the device and
 * ssd_surface_moments_host agree bit for bit.  So m.n + n_far of surface k is its n_in_quad (the ground: ground_n_in_quad).
 * Surface order is k_final's, as for labels; records at k >= n_surfaces are zero; a frame with SSD_ST_THROW or n_steps == 0 is all
 * zero.  Surface 0's m of a frame with ground = 1 goes straight into ssd_ground_fit_solve: the detector's own ground points lie
 * inside the ground quadrilateral, in front of the first riser, so a calibration can be polished or watched for drift in the same
 * call that detects.
 * Camera batches have their own entry points (ssd_enqueue_cameras_surface_moments, ssd_process_host_cameras_surfaces, below): each
 * frame's moments under its own camera, and ssd_camera_drift_fold on top of them. */
typedef struct
{
  ssd_ground_moments m;
  int64_t n_far;      /* labelled points left out of m: some |q| >= 2^20 */
} ssd_surface_moments;

typedef struct
{
  int32_t n_surfaces; /* the frame's n_steps */
  int32_t ground;     /* 1: surface 0 is the ground (quirk Q6 included: the ground reported as the all-zero surface) */
  ssd_surface_moments s[SSD_MAX_STEPS];
} ssd_frame_moments;

typedef struct
{
  int32_t status, reserved;   /* SSD_GF_OK / SSD_GF_FEW / SSD_GF_DEGENERATE */
  int64_t n, n_far;
  double normal[3];   /* unit, pointing up, external world coordinates (as ssd_step's corners) */
  double centroid[3]; /* mean of the surface's points, external world: x, y as ssd_step's corners, z + world_z as ssd_step.height */
  double tilt;        /* angle between normal and the vertical, radians */
  double rms;         /* sqrt(lambda_min): rms distance of the points from the plane, metres */
  double extent[2];   /* sqrt(lambda_max), sqrt(lambda_mid): rms half-extents of the points within the plane, metres */
} ssd_surface_fit;

typedef struct
{
  int32_t n_surfaces, ground;
  ssd_surface_fit s[SSD_MAX_STEPS];
} ssd_frame_surfaces;

/* ssd_enqueue / ssd_enqueue_depth plus the frames' surface moments: frame i's record at d_out + i (device memory, nframes contiguous
 * records).  The contracts are those of ssd_enqueue_labels: the pass runs behind k_final and in front of the batch's completion
 * event, so the records are complete when ssd_fetch / ssd_fetch_back of the batch returns, and for a stream made to wait with
 * ssd_stream_wait; with several workspaces the batches take them in turn like any others.  The records are zeroed on the batch's
 * stream in front of the pass.  A null destination: SSD_E_ARG.  A handle that never asks for surface moments allocates and launches
 * nothing for them. */
int ssd_enqueue_surface_moments(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream, ssd_frame_moments *d_out);
int ssd_enqueue_depth_surface_moments(ssd_handle *h, const void *d_depth, size_t frame_stride_bytes, int nframes, void *stream, ssd_frame_moments *d_out);
/* the pass's device time for the same enqueue (0 when that enqueue gathered no surface moments); as ssd_get_labels_time_back */
int ssd_get_surface_moments_time_back(ssd_handle *h, int back, float *ms);
/* host only, no GPU needed: one frame's sums from a label array (width * height bytes, as the label entry points write them; a label
 * above n_surfaces: SSD_E_ARG).  input = SSD_INPUT_VERTICES (width * height xyz floats) or SSD_INPUT_DEPTH16 (width * height uint16,
 * intr required, else ignored).  n_surfaces (0 .. SSD_MAX_STEPS) and ground go into the record's header as given. */
int ssd_surface_moments_host(const ssd_config *cfg, int input, const ssd_intrinsics *intr, const void *frame, const uint8_t *labels,
                             int n_surfaces, int ground, ssd_frame_moments *out);
/* host only: a frame's moments -> a plane per surface, by the solve of ssd_ground_fit_solve (the same code, shared: exact centred
 * scatter, cyclic Jacobi, n0 = the eigenvector of lambda_min signed away from the camera).  Status per surface in this order: FEW
 * (n < max(min_points, 1)), DEGENERATE (lambda_mid <= 0 or lambda_mid < SSD_GF_PLANARITY * lambda_min, eigenvalues at the rounding
 * level counting as 0), OK.  normal = -(A n0), its x and y through r2; centroid through CameraToWorld and ToExternalWorld; tilt,
 * rms, extent as above.  Unless OK the doubles are 0; n and n_far are always the moments'.  Records at k >= n_surfaces are zero. */
int ssd_surface_fit_solve(const ssd_frame_moments *moments, const ssd_calibration *cal, int min_points, ssd_frame_surfaces *out);
/* frames in host memory (input = SSD_INPUT_VERTICES: as ssd_process_host; SSD_INPUT_DEPTH16: as ssd_process_depth_host), through the
 * same slices: fills results[nframes], out[nframes] (each frame's moments solved against the handle's calibration) and, when not
 * NULL, moments[nframes]; returns when all of it is there. */
int ssd_process_host_surfaces(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                              ssd_frame_moments *moments, int min_points, ssd_frame_surfaces *out);

/* ---- surface fit of cameras batches, and drift per camera ---------------------------------------------------------------
 * EXTENSION: the contract of per-frame calibration, extended to the surface fit.
 *   ssd_enqueue_cameras_surface_moments  as ssd_enqueue_cameras (no labels) plus the frames' surface moments at d_out + i.
 *   ssd_process_host_cameras_surfaces    as ssd_process_host_surfaces, through the slices of ssd_process_host_cameras.
 * Contract: frame i's ssd_frame_moments is byte for byte what a handle made by ssd_create(cfg, &cams[camera_of_frame[i]].cal) (with
 * ssd_set_intrinsics(&...intr) for depth input) returns for that frame alone, and out[i] is
 * ssd_surface_fit_solve(moments + i, &cams[camera_of_frame[i]].cal, min_points, ..).  Stream, completion, zeroing, several
 * workspaces and ssd_get_surface_moments_time_back are those of ssd_enqueue_surface_moments; camera_of_frame (HOST memory) is copied
 * during the call.  SSD_E_ARG, before anything is launched or copied: what ssd_enqueue_cameras refuses, and a null destination.  A
 * handle that never asks allocates and launches nothing more. */
int ssd_enqueue_cameras_surface_moments(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                                        const uint16_t *camera_of_frame, int input, ssd_frame_moments *d_out);
int ssd_process_host_cameras_surfaces(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                      ssd_frame_result *results, ssd_frame_moments *moments, int min_points, ssd_frame_surfaces *out);

/* Drift per camera: the ground moments (surface 0 of a frame with ground = 1) of all of a camera's frames in a batch, added exactly,
 * and one ssd_ground_fit_solve per camera against its table entry: fit.tilt and fit.height_delta say how far the mounting has moved
 * from what the table holds, fit.cal is the refined entry.  Frames are folded in index order; a frame is added whole or not at all:
 * when any of its ten sums or n_far would carry an int64 sum past its range the frame is counted in frames_left and skipped (a later,
 * smaller frame may still fit).  The sums are exact integers, so the record does not depend on the order of the folded frames unless
 * the order changes which frames fit. */
typedef struct
{
  int32_t camera, frames;        /* table index; frames of the batch that name it */
  int32_t frames_ground;         /* ... of those, folded: ground == 1 and n_surfaces >= 1 */
  int32_t frames_left;           /* ... with a ground, NOT folded: adding them would overflow an int64 sum */
  ssd_ground_moments m;          /* exact sum of s[0].m over the folded frames */
  int64_t n_far;
  ssd_ground_fit fit;            /* ssd_ground_fit_solve(&m, &cams[camera].cal, min_points, ..): tilt, height_delta, rms, refined cal */
} ssd_camera_drift;

/* host only, no GPU needed: out[ncams], one record per camera of the table (a camera no frame names: frames = 0, fit.status =
 * SSD_GF_FEW).  SSD_E_ARG: a null pointer, ncams outside 1 .. SSD_MAX_CAMERAS, nframes < 0, an index >= ncams (out is then untouched). */
int ssd_camera_drift_fold(const ssd_frame_moments *moments, const uint16_t *camera_of_frame, int nframes,
                          const ssd_camera *cams, int ncams, int min_points, ssd_camera_drift *out /* ncams records */);

/* ---- riser fit: plane, lean and going of every vertical face ------------------------------------------------------------------
 * EXTENSION: what the surface fit does for the treads, for the risers between them.  While the riser moments
 * are on, the riser pass (ssd_set_risers) gathers in the SAME walk, beside the count and the mean offset of every riser, the exact
 * integer moments of its evidence points, and a small host solve turns them into a plane per riser: is the face vertical (lean), is it
 * parallel to the front edge the detector drew (skew), and how far is it from the next face (going: the tread depth a stair-climbing
 * consumer needs beside the rise).
 * Evidence point of riser i: exactly the points ssd_riser.n_points counts (above).  The riser moments of a frame are an
 * ssd_frame_moments: n_surfaces = the frame's n_risers, ground = 0, s[i] = riser i, records at i >= n_risers zero.  s[i].m holds the
 * ten sums of ssd_ground_moments over riser i's evidence points, q = llrint(double(v) * 65536.0) on the float camera coordinates
 * (16-bit depth input is deprojected first, bit-equal to ssd_deproject_host); an evidence point with some |q| >= 2^20 is left out of
 * the sums and counted in s[i].n_far, so s[i].m.n + s[i].n_far == risers[i].n_points.  The overflow argument is the ground fit's: all
 * sums are exact integers, independent of the order of summation; the device and ssd_surface_moments_host over the riser labels of a
 * host restatement agree bit for bit (the device's own riser labels, ssd_set_riser_labels and ssd_labels_split above, are such labels).
 *   ssd_set_riser_moments    waits for the handle's batches in flight.  While it is on AND risers are on, every riser pass of a whole
 *                            run (ssd_enqueue*, ssd_process_*, the cameras entry points) also gathers the moments; it may be set while
 *                            risers are off and takes effect when they come on.  Results, risers and debug records do not change.
 *                            Its device and pinned buffers (one ssd_frame_moments per frame of max_frames_per_batch each) are made on
 *                            the first enable and counted in ssd_workspace_bytes from then on; a handle that never enables it
 *                            allocates and launches nothing more.  Not part of ssd_enqueue_stages or ssd_pipeline_*.
 *   ssd_fetch_riser_moments  the contract of ssd_fetch_risers: the last enqueue, or the whole batch of the last host call (collected
 *                            slice by slice).  SSD_E_ARG when the last pass gathered none or nframes exceeds what it processed.
 * Camera batches: frame i's riser moments are byte for byte those of a handle made by ssd_create(cfg, &cams[camera_of_frame[i]].cal)
 * (with its intrinsics for depth input) for that frame alone. */
typedef struct
{
  int32_t status, reserved;   /* SSD_GF_OK / SSD_GF_FEW / SSD_GF_DEGENERATE */
  int64_t n, n_far;           /* as in the moments */
  double normal[3];   /* unit, external world coordinates, out of the face toward the camera: -(A n0), x and y through r2 */
  double centroid[3]; /* mean of the evidence points, external world (as ssd_surface_fit.centroid) */
  double lean;        /* asin(normal z), signed: the angle of the face from the vertical, positive when the face looks upward */
  double skew;        /* asin(|h . u|) in [0, pi/2], h = the unit horizontal projection of normal, u = the unit direction left -> right of
                         the riser's ssd_riser: the angle between the fitted face and the front edge the detector drew */
  double rms;         /* sqrt(lambda_min): rms distance of the points from the plane, metres */
  double extent[2];   /* sqrt(lambda_max), sqrt(lambda_mid): rms half-extents of the points within the plane, metres */
  double rise;        /* height_top - height_bottom of the ssd_riser (whatever the status) */
  double going;       /* this riser and the next both OK: |(centroid[i + 1] - centroid[i]) . h_i|, the horizontal distance from this
                         face to the next = the depth of the tread between them; otherwise 0 */
} ssd_riser_fit;

typedef struct
{
  int32_t n_risers, reserved;
  ssd_riser_fit r[SSD_MAX_RISERS];
} ssd_frame_riser_fits;

int ssd_set_riser_moments(ssd_handle *h, int enable);
int ssd_fetch_riser_moments(ssd_handle *h, ssd_frame_moments *out, int nframes, void *stream);
/* host only, no GPU needed: a frame's riser moments and riser records -> a plane per riser, by the solve of ssd_ground_fit_solve (the
 * same code, shared).  Status per riser in this order: FEW (n < max(min_points, 1)), DEGENERATE (the shared SSD_GF_PLANARITY rule), OK.
 * Unless OK the doubles other than rise are 0; n and n_far are always the moments'.  A horizontal normal or a drawn edge of length 0
 * gives skew 0.  Records at i >= n_risers are zero.  SSD_E_ARG: a null pointer, n_surfaces outside 0 .. SSD_MAX_RISERS or not the
 * risers' n_risers. */
int ssd_riser_fit_solve(const ssd_frame_moments *moments, const ssd_frame_risers *risers, const ssd_calibration *cal, int min_points,
                        ssd_frame_riser_fits *out);
/* frames in host memory through the slices of ssd_process_host / ssd_process_depth_host (input as ssd_process_host_surfaces) resp.
 * ssd_process_host_cameras: fills results[nframes], risers[nframes], out[nframes] (out[i] = ssd_riser_fit_solve under the frame's own
 * calibration) and, when not NULL, moments[nframes].  Risers must be on (ssd_set_risers), else SSD_E_ARG before anything is copied; the
 * riser moments are switched on for the call and the previous setting is restored. */
int ssd_process_host_riser_fits(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                                ssd_frame_risers *risers, ssd_frame_moments *moments /* may be NULL */, int min_points,
                                ssd_frame_riser_fits *out);
int ssd_process_host_cameras_riser_fits(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                        ssd_frame_result *results, ssd_frame_risers *risers, ssd_frame_moments *moments /* may be NULL */,
                                        int min_points, ssd_frame_riser_fits *out);

/* ---- trimmed surface refit: the moments of the points near each fitted plane ------------------------------------------------------
 * EXTENSION.  A surface's points are a band of height bins inside its quadrilateral; where the band reaches a
 * riser's foot or a tread's rim those points tilt the fitted plane: the surface fit's error is bias, not noise.  The remedy is a
 * trimmed refit: the moments gathered again over the SAME labelled points, keeping only those within a gate of the plane the fit
 * before found.  A gate is a plane in float camera coordinates and a half-width; a frame has one per surface.
 * Refit moments of surface k of a frame: the ten sums of ssd_ground_moments and n_far, by the fixed-point rule of the surface fit
 * exactly as it stands, over the points that would carry label k + 1 AND satisfy
 *     fabs(((n[0] * x + n[1] * y) + n[2] * z) - dist) <= gate
 * with x, y, z the point's float camera coordinates widened to double, the products and sums in that order, no FMA.  A surface whose
 * gate is not a finite number above 0, or at k >= the gates' n_surfaces, gathers nothing (a NaN in its plane: likewise, no point
 * passes).  n_far counts the labelled points INSIDE the gate that the fixed-point rule leaves out; a point trimmed by the gate is
 * counted nowhere, so m.n + n_far is the points kept.  The record's header (n_surfaces, ground) is the first pass's; records at
 * k >= n_surfaces are zero; a frame with SSD_ST_THROW or n_steps == 0 is all zero.  All sums are exact integers: the device and
 * ssd_surface_refit_moments_host agree bit for bit, and a refit record goes wherever a first-pass record goes - ssd_surface_fit_solve,
 * ssd_ground_fit_solve on surface 0, ssd_camera_drift_fold - unchanged.
 * Camera batches have their own entry points (ssd_enqueue_cameras_surface_refit, ssd_process_host_cameras_surfaces_refit, below).
 * The gates can also be made on the device (ssd_enqueue_surface_refit_device, DESIGN.md section 7i, below).
 * Out of scope: the riser fit, ssd_pipeline_*, and a gate that reaches points outside the labelled set (the
 * bias of a band cut askew by a wrong calibration is only partly answered). */
typedef struct
{
  double n[3];        /* the plane's normal, camera coordinates (unit when made by ssd_surface_gates_from_moments) */
  double dist;        /* n . p of the plane's points */
  double gate;        /* half-width: a point is kept iff |n . p - dist| <= gate; not a finite number above 0: nothing is kept */
} ssd_plane_gate;     /* camera coordinates */

typedef struct
{
  int32_t n_surfaces, reserved;
  ssd_plane_gate g[SSD_MAX_STEPS];
} ssd_frame_gates;

/* host only, no GPU needed: a frame's moments -> a gate per surface, through the solve the fits share (plane_of_moments): n = n0
 * (unit, away from the camera), dist = n0 . centroid, gate = max(k_sigma * rms, gate_min), rms = sqrt(lambda_min).  A surface whose
 * status is not SSD_GF_OK (FEW by min_points, DEGENERATE) gets an all-zero gate and so gathers nothing; gates at k >= n_surfaces are
 * zero.  A perfectly flat surface (rms 0) with gate_min 0 also gets gate 0: give a gate_min of a few fixed-point steps (2^-16 m) to keep
 * it.  SSD_E_ARG: a null pointer, n_surfaces outside 0 .. SSD_MAX_STEPS, k_sigma not in (0, 16], gate_min not in [0, 1]. */
int ssd_surface_gates_from_moments(const ssd_frame_moments *m, int min_points, double k_sigma, double gate_min, ssd_frame_gates *out);
/* host only, no GPU needed: ssd_surface_moments_host with the gate (one walk, shared: the arguments, the deprojection and the
 * fixed-point rule are that function's); gates: one frame's, SSD_E_ARG when null */
int ssd_surface_refit_moments_host(const ssd_config *cfg, int input, const ssd_intrinsics *intr, const void *frame, const uint8_t *labels,
                                   const ssd_frame_gates *gates, int n_surfaces, int ground, ssd_frame_moments *out);
/* The refit pass alone (k_surface_refit), against the workspace of the handle's last WHOLE enqueue - whichever of ssd_enqueue,
 * ssd_enqueue_depth or their _surface_moments / _labels forms ran last - behind it on that batch's stream and in front of a completion
 * event of its own: frame i's record at d_out + i (device memory, nframes contiguous records), zeroed on the stream in front of the
 * pass.  d_frames, frame_stride_bytes, nframes and input (SSD_INPUT_VERTICES / SSD_INPUT_DEPTH16) must be that enqueue's, and the
 * frames must still be untouched: the pass reads the cell records and quadrilaterals the enqueue left and the points again.  gates:
 * HOST memory, nframes records, copied during the call.  It may be repeated (each pass gated by the planes of the one before) until
 * the next enqueue takes the workspace; a later enqueue on any stream is ordered behind it.  It leaves results, result slots, risers
 * and debug records, and everything ssd_fetch* reads, untouched.  The device gates are one set per handle: refit passes run in the
 * order of their calls, each behind the one before, also where they follow batches of different workspaces (enqueue A, refit A,
 * enqueue B, refit B without a fetch between is fine; refit B starts when refit A has ended).  ssd_set_intrinsics between an enqueue
 * and its refit withdraws the enqueue (the pass would deproject with other maps): the refit is then refused.
 * SSD_E_ARG, before anything is launched or copied: no such enqueue (none yet, or the last one was a partial ssd_enqueue_stages run or
 * a cameras batch: ssd_enqueue_cameras_surface_refit refits those), other frames, stride, nframes or input than it had, a null pointer,
 * depth input without intrinsics.
 * The pinned and device gate buffers (one ssd_frame_gates per frame of max_frames_per_batch each) are made on the first call and
 * counted in ssd_workspace_bytes from then on; a handle that never refits allocates and launches nothing more. */
int ssd_enqueue_surface_refit(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                              int input, const ssd_frame_gates *gates /* HOST, nframes, copied during the call */,
                              ssd_frame_moments *d_out);
/* waits for the last ssd_enqueue_surface_refit (SSD_E_ARG: there was none) and, as passes run in the order of their calls, for every
 * one before it: the records of all refit calls so far are complete when it returns */
int ssd_fetch_surface_refit(ssd_handle *h, void *stream);
/* the device time of the last refit pass, the memset in front of it included (0 when timing was off for it); enable timing before */
int ssd_get_surface_refit_time(ssd_handle *h, float *ms);
/* frames in host memory (input as ssd_process_host_surfaces), in the slices of ssd_process_host.  Per slice, while it is still in
 * its staging buffer: detection and the first moments, fetch, gates on the host (ssd_surface_gates_from_moments with min_points,
 * k_sigma, gate_min), the refit pass, fetch - the last three `passes` times (1 .. 4), each pass gated by the planes of the one
 * before.  So a slice is FINISHED before the next one's kernels go out (only its copy overlaps the slice before): the gates need the
 * host between the passes.  Fills results[nframes] (byte for byte ssd_process_host's), out[nframes] (ssd_surface_fit_solve of the last
 * pass against the handle's calibration) and, when not NULL, first[nframes] (the first pass's records) and refit[nframes] (the last
 * pass's).  SSD_E_ARG before anything is copied: a null pointer, passes outside 1 .. 4, what ssd_surface_gates_from_moments refuses. */
int ssd_process_host_surfaces_refit(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                                    ssd_frame_moments *first /* may be NULL */, ssd_frame_moments *refit /* may be NULL */,
                                    int min_points, double k_sigma, double gate_min, int passes /* 1..4 */, ssd_frame_surfaces *out);

/* ---- trimmed refit of cameras batches, and the drift watch on refit records ------------------------------------------------------
 * EXTENSION: the contract of per-frame calibration, extended to the trimmed refit, so that the records
 * ssd_camera_drift_fold folds can be refit records.
 *   ssd_enqueue_cameras_surface_refit        ssd_enqueue_surface_refit where the handle's last whole enqueue was a cameras batch -
 *                                            ssd_enqueue_cameras with or without labels, or ssd_enqueue_cameras_surface_moments.
 *   ssd_process_host_cameras_surfaces_refit  ssd_process_host_surfaces_refit through the slices of ssd_process_host_cameras.
 *   ssd_camera_ground_gates                  host only: every frame's ground gate from its CAMERA's folded floor plane.
 * Contract: frame i's record is byte for byte what a handle made by ssd_create(cfg, &cams[camera_of_frame[i]].cal) (with
 * ssd_set_intrinsics(&...intr) for depth input) gives from ssd_enqueue_surface_refit for that frame alone under gates[i]; hence it is
 * bit for bit ssd_surface_refit_moments_host over that frame's labels.  The gates go by FRAME (gates[i], HOST memory, copied during the
 * call), never by camera: two frames of one camera may carry different gates.  The pass takes no camera index of its own: it reads the
 * index the enqueue left in its workspace's device array, and the handle's table.  Everything else is ssd_enqueue_surface_refit's and is
 * shared with it: the stream and the completion event of its own, ssd_fetch_surface_refit and ssd_get_surface_refit_time, the zeroing in
 * front of the pass, the one set of device gates per handle (passes of either kind run in the order of their calls, across workspaces),
 * the gate buffers made on the first call of either kind and counted in ssd_workspace_bytes, and that nothing ssd_fetch* reads is
 * touched.  ssd_set_cameras between a cameras enqueue and its refit withdraws the enqueue (the table, the index arrays and the maps
 * would be other ones): the refit is then refused.
 * SSD_E_ARG, before anything is launched or copied: the last enqueue was not a whole cameras batch (none yet, a partial run, a withdrawn
 * one - or a whole one-calibration enqueue, which the message names as such), other frames, stride, nframes or input than that enqueue
 * had, a null pointer. */
int ssd_enqueue_cameras_surface_refit(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                                      int input, const ssd_frame_gates *gates /* HOST, nframes, copied during the call */,
                                      ssd_frame_moments *d_out);
/* Per slice, while it is still in its staging buffer: a cameras enqueue with the first moments, fetch, gates on the host per frame
 * (ssd_surface_gates_from_moments), the refit pass, fetch - the last three `passes` times.  Fills results[nframes] (byte for byte
 * ssd_process_host_cameras'), out[nframes] (out[i] = ssd_surface_fit_solve of the last pass's record i against
 * cams[camera_of_frame[i]].cal) and, when not NULL, first[nframes] (ssd_process_host_cameras_surfaces' records) and refit[nframes] (the
 * last pass's: what ssd_camera_drift_fold takes).  SSD_E_ARG before anything is copied: what ssd_process_host_cameras_surfaces and
 * ssd_process_host_surfaces_refit refuse. */
int ssd_process_host_cameras_surfaces_refit(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                            ssd_frame_result *results, ssd_frame_moments *first /* may be NULL */,
                                            ssd_frame_moments *refit /* may be NULL */, int min_points, double k_sigma, double gate_min,
                                            int passes /* 1..4 */, ssd_frame_surfaces *out);
/* host only, no GPU needed.  The floor's plane in CAMERA coordinates is a property of the mounting: all frames of a camera share it, and
 * the fold's plane (ssd_camera_drift_fold) is the best estimate a batch holds.  For every frame i with moments[i].ground == 1,
 * moments[i].n_surfaces >= 1 and drift[camera_of_frame[i]].fit.status == SSD_GF_OK, gates[i].g[0] becomes n = fit.normal,
 * dist = fit.dist, gate = max(k_sigma * fit.rms, gate_min), and gates[i].n_surfaces is raised to at least 1; every other gate and every
 * other frame is left as given (make `gates` with ssd_surface_gates_from_moments first).  So a frame whose own ground fit was FEW or
 * DEGENERATE still contributes its floor points to the next fold, and all of a camera's frames are trimmed against one plane.
 * SSD_E_ARG, gates untouched: a null pointer, ncams outside 1 .. SSD_MAX_CAMERAS, nframes < 0, an index >= ncams, k_sigma not in
 * (0, 16], gate_min not in [0, 1]. */
int ssd_camera_ground_gates(const ssd_frame_moments *moments, const uint16_t *camera_of_frame, int nframes,
                            const ssd_camera_drift *drift /* ncams records */, int ncams, double k_sigma, double gate_min,
                            ssd_frame_gates *gates /* in/out, nframes */);

/* ---- surface gates on the device: refit passes chained with no host round trip ----------------------------------------------------
 * EXTENSION.  Between two refit passes stands one step, ssd_surface_gates_from_moments - a 3 x 3 eigen-solve per
 * surface.  Made on the host it costs a wait, a copy down and a copy up per pass, and a caller who enqueues ahead of its fetches loses
 * that the moment it asks for a refit.  k_surface_gates makes the gates on the device, from records in device memory, by the same text
 * as the host function (csrc/ssd_solve.h, both sides without FMA contraction).
 * Contract: frame i's ssd_frame_gates is byte for byte what ssd_surface_gates_from_moments(&rec[i], min_points, k_sigma, gate_min, ..)
 * fills, all 688 bytes of it (the header, zero gates at k >= n_surfaces and for FEW / DEGENERATE surfaces); moments at k >= n_surfaces
 * are not read.  A record whose n_surfaces lies outside 0 .. SSD_MAX_STEPS - which the host function refuses - gives the all-zero
 * record (n_surfaces = 0): the device has nobody to refuse to.
 *   ssd_enqueue_surface_gates                 records on the device -> gates on the device, on `stream`, without synchronising; the
 *                                             handle gives the device and the limit of nframes, nothing of it is touched.  d_gates
 *                                             must not overlap d_moments (not checked).
 *   ssd_enqueue_surface_refit_device          ssd_enqueue_surface_refit whose gates are made from d_prev (nframes records in device
 *   ssd_enqueue_cameras_surface_refit_device  memory: the first pass's, or a refit pass's) by k_surface_gates on the pass's stream, in
 *                                             front of the zeroing: no host copy, no wait.  d_prev == d_out is allowed.
 * The chain: ssd_enqueue_surface_moments(.., d_first); .._refit_device(d_prev = d_first, d_out); .._refit_device(d_prev = d_out, d_out);
 * no fetch between; with one workspace and with several (the pass runs on the stream its batch ran on, behind it).  Everything else
 * is ssd_enqueue_surface_refit's, shared: the "last whole enqueue" checks, the one set of device gates per handle (passes of every
 * kind run in the order of their calls, across workspaces), ssd_fetch_surface_refit, ssd_get_surface_refit_time (which includes the
 * gates kernel), the gate buffers made on the first call of any kind and counted in ssd_workspace_bytes.  The gates depend on camera
 * coordinates alone: the cameras form launches the same kernel.
 * SSD_E_ARG, before anything is launched or copied: what ssd_enqueue_surface_refit / ssd_enqueue_cameras_surface_refit refuse, k_sigma
 * not in (0, 16], gate_min not in [0, 1], a null d_prev, d_moments or d_gates, nframes outside 1 .. max_frames_per_batch.
 * A handle that never calls any of these allocates and launches nothing more.
 * Limits: the riser fit has no refit; ssd_pipeline_* does not refit; ssd_surface_fit_solve stays on the host (the camera's gate has a
 * device form of its own: ssd_enqueue_camera_ground_gates, below); the host paths below still finish a slice before the next one's
 * kernels go out. */
int ssd_enqueue_surface_gates(ssd_handle *h, const ssd_frame_moments *d_moments, int nframes, void *stream,
                              int min_points, double k_sigma, double gate_min, ssd_frame_gates *d_gates /* DEVICE, nframes */);
int ssd_enqueue_surface_refit_device(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                     const ssd_frame_moments *d_prev /* DEVICE, nframes */, int min_points, double k_sigma, double gate_min,
                                     ssd_frame_moments *d_out);
int ssd_enqueue_cameras_surface_refit_device(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                             const ssd_frame_moments *d_prev /* DEVICE, nframes */, int min_points, double k_sigma,
                                             double gate_min, ssd_frame_moments *d_out);
/* ssd_process_host_surfaces_refit / ssd_process_host_cameras_surfaces_refit with the gates made on the device: per slice an enqueue with
 * the first moments, `passes` device-gated refits behind it (the first from the first pass's records, later ones in place), then the
 * results and the records - the passes of a slice are waited for once (the copies of the records each end in a wait of their own,
 * behind it) where the host-gated functions wait once per pass.  Arguments,
 * refusals and every output (results, first, refit, out) are those functions', byte for byte. */
int ssd_process_host_surfaces_refit_device(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                                           ssd_frame_moments *first /* may be NULL */, ssd_frame_moments *refit /* may be NULL */,
                                           int min_points, double k_sigma, double gate_min, int passes /* 1..4 */, ssd_frame_surfaces *out);
int ssd_process_host_cameras_surfaces_refit_device(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                                   ssd_frame_result *results, ssd_frame_moments *first /* may be NULL */,
                                                   ssd_frame_moments *refit /* may be NULL */, int min_points, double k_sigma,
                                                   double gate_min, int passes /* 1..4 */, ssd_frame_surfaces *out);

/* ---- camera fold on the device: the camera's gate and the drift in one chain ------------------------------------------------------
 * EXTENSION.  ssd_camera_drift_fold was the one link of the drift watch that lived on the host alone, so the
 * camera's gate (ssd_camera_ground_gates: the best configuration profiles/camera_drift_refit_accuracy.txt records) cost a resident-frames
 * caller a wait, 1.5 KB per frame down and 688 bytes per frame up between two passes.  k_camera_fold folds records in device memory
 * by the host's own step (csrc/ssd_fold.h), k_camera_ground_gates solves each camera's sum and overlays its plane on the frames' gates
 * by the host's own text (csrc/ssd_solve.h, both sides without FMA contraction).
 *
 * ssd_camera_fold is the head of ssd_camera_drift, field for field: everything of it that needs no calibration. */
typedef struct
{
  int32_t camera, frames, frames_ground, frames_left;
  ssd_ground_moments m;
  int64_t n_far;
} ssd_camera_fold;               /* 104 bytes */

/* ssd_enqueue_camera_fold: d_fold[c] (DEVICE, ncams records) is byte for byte the first 104 bytes of out[c] of ssd_camera_drift_fold over
 * the same records (d_moments: DEVICE, nframes) and the same index (d_camera_of_frame: DEVICE, one int32 per frame - the form a
 * workspace keeps its own index in).  accumulate == 0: all 104 bytes of all ncams records are written, whatever was there, and nothing
 * behind them.  accumulate != 0: d_fold holds the records of earlier calls and the frames are folded on top in index order: two calls
 * equal one call over the concatenation, frames_left included.  A frame whose index lies outside 0 .. ncams - 1 - which the host function
 * refuses - is counted nowhere: the device has nobody to refuse to.  Moments at s[1..], and s[0] of a frame without a ground, are not
 * read.  Launches on `stream` without synchronising; the handle gives the device and the limit of nframes, nothing of it is touched.
 * SSD_E_ARG before anything is launched: a null pointer, nframes outside 1 .. max_frames_per_batch, ncams outside 1 .. SSD_MAX_CAMERAS. */
int ssd_enqueue_camera_fold(ssd_handle *h, const ssd_frame_moments *d_moments, const int32_t *d_camera_of_frame, int nframes, int ncams,
                            int accumulate, void *stream, ssd_camera_fold *d_fold /* DEVICE, ncams */);
/* ssd_enqueue_camera_ground_gates: d_gates (DEVICE, nframes, in/out) afterwards is byte for byte what ssd_camera_ground_gates leaves, given
 * drift[c].fit = ssd_ground_fit_solve(&d_fold[c].m, .., fold_min_points, ..): g[0] of frame i becomes n = normal, dist, gate =
 * max(k_sigma * rms, gate_min) and n_surfaces is raised to at least 1 when the frame has a ground (ground == 1, n_surfaces >= 1) and its
 * camera's status is SSD_GF_OK; every other byte stays as given.  normal, dist, rms and the status do not depend on the prior's
 * calibration, so the call takes no table; fit.tilt stays on the host.  A frame whose index lies outside 0 .. ncams - 1 is left as given.
 * Stream and handle as ssd_enqueue_camera_fold.  SSD_E_ARG before anything is launched: what ssd_enqueue_camera_fold refuses, k_sigma not
 * in (0, 16], gate_min not in [0, 1]. */
int ssd_enqueue_camera_ground_gates(ssd_handle *h, const ssd_frame_moments *d_moments, const int32_t *d_camera_of_frame, int nframes,
                                    const ssd_camera_fold *d_fold /* DEVICE, ncams */, int ncams, int fold_min_points, double k_sigma,
                                    double gate_min, void *stream, ssd_frame_gates *d_gates /* DEVICE, nframes, in/out */);
/* ssd_enqueue_cameras_surface_refit_device with the camera's gate: in front of the zeroing, on the pass's stream, k_surface_gates(d_prev)
 * into the handle's device gates, the fold of d_prev under the batch's own index and the table's count into a fold buffer of the handle's
 * (made on the first call, counted in ssd_workspace_bytes, one per handle like the device gates), and the overlay.  Frame i's record is
 * byte for byte ssd_enqueue_cameras_surface_refit under the gates ssd_surface_gates_from_moments, ssd_camera_drift_fold(fold_min_points)
 * and ssd_camera_ground_gates make from the downloaded d_prev.  d_prev == d_out is allowed.  Everything else - the refusals, streams and
 * workspaces, ssd_fetch_surface_refit, ssd_get_surface_refit_time (which includes the three kernels) - is that function's. */
int ssd_enqueue_cameras_surface_refit_folded(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                             const ssd_frame_moments *d_prev /* DEVICE, nframes */, int min_points, double k_sigma,
                                             double gate_min, int fold_min_points, ssd_frame_moments *d_out);
/* host only, no GPU needed: the head copied, then ssd_ground_fit_solve(&fold[c].m, &cams[c].cal, min_points, ..) per camera.  out is byte
 * for byte ssd_camera_drift_fold's over the records that made the fold.  SSD_E_ARG (out untouched): a null pointer, ncams outside
 * 1 .. SSD_MAX_CAMERAS, fold[c].camera != c. */
int ssd_camera_drift_from_fold(const ssd_camera_fold *fold, const ssd_camera *cams, int ncams, int min_points, ssd_camera_drift *out /* ncams */);
/* The drift watch on host frames with no per-frame record on the host.  Through the slices of ssd_process_host_cameras; per slice a
 * cameras enqueue with the first moments, `passes` (0 .. 4) device-gated refits (min_points, k_sigma, gate_min: those of
 * ssd_process_host_cameras_surfaces_refit_device) and an accumulating fold of the last records on the slice's stream; after the last slice
 * one copy of table-count x 104 bytes, then ssd_camera_drift_from_fold(fold_min_points).  results[nframes] is byte for byte
 * ssd_process_host_cameras', out[table count] byte for byte ssd_camera_drift_fold over the last pass's records of
 * ssd_process_host_cameras_surfaces_refit_device (passes == 0: over ssd_process_host_cameras_surfaces' records).
 * Per-frame gates only: a slice does not hold a camera's batch, and a refit needs the points again - the camera's gate is for resident
 * frames (ssd_enqueue_cameras_surface_refit_folded).  A slice is finished before the next one's kernels go out.
 * SSD_E_ARG before anything is copied: what ssd_process_host_cameras refuses, a null out, passes outside 0 .. 4, the gate rule. */
int ssd_process_host_cameras_drift(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                   ssd_frame_result *results, int min_points, double k_sigma, double gate_min, int passes /* 0..4 */,
                                   int fold_min_points, ssd_camera_drift *out /* table count */);

/* ---- tread clearance: what stands on each reported surface, and where --------------------------------------------------------------
 * EXTENSION.  A result says where every tread is; it does not say whether the tread is FREE.  A box, a foot or a
 * bag on a step lies in the points of no plateau, which the reference drops (pointcloud.cpp:285-294).  One more pass gathers, per reported
 * surface, the points that stand on it.  The rule is stated on public data only - the frame's ssd_frame_result, the calibration, the
 * points - in doubles without FMA contraction, in the order written; one text for host and device (csrc/ssd_clearance.h).
 * A frame whose status has SSD_ST_THROW, or with n_steps == 0, has no occupant.  Otherwise a point is an OCCUPANT OF SURFACE k (k in the
 * result's order) iff
 *   1. it is valid and in range exactly as a labelled point is: z > 0 on the float camera point (16-bit depth deprojected first, bit-equal
 *      to ssd_deproject_host), and w = A p + b - each row (a0 x + a1 y) + a2 z, then + b - strictly inside the measuring range;
 *   2. with ex = (r2[0] wx + r2[1] wy) + t2[0], ey = (r2[2] wx + r2[3] wy) + t2[1], ez = wz + world_z:
 *   3. fabs(ez - steps[j].height) > lo for EVERY j < n_steps - a slab around every reported height belongs to the surfaces, whatever
 *      their quadrilaterals say;
 *   4. k is the lowest index with ez > steps[k].height + lo && ez < steps[k].height + hi and (ex, ey) inside surface k's quadrilateral
 *      shrunk by margin:  ring FL, FR, BR, BL = quad[0..1], [2..3], [6..7], [4..5];  A2 = ((t0 + t1) + t2) + t3, t_i = x_i y_(i+1) -
 *      x_(i+1) y_i;  A2 == 0 or unordered: the surface takes nothing (quirk Q6's all-zero ground);  o = A2 > 0 ? 1 : -1;  per side
 *      dx = x_(i+1) - x_i, dy = y_(i+1) - y_i, c = o (dx (ey - y_i) - dy (ex - x_i));  kept iff c >= 0 && c c >= (margin margin)
 *      (dx dx + dy dy) on all four sides.  No square root, no division; a NaN corner keeps nothing.
 * The margin keeps the riser faces that hang over a tread's rim out (DESIGN.md section 7m has the figures).
 * Clearance moments of a frame: an ssd_frame_moments - the header as the surface moments' (n_surfaces = n_steps, ground), s[k] the ten sums
 * and n_far over surface k's occupants by the fixed-point rule of the surface fit as it stands; records at k >= n_surfaces are zero.
 * Clearance mask: width * height bytes per frame, k + 1 on an occupant of surface k, 0 elsewhere - a buffer of its own, NOT the label
 * mask, in the form ssd_surface_moments_host accepts: the host sums over the device's mask equal the device's moments byte for byte.
 * Out of scope: ssd_pipeline_* and ssd_enqueue_stages; the label mask (untouched); the tallest occupant point (a maximum, not a sum);
 * occupants inside the slabs of item 3 (an object lower than lo is not seen). */
typedef struct
{
  double margin;      /* [0, 1] m: how far inside the quadrilateral's sides an occupant must lie */
  double lo;          /* (0, 1] m: half-width of the slab around every reported height, and the band's lower end above the surface */
  double hi;          /* (lo, 8] m: the band's upper end above the surface */
} ssd_clearance_rule;

#define SSD_CL_FREE 0
#define SSD_CL_OCCUPIED 1
typedef struct
{
  int32_t status, reserved;   /* SSD_CL_FREE / SSD_CL_OCCUPIED */
  int64_t n, n_far;           /* the moments' */
  double centroid[3];         /* mean of the occupants, external world (as ssd_surface_fit's) */
  double height_mean;         /* centroid z - the step's height */
  double height_rms;          /* rms spread of the occupants along the world's up axis, metres */
  double from_front;          /* the centroid's distance behind the surface's front edge (FL -> FR), positive towards the back, metres */
  double along_front;         /* ... and its position along that edge from FL, metres */
  double extent[3];           /* square roots of the scatter's eigenvalues, descending, metres */
} ssd_clearance;              /* 104 bytes */

typedef struct
{
  int32_t n_surfaces, ground;
  ssd_clearance s[SSD_MAX_STEPS];
} ssd_frame_clearance;

/* The pass alone (k_clearance), against the workspace of the handle's last WHOLE enqueue, behind it on that batch's stream and in front
 * of a completion event of its own - every check, stream rule and withdrawal of ssd_enqueue_surface_refit (ssd_enqueue_cameras_clearance:
 * of ssd_enqueue_cameras_surface_refit; frame i is byte for byte a one-camera handle's).  d_out: nframes contiguous records; d_mask (may
 * be NULL): frame i's bytes at d_mask + i * mask_stride; both device memory, zeroed on the stream in front of the pass - of the mask only
 * the width * height bytes of every stride.  The pass reads the results k_final left, the state and the cell records, and writes the
 * caller's two buffers alone: nothing ssd_fetch* reads changes.  It may be repeated, with other rules, until the next enqueue takes the
 * workspace.  The first call makes events only: ssd_workspace_bytes does not move, and a handle that never calls it allocates and
 * launches nothing.  SSD_E_ARG before anything is launched: the refit's refusals, a null rule or destination, a rule outside the ranges
 * above, mask_stride < width * height with a mask. */
int ssd_enqueue_clearance(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                          const ssd_clearance_rule *rule, ssd_frame_moments *d_out, uint8_t *d_mask /* may be NULL */, size_t mask_stride);
int ssd_enqueue_cameras_clearance(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                  const ssd_clearance_rule *rule, ssd_frame_moments *d_out, uint8_t *d_mask /* may be NULL */, size_t mask_stride);
/* waits for the last clearance pass (SSD_E_ARG: there was none) */
int ssd_fetch_clearance(ssd_handle *h, void *stream);
/* the device time of the last clearance pass, the zeroing in front of it included (0 when timing was off for it) */
int ssd_get_clearance_time(ssd_handle *h, float *ms);
/* host only, no GPU needed: one frame's occupants by the shared text.  input, intr and frame as ssd_surface_moments_host; result: the
 * frame's; ground goes into the record's header as given.  out and mask (width * height bytes) may each be NULL.  SSD_E_ARG: a null
 * cfg, cal, frame, result or rule, a bad input, depth without good intrinsics, n_steps outside 0 .. SSD_MAX_STEPS, a rule outside its ranges. */
int ssd_clearance_host(const ssd_config *cfg, const ssd_calibration *cal, int input, const ssd_intrinsics *intr, const void *frame,
                       const ssd_frame_result *result, int ground, const ssd_clearance_rule *rule, ssd_frame_moments *out /* may be NULL */,
                       uint8_t *mask /* may be NULL */);
/* host only: a frame's clearance moments -> what stands on each surface.  Per surface k < n_surfaces: status OCCUPIED iff n + n_far >=
 * max(min_support, 1); n, n_far always; the doubles (0 unless occupied with n > 0): centroid formed as ssd_surface_fit_solve forms it,
 * height_mean = centroid z - steps[k].height, height_rms = sqrt of the exact centred scatter's variance along row 3 of cal->a,
 * from_front / along_front against the front edge quad[0..1] -> quad[2..3] (0 where that edge has no length), extent by the shared
 * Jacobi.  Records at k >= n_surfaces are zero.  SSD_E_ARG: a null pointer, n_surfaces outside 0 .. SSD_MAX_STEPS. */
int ssd_clearance_solve(const ssd_frame_moments *moments, const ssd_frame_result *result, const ssd_calibration *cal, int min_support,
                        ssd_frame_clearance *out);
/* frames in host memory through the slices of ssd_process_host (ssd_process_host_cameras): per slice enqueue, pass, fetch, solve.  Fills
 * results[nframes] (byte for byte ssd_process_host's / ssd_process_host_cameras'), out[nframes] (each frame solved against the handle's
 * calibration / its camera's) and, when not NULL, moments[nframes] and mask (nframes x width * height bytes, packed). */
int ssd_process_host_clearance(ssd_handle *h, const void *frames, int nframes, int input, const ssd_clearance_rule *rule, int min_support,
                               ssd_frame_result *results, ssd_frame_moments *moments /* may be NULL */, uint8_t *mask /* may be NULL */,
                               ssd_frame_clearance *out);
int ssd_process_host_cameras_clearance(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                       const ssd_clearance_rule *rule, int min_support, ssd_frame_result *results,
                                       ssd_frame_moments *moments /* may be NULL */, uint8_t *mask /* may be NULL */, ssd_frame_clearance *out);

/* ---- tread grid: free, occupied and unseen cells per tread, and a foothold ---------------------------------------------------------
 * EXTENSION.  A clearance record is one centroid per tread: it cannot say WHERE on the tread to step.  Two
 * objects give a centroid between them; an occupant hides the tread behind it, which is then neither occupied nor known to be free; and
 * whether something can be stepped over is a maximum, not a sum.  This pass lays a small top-down grid over every reported surface, in
 * the surface's own frame - SSD_TG_COLS cells along its front edge, SSD_TG_ROWS behind it - and counts per cell the tread points seen
 * there, the occupants there, and the tallest occupant.  The rule is stated on public data only, in doubles without FMA contraction, in
 * the order written; sqrt and / are correctly rounded; one text for host and device (csrc/ssd_treadgrid.h, on csrc/ssd_clearance.h).
 * A frame whose status has SSD_ST_THROW, or with n_steps == 0, gives a record that is zero apart from its header.  Otherwise
 *   1. validity and range are item 1 of the clearance rule; ex, ey, ez as in its item 2;
 *   2. a point is an OCCUPANT of surface k exactly as ssd_enqueue_clearance decides under rule.clearance (its items 3 and 4);
 *   3. otherwise it is a TREAD POINT of surface k iff k is the lowest index with !(fabs(ez - steps[k].height) > lo) and (ex, ey) inside
 *      surface k's quadrilateral shrunk by margin (the clearance rule's test).  No point is both;
 *   4. its cell on surface k: side 0 of the ring (FL -> FR) x0, y0, dx, dy, o as the clearance rule has them, L = sqrt(dx dx + dy dy);
 *      the grid is live iff o != 0 && L > 0;  ax = ex - x0, ay = ey - y0;  u = (dx ax + dy ay) / L;  v = (o (dx ay - dy ax)) / L
 *      (behind the front edge, positive inside for either ring orientation);  u0 = the least u of the ring's corners: 0 for FL, then
 *      if(ui < u0) u0 = ui for FR, BR, BL;  c = floor((u - u0) / cell), r = floor(v / cell) as doubles; in the grid iff
 *      c >= 0 && c < SSD_TG_COLS && r >= 0 && r < SSD_TG_ROWS, compared as doubles before any conversion (a NaN is out);
 *   5. a tread point in the grid adds 1 to seen[r][c], outside it (or on a grid that is not live) to n_seen_out; an occupant adds 1 to
 *      occ[r][c] or n_occ_out and raises top[r][c] or top_out to (int32_t)rint((ez - steps[k].height) 65536): units of 2^-16 m.
 * So for every frame and surface sum(occ) + n_occ_out equals n + n_far of the clearance record under the same rule.
 * Out of scope: ssd_pipeline_* and ssd_enqueue_stages; a mask; grids that follow a tread's curved sides; objects lower than lo. */
#define SSD_TG_COLS 32   /* cells along the front edge */
#define SSD_TG_ROWS 8    /* cells behind it */
typedef struct
{
  ssd_clearance_rule clearance;
  double cell;        /* [0.005, 1] m: a cell's side */
} ssd_tread_grid_rule;

typedef struct
{
  uint32_t n_seen_out, n_occ_out;   /* tread points / occupants of the surface that fall outside the grid */
  int32_t top_out, reserved;        /* the tallest of those occupants (units of 2^-16 m), 0 if none */
  uint32_t seen[SSD_TG_ROWS][SSD_TG_COLS];
  uint32_t occ[SSD_TG_ROWS][SSD_TG_COLS];
  int32_t top[SSD_TG_ROWS][SSD_TG_COLS];
} ssd_tread_grid;                   /* 3088 bytes */

typedef struct
{
  int32_t n_surfaces, ground;       /* as the clearance record's */
  ssd_tread_grid s[SSD_MAX_STEPS];
} ssd_frame_tread_grid;             /* 52504 bytes */

#define SSD_TG_OUT 0        /* the cell's centre is not inside the shrunk quadrilateral */
#define SSD_TG_FREE 1       /* tread seen, nothing on it */
#define SSD_TG_OCCUPIED 2
#define SSD_TG_UNSEEN 3     /* inside, but neither: hidden behind an occupant, or no data */
typedef struct
{
  uint8_t state[SSD_TG_ROWS][SSD_TG_COLS];
  int32_t n_free, n_occupied, n_unseen;
  int32_t foothold;                 /* 1: the rectangle below exists */
  int32_t col0, row0, cols, rows;   /* the best free rectangle, in cells (all 0 without a foothold) */
  double tallest;                   /* the tallest occupant of the surface, metres above it (0: none) */
  double centre[2];                 /* the rectangle's centre, external world x, y */
  double size[2];                   /* cols cell, rows cell: metres along the front edge and behind it */
} ssd_foothold;                     /* 328 bytes */

typedef struct
{
  int32_t n_surfaces, ground;
  ssd_foothold s[SSD_MAX_STEPS];
} ssd_frame_footholds;

/* The pass alone (k_tread_grid), against the workspace of the handle's last WHOLE enqueue, behind it on that batch's stream and in front
 * of a completion event of its own - every check, stream rule and withdrawal of ssd_enqueue_clearance (ssd_enqueue_cameras_tread_grid: of
 * ssd_enqueue_cameras_clearance; frame i is byte for byte a one-camera handle's).  d_out: nframes contiguous records in device memory,
 * zeroed on the stream in front of the kernel; records past nframes are not written.  It may be repeated, with other rules, until the
 * next enqueue takes the workspace.  The first call makes events only: ssd_workspace_bytes does not move, and a handle that never calls
 * it allocates and launches nothing.  SSD_E_ARG before anything is launched: the refit's refusals, a null rule or destination, a
 * clearance rule outside its ranges, cell outside [0.005, 1] or NaN. */
int ssd_enqueue_tread_grid(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                           const ssd_tread_grid_rule *rule, ssd_frame_tread_grid *d_out);
int ssd_enqueue_cameras_tread_grid(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                   const ssd_tread_grid_rule *rule, ssd_frame_tread_grid *d_out);
/* waits for the last tread grid pass (SSD_E_ARG: there was none) */
int ssd_fetch_tread_grid(ssd_handle *h, void *stream);
/* the device time of the last tread grid pass, the zeroing in front of it included (0 when timing was off for it) */
int ssd_get_tread_grid_time(ssd_handle *h, float *ms);
/* host only, no GPU needed: one frame's grids by the shared text.  Arguments and refusals as ssd_clearance_host's (out may not be NULL),
 * plus the rule's cell. */
int ssd_tread_grid_host(const ssd_config *cfg, const ssd_calibration *cal, int input, const ssd_intrinsics *intr, const void *frame,
                        const ssd_frame_result *result, int ground, const ssd_tread_grid_rule *rule, ssd_frame_tread_grid *out);
/* host only: a frame's grids -> the state of every cell and a foothold per surface k < n_surfaces.  A cell is OUT iff its centre, mapped
 * back by FL + ((u0 + (c + .5) cell) / L) e + (((r + .5) cell) / L) o (-dy, dx), is not inside the shrunk quadrilateral; else OCCUPIED
 * iff occ >= max(min_occ, 1); else FREE iff seen >= max(min_seen, 1); else UNSEEN.  tallest = max(top, top_out) / 65536.  The best
 * rectangle is the all-FREE axis-aligned rectangle of the largest area with cols >= ceil(foot_along / cell) and rows >=
 * ceil(foot_deep / cell) (a foot size of 0: at least one cell); ties go to the smallest row0, then the smallest col0, then the most
 * cols; none: foothold = 0 and the rectangle's fields are zero.  Records at k >= n_surfaces are zero.  SSD_E_ARG: a null pointer,
 * n_surfaces outside 0 .. SSD_MAX_STEPS, a rule outside its ranges, a negative or NaN foot size. */
int ssd_tread_grid_solve(const ssd_frame_tread_grid *grid, const ssd_frame_result *result, const ssd_tread_grid_rule *rule, int min_seen,
                         int min_occ, double foot_along, double foot_deep, ssd_frame_footholds *out);
/* frames in host memory through the slices of ssd_process_host (ssd_process_host_cameras): per slice enqueue, pass, fetch, solve.  Fills
 * results[nframes] (byte for byte ssd_process_host's / ssd_process_host_cameras'), out[nframes] and, when not NULL, grids[nframes]. */
int ssd_process_host_tread_grid(ssd_handle *h, const void *frames, int nframes, int input, const ssd_tread_grid_rule *rule, int min_seen,
                                int min_occ, double foot_along, double foot_deep, ssd_frame_result *results,
                                ssd_frame_tread_grid *grids /* may be NULL */, ssd_frame_footholds *out);
int ssd_process_host_cameras_tread_grid(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                        const ssd_tread_grid_rule *rule, int min_seen, int min_occ, double foot_along, double foot_deep,
                                        ssd_frame_result *results, ssd_frame_tread_grid *grids /* may be NULL */, ssd_frame_footholds *out);

/* ---- stair map: the tread grids of many frames and cameras on one staircase --------------------------------------------------------
 * EXTENSION.  A frame's tread grid is laid in the frame of that frame's OWN quadrilaterals, which move from frame
 * to frame, so the grids of two frames cannot be added; and what one camera cannot see behind an occupant (SSD_TG_UNSEEN) another camera,
 * or the same one a moment later, can.  A STAIR MAP is a staircase the caller gives, in the external world that ssd_set_cameras' cameras
 * share; this pass runs the tread grid's rule, unchanged, with that staircase in place of each frame's own result and adds every frame
 * that names the map into ONE record, an ssd_frame_tread_grid as it stands.  Everything counted is an integer sum or an integer
 * maximum, so the record is exact and independent of the order of frames, blocks and calls.
 *
 * The record of map m after a call with accumulate == 0 is, byte for byte, the fold (ssd_tread_grid_add) of
 *   ssd_tread_grid_host(cfg, cal_i, input, intr_i, frame_i, &maps[m].stairs, maps[m].ground, rule, &g_i)
 * over the frames i with map_of_frame[i] == m, in any order: the header is g_i's (n_surfaces = the map's n_steps and ground != 0; both 0
 * for a map with SSD_ST_THROW or n_steps == 0, whose record is all zero), every uint32_t is added, every int32_t top is maximised.
 * cal_i / intr_i are the handle's, or for a cameras batch those of frame i's camera.  A map no frame names: the header and zeros.  The
 * frame's own result, status and debug record are NOT read: a frame too poor for a detection of its own contributes like any other.
 * accumulate != 0: the same is added on top of what d_out holds, and the headers are rewritten - two calls equal one call over the
 * concatenation of their frames.
 * Out of scope: ssd_pipeline_* and ssd_enqueue_stages; a mask; a count of contributing frames per map (the caller holds map_of_frame);
 * choosing a frame's map on the device. */
#define SSD_MAX_STAIR_MAPS 64        /* 64 records of 52,504 bytes = 3.4 MB: what the host path stages */
#define SSD_STAIR_MAP_NONE 0xffff    /* a frame that names no map adds nothing */

typedef struct
{
  ssd_frame_result stairs;   /* the staircase, external world: n_steps, steps[]; read exactly as ssd_tread_grid_host reads a result */
  int32_t ground, reserved;  /* ground goes into the record's header as ssd_tread_grid_host's `ground` does */
} ssd_stair_map;             /* 1240 bytes */

/* host only: the fold's step.  acc's header becomes in's, every count of in is added to acc's, every top of acc is raised to in's.  If
 * any count would pass 2^32 - 1: SSD_E_CAP, and acc is untouched - a record whole or not at all.  SSD_E_ARG: a null pointer. */
int ssd_tread_grid_add(const ssd_frame_tread_grid *in, ssd_frame_tread_grid *acc);
/* host only: a reference staircase from a run of results.  Used frames: no SSD_ST_THROW, no SSD_ST_OVERFLOW, 0 < n_steps <=
 * SSD_MAX_STEPS, and the height and the eight quadrilateral coordinates of every step below n_steps finite.  Of those only the frames
 * with the most frequent n_steps are kept (ties go to the larger n_steps); per step, the height and each of the eight coordinates are
 * the LOWER MEDIAN over the kept frames (the value at index (n - 1) / 2 of the sorted values): no arithmetic, so the result is exact
 * and independent of the frames' order.  out is zeroed first; out->ground = ground as given; *n_used (may be NULL) = the kept frames.
 * No usable frame: n_steps = 0, *n_used = 0, SSD_OK.  SSD_E_ARG: a null results or out, nframes < 0. */
int ssd_stair_map_from_results(const ssd_frame_result *results, int nframes, int ground, ssd_stair_map *out, int *n_used);

/* The pass alone (k_stair_map; ssd_enqueue_cameras_stair_map: k_stair_map_cams), a fifth pass behind the handle's last WHOLE enqueue:
 * it needs that enqueue's cell records, its depth maps and its camera index, but not its results.  Refusals, stream rule, withdrawals
 * and the completion event of its own are ssd_enqueue_tread_grid's; it runs on one workspace and on several.
 * maps: nmaps records in HOST memory; map_of_frame: nframes entries in HOST memory, each below nmaps or SSD_STAIR_MAP_NONE (NULL: every
 * frame names map 0).  Both are copied during the call, through pinned buffers of the handle's own that the first call makes and
 * ssd_workspace_bytes counts from then on (a call waits for the previous call's copy before it refills them); a handle that never calls
 * this allocates and launches nothing.  d_out: nmaps contiguous records in DEVICE memory.  accumulate == 0 zeroes them on the stream in
 * front of the kernel; records past nmaps are not written.
 * SSD_E_ARG before anything is launched or copied: what ssd_enqueue_tread_grid refuses; null maps or d_out; nmaps outside 1 ..
 * SSD_MAX_STAIR_MAPS; a map's n_steps outside 0 .. SSD_MAX_STEPS (ssd_tread_grid_host refuses it); an index that is neither below nmaps
 * nor SSD_STAIR_MAP_NONE; a call in which (frames naming one map) x width x height exceeds 2^32 - 1 (computed in 64 bits), so that no
 * count can overflow within one call (an enqueue takes at most max_frames_per_batch frames, so only a handle made for tens of
 * thousands of frames can meet this bound here; the host forms, whose calls have no such limit, are where it bites).
 * ACROSS accumulating calls that bound is the caller's to keep: the device adds modulo 2^32 and does not report a carry. */
int ssd_enqueue_stair_map(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                          const ssd_stair_map *maps /* HOST, nmaps, copied during the call */, int nmaps,
                          const uint16_t *map_of_frame /* HOST, nframes; NULL: every frame names map 0 */,
                          const ssd_tread_grid_rule *rule, int accumulate, ssd_frame_tread_grid *d_out /* DEVICE, nmaps */);
int ssd_enqueue_cameras_stair_map(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                  const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule,
                                  int accumulate, ssd_frame_tread_grid *d_out);
/* waits for the last stair map pass (SSD_E_ARG: there was none) */
int ssd_fetch_stair_map(ssd_handle *h, void *stream);
/* the device time of the last stair map pass, the zeroing in front of it included (0 when timing was off for it) */
int ssd_get_stair_map_time(ssd_handle *h, float *ms);
/* frames in host memory through the slices of ssd_process_host (ssd_process_host_cameras): per slice an enqueue and the pass,
 * accumulate = 0 for the first slice and 1 after, into a buffer of the pass's own; nothing per frame is copied up.  Behind the last
 * slice one copy of nmaps records, then ssd_tread_grid_solve(grids + m, &maps[m].stairs, rule, ..) -> out[m] per map.  Fills
 * results[nframes] (byte for byte ssd_process_host's / ssd_process_host_cameras'), out[nmaps] and, when not NULL, grids[nmaps].  The
 * refusals are the enqueue's, the overflow bound held over the WHOLE call, and ssd_tread_grid_solve's for the foot sizes. */
int ssd_process_host_stair_map(ssd_handle *h, const void *frames, int nframes, int input, const ssd_stair_map *maps, int nmaps,
                               const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule, int min_seen, int min_occ,
                               double foot_along, double foot_deep, ssd_frame_result *results,
                               ssd_frame_tread_grid *grids /* nmaps, may be NULL */, ssd_frame_footholds *out /* nmaps */);
int ssd_process_host_cameras_stair_map(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                       const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule,
                                       int min_seen, int min_occ, double foot_along, double foot_deep, ssd_frame_result *results,
                                       ssd_frame_tread_grid *grids /* nmaps, may be NULL */, ssd_frame_footholds *out /* nmaps */);

/* ---- stair pose: a camera located against a stair map from its treads and risers ------------------------------------------------------
 * EXTENSION.  The ground fit refines CameraToWorld (a, b) from the floor and carries ToExternalWorld (r2, t2,
 * world_z) over from the prior; a camera that sees no floor, or whose yaw or place in the shared world is off, has no tool.  A stair map
 * has what is missing: its treads are horizontal planes at known heights (height, pitch, roll), its risers vertical planes under known
 * front edges (yaw, the place along the going).  One streaming pass sorts every point of a frame onto the MAP's planes and sums each
 * class into the exact integer moments of ssd_ground_moments; a host solve turns the moments of many frames into one rigid correction
 * and a whole ssd_calibration.  The frame's own detection is not read: every frame counts, as for the stair map.
 *
 * A point (float camera coordinates; 16-bit depth is deprojected first, bit-equal to ssd_deproject_host, under the prior's intrinsics) is
 * valid when z > 0; w = A p + b as K1's doubles form it (each row (a0 x + a1 y) + a2 z, then + b, no FMA); it is in range when w lies
 * strictly inside the x and y measuring range; (ex, ey) = r2 w_xy + t2 row sums left to right, ez = w.z + world_z.  A valid, in-range
 * point belongs to the first class that applies:
 *   tread k   the lowest k < n_steps with !(fabs(ez - h_k) > band) and (ex, ey) inside step k's quadrilateral shrunk by margin (the tread
 *             grid's tread point, against the map);
 *   riser i   the lowest i in 0 .. n_steps - 2 with ez > h_i + clear && ez < h_(i+1) - clear and, FL -> FR the front edge of step i + 1,
 *             (dx, dy) = FR - FL, L2 = dx dx + dy dy, a = ex - FL.x, b = ey - FL.y, c = b dx - a dy, t = a dx + b dy:
 *             c c <= (reach reach) L2 && t >= 0 && t <= L2 - no square root, no division; L2 == 0 or any NaN takes nothing;
 *   otherwise none.
 * A classified point adds the ten sums to its class (q = llrint(double(v) * 65536.0) per camera coordinate); one with some |q| >= 2^20
 * adds 1 to the class's n_far instead.  Everything summed is an integer: the device and ssd_stair_pose_host agree bit for bit.
 * The record is one per FRAME (a frame's sums cannot overflow - the ground fit's argument; a sum over frames can, so the fold over frames
 * is the host's, where overflow is caught): treads.n_surfaces = n_steps, treads.ground = the map's ground != 0, risers.n_surfaces =
 * max(n_steps - 1, 0), risers.ground = 0, classes past the counts zero.  A map with SSD_ST_THROW or n_steps == 0, and a frame that names
 * SSD_STAIR_MAP_NONE, give an all-zero record.
 *
 * The solve (ssd_stair_pose_solve) is ONE Gauss-Newton step of point-to-plane alignment formed from the moments alone.  A class takes part
 * when n >= max(min_points, 1), a tread also when its ring has an orientation (twice its signed area != 0), a riser when L2 > 0.  Tread k's
 * plane is normal (0, 0, 1), offset h_k; riser i's normal (-dy, dx, 0) / sqrt(L2), offset normal . FL.  With e = T p + c the prior's affine
 * map camera -> external world, the residual is r = n . e - d and the correction e' = Rot(w)(e - E) + E + t, E the centroid of all used
 * points; r and the Jacobian row [(e - E) x n ; n] are affine in p, so the 6 x 6 normal matrix and its right-hand side follow from each
 * class's n, s, ss - centroid and centred scatter exact in 128-bit integers, doubles after that.  The rotation columns are scaled by rho,
 * the rms distance of the used points from E, so that the six eigenvalues (cyclic Jacobi, divided by the point count) are comparable;
 * the directions with lambda_j >= observable * lambda_max, and above the 64 eps lambda_max rounding level, are kept and the step is
 * solved in their span.  A STRAIGHT staircase does not observe the translation along its edges: the expected dof is 5 (6 with risers in
 * two directions, 3 from treads alone).
 * SSD_SP_OBSERVABLE is the geometric mean of two ratios lambda / lambda_max from the spectra profiles/stair_pose_accuracy.txt records on the
 * median map of the 3-step scene: the largest of the direction a straight staircase does not observe - 0 there, the map's drawn edges
 * being exactly parallel, so the solve's rounding level 64 eps = 1.421e-14 stands in for it - and 8.533e-02, the smallest of a direction
 * it does observe.  A map whose edges are a little out of parallel lifts the unobserved direction above this default: a caller who
 * knows its staircase straight passes an `observable` of its own. */
#define SSD_SP_OBSERVABLE 3.5e-8
#define SSD_SP_MARGIN 0.03     /* the defaults of ssd_stair_pose_rule, metres: the tread grid's margin and slab, ... */
#define SSD_SP_BAND 0.03
#define SSD_SP_CLEAR 0.03      /* ... a riser point stays this far from the treads above and below it, ... */
#define SSD_SP_REACH 0.04      /* ... and within this of the plane under the front edge */

typedef struct
{
  double margin;   /* [0, 1]: how far inside a tread's sides a tread point lies */
  double band;     /* (0, 1]: |ez - h_k| <= band */
  double clear;    /* (0, 1]: a riser point lies in (h_i + clear, h_(i+1) - clear) */
  double reach;    /* (0, 1]: ... and within reach of the vertical plane under the front edge of step i + 1 */
} ssd_stair_pose_rule;

typedef struct
{
  ssd_camera prior;      /* the calibration the frames are read under (and the intrinsics, for 16-bit depth) */
  ssd_stair_map map;     /* the staircase, external world */
} ssd_stair_pose_target;

typedef struct
{
  ssd_frame_moments treads;   /* s[k]: tread k */
  ssd_frame_moments risers;   /* s[i]: the riser between steps i and i + 1 */
} ssd_stair_pose_moments;     /* 3008 bytes */

typedef struct
{
  int32_t status;             /* in this order: SSD_GF_FEW (no class used), SSD_GF_DEGENERATE (no direction kept, or no calibration), SSD_GF_OK */
  int32_t dof;                /* directions kept */
  uint32_t treads_used, risers_used;   /* bit k: tread k / riser k took part */
  int64_t n, n_far;           /* over the used classes */
  double rotation[3];         /* w, radians, external axes */
  double translation[3];      /* t, metres */
  double centre[3];           /* E */
  double eig[6];              /* of the scaled normal matrix over n, ascending */
  double rms_before;          /* of r over the used points */
  double rms_after;           /* ... as the linear model predicts it behind the step */
  ssd_calibration cal;        /* with R' = Rot(w) T (Rodrigues) and c' = Rot(w)(c - E) + E + t: the floor plane n0 = -row3(R'), dist = c'_z -
                                 world_z gives a, b (ssd_calibration_from_plane's code); r2 = R'[0:2,:] a[0:2,:]^T, t2 = c'_xy, world_z the
                                 prior's.  Unless status is SSD_GF_OK: the prior, and the doubles above 0 */
} ssd_stair_pose;

/* host only, no GPU needed: the rule restated for ONE frame.  input = SSD_INPUT_VERTICES (width * height xyz floats) or SSD_INPUT_DEPTH16
 * (width * height uint16; the prior's intrinsics are required).  SSD_E_ARG: a null pointer, a bad input, a rule outside its ranges (a NaN
 * fails), the map's n_steps outside 0 .. SSD_MAX_STEPS, depth input without valid intrinsics. */
int ssd_stair_pose_host(const ssd_config *cfg, const ssd_stair_pose_target *target, int input, const void *frame,
                        const ssd_stair_pose_rule *rule, ssd_stair_pose_moments *out);
/* host only: the fold's step.  acc's headers become in's and every int64 of in is added to acc's; if a sum would leave int64: SSD_E_CAP,
 * and acc is untouched - a record whole or not at all.  SSD_E_ARG: a null pointer. */
int ssd_stair_pose_add(const ssd_stair_pose_moments *in, ssd_stair_pose_moments *acc);
/* host only: the solve above.  moments: a frame's record or a fold of many.  Always SSD_OK for non-null arguments and a map whose n_steps
 * lies in 0 .. SSD_MAX_STEPS (else SSD_E_ARG). */
int ssd_stair_pose_solve(const ssd_stair_pose_moments *moments, const ssd_stair_pose_target *target, int min_points, double observable,
                         ssd_stair_pose *out);
/* The pass (k_stair_pose) over frames resident in device memory, on the caller's stream, in order, without synchronising: the ground
 * fit's contract - no detection workspace, nothing ssd_fetch* reads is touched; calls on different streams run in call order.
 * targets: ntargets records in HOST memory, 1 .. SSD_MAX_STAIR_MAPS; target_of_frame: nframes entries in HOST memory, each below
 * ntargets or SSD_STAIR_MAP_NONE (NULL: every frame names target 0); both are copied during the call.  The buffers (a record per frame
 * of max_frames_per_batch on the device and pinned, the targets, the index) are made on the first call and counted in
 * ssd_workspace_bytes from then on; a handle that never calls this allocates and launches nothing for it.
 * SSD_E_ARG before anything is launched or copied: the ground fit's refusals (null handle or frames, nframes outside 1 ..
 * max_frames_per_batch, a bad input, frames off their element's alignment or a stride that holds no frame), a null or bad rule, null
 * targets, ntargets out of range, a map's n_steps outside 0 .. SSD_MAX_STEPS, a bad index, depth input with a target without valid
 * intrinsics. */
int ssd_enqueue_stair_pose(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                           const ssd_stair_pose_target *targets /* HOST, ntargets */, int ntargets,
                           const uint16_t *target_of_frame /* HOST, nframes; NULL: 0 */, const ssd_stair_pose_rule *rule);
/* waits for the last ssd_enqueue_stair_pose and hands over its records, byte for byte ssd_stair_pose_host's; nframes <= its */
int ssd_fetch_stair_pose_moments(ssd_handle *h, ssd_stair_pose_moments *out, int nframes, void *stream);
/* waits likewise; per target of the last call the fold (ssd_stair_pose_add, frame order) of the records of the frames that name it,
 * then ssd_stair_pose_solve against that target.  out: that call's ntargets records.  SSD_E_CAP: a fold left int64. */
int ssd_fetch_stair_pose(ssd_handle *h, ssd_stair_pose *out, int min_points, double observable, void *stream);
/* the device time of the last pass, the zeroing in front of it and the copy of its records behind it included (0 when timing was off for it) */
int ssd_get_stair_pose_time(ssd_handle *h, float *ms);
/* frames in host memory (pinned or pageable), any nframes >= 1, in slices through the staging buffers of ssd_process_host; the records
 * are folded across the slices on the host.  moments (may be NULL): nframes records; out: ntargets. */
int ssd_process_host_stair_pose(ssd_handle *h, const void *frames, int nframes, int input, const ssd_stair_pose_target *targets, int ntargets,
                                const uint16_t *target_of_frame, const ssd_stair_pose_rule *rule, int min_points, double observable,
                                ssd_stair_pose_moments *moments /* may be NULL */, ssd_stair_pose *out /* ntargets */);

/* ---- depth fusion: one trimmed-median frame from n frames of a still camera -----------------------------------
 * A group is n 16-bit depth frames (1 <= n <= SSD_FUSE_MAX_FRAMES) of the handle's width x height, taken while the camera stands still:
 * along a pixel's ray its n samples measure one quantity.  Integers only.  For one pixel with samples d_0 .. d_(n-1):
 *   1. a sample is valid iff it is not 0; m = the number of valid samples.  m == 0: output 0, the pixel is EMPTY.  0 < m < min_valid:
 *      output 0, FEW.
 *   2. med = the lower median of the valid samples: the (m - 1) / 2-th smallest, counted from 0.
 *   3. a valid sample agrees iff |d_j - med| <= tol (no wrap); c = the number of agreeing samples (>= 1), s = their sum.
 *   4. c < min_agree: output 0, SPLIT.
 *   5. otherwise FUSED: output (2 s + c) / (2 c), the agreeing samples' mean rounded half up - within tol of med, never 0, never
 *      above 65535.
 *   6. the optional support byte is c for a fused pixel, else 0.
 * With the defaults a majority has to agree: a pixel that flickers between two surfaces gives the majority's surface or nothing, never a
 * depth between them.  Per group one exact record (the four counts add up to the pixel count; sum_abs_dev / sum_agree is the camera's
 * noise in raw units).  Within a batch of nframes frames group g is frames g * hop .. g * hop + n - 1, 1 <= hop <= n, ngroups =
 * (nframes - n) / hop + 1: hop == n gives disjoint groups (a batch of several cameras, each camera's frames together, gives one fused
 * frame per camera), hop == 1 a sliding temporal filter at the full frame rate. */
#define SSD_FUSE_MAX_FRAMES 16
#define SSD_FUSE_TOL 40              /* the default tol, raw units: 1 cm at the L515's 0.00025 m */
typedef struct
{
  int32_t min_valid, min_agree, tol, reserved;
} ssd_depth_fuse_rule;
typedef struct
{
  int64_t n_fused, n_empty, n_few, n_split;
  int64_t sum_valid;            /* the sum of m over all pixels */
  int64_t sum_agree;            /* the sum of c over fused pixels */
  int64_t sum_abs_dev;          /* over fused pixels, the sum over agreeing samples of |d_j - output| */
  int64_t reserved;
} ssd_depth_fuse_stats;         /* 64 bytes */
/* host only: min_valid = min_agree = (n + 1) / 2, tol = SSD_FUSE_TOL.  SSD_E_ARG: null, n outside 1 .. SSD_FUSE_MAX_FRAMES */
int ssd_depth_fuse_default_rule(int n, ssd_depth_fuse_rule *rule);
/* host only, no GPU needed: the rule over ONE group.  frames: frame j at frames + j * frame_stride_bytes (a multiple of 2 that holds a
 * frame when n > 1); rule NULL: the defaults for n; out: width * height values; support (may be NULL): as many bytes; stats: the
 * group's record.  SSD_E_ARG: a null pointer, width or height not positive, n out of range, a bad stride, a rule outside
 * 1 <= min_valid <= n, 1 <= min_agree <= n, 0 <= tol <= 65535. */
int ssd_depth_fuse_host(int width, int height, const uint16_t *frames, size_t frame_stride_bytes, int n, const ssd_depth_fuse_rule *rule,
                        uint16_t *out, uint8_t *support /* may be NULL */, ssd_depth_fuse_stats *stats);
/* The pass (k_depth_fuse) over depth frames resident in device memory, on the caller's stream, in order, without synchronising: the
 * ground fit's contract - no detection workspace, nothing ssd_fetch* reads is touched, no intrinsics or calibration needed; calls on
 * different streams run in call order.  Fused frame g goes to d_out + g * out_stride_bytes, its support bytes (d_support may be NULL) to
 * d_support + g * support_stride_bytes, byte for byte ssd_depth_fuse_host's.  A depth-input enqueue on the same stream may read d_out
 * with no host wait in between (one workspace or several: a lane's stream goes behind what the caller's stream holds).  The stats
 * buffer (max_frames_per_batch records on the device and pinned) is made on the first call and counted in ssd_workspace_bytes from
 * then on; a handle that never calls this allocates, creates and launches nothing for it.
 * SSD_E_ARG before anything is launched or copied: a null handle, input or output; n outside 1 .. SSD_FUSE_MAX_FRAMES; hop outside
 * 1 .. n; nframes < n, nframes or ngroups above max_frames_per_batch; a rule out of range; frames or output off 2-byte alignment or a
 * stride that holds no frame (support: a stride below width * height with more than one group); an output or support range that
 * overlaps the input range. */
int ssd_enqueue_depth_fuse(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                           int n, int hop, const ssd_depth_fuse_rule *rule /* NULL: the defaults for n */,
                           void *d_out, size_t out_stride_bytes, uint8_t *d_support /* may be NULL */, size_t support_stride_bytes);
/* waits for the last ssd_enqueue_depth_fuse and hands over its groups' records; ngroups <= its */
int ssd_fetch_depth_fuse(ssd_handle *h, ssd_depth_fuse_stats *out, int ngroups, void *stream);
/* the device time of the last pass, the zeroing in front of it and the copy of its records behind it included (0 when timing was off for it) */
int ssd_get_depth_fuse_time(ssd_handle *h, float *ms);
/* depth frames in host memory (pinned or pageable), disjoint groups only: frames g * n .. g * n + n - 1 are fused on the device and
 * the fused frame is detected, slice by slice through the staging buffers of ssd_process_depth_host.  results: nframes / n records, byte
 * for byte ssd_process_depth_host's over ssd_depth_fuse_host's output; fused (may be NULL): nframes / n packed frames; stats (may be
 * NULL): as many records.  SSD_E_ARG: nframes no multiple of n, n above max_frames_per_batch, no intrinsics, a rule out of range. */
int ssd_process_depth_host_fused(ssd_handle *h, const uint16_t *depth, int nframes, int n, const ssd_depth_fuse_rule *rule,
                                 ssd_frame_result *results /* nframes / n */, uint16_t *fused /* may be NULL */,
                                 ssd_depth_fuse_stats *stats /* may be NULL */);

/* ---- depth edge filter: mixed and lone pixels out of ONE frame, from its spatial neighbours ---------------------
 * A frame is width x height 16-bit depth samples.  For the pixel with sample d, its neighbours are the up to eight pixels around it that
 * lie inside the frame; nothing outside the frame exists.  The decision is taken from the INPUT frame alone, never from another pixel's
 * output: the result does not depend on order.  Integers only:
 *   t(d)  = min(65535, tol + ((d * slope) >> 12))                       (32 bits)
 *   near(q): q exists, d_q != 0, |d_q - d| <= t(d)                      (the difference in 32 bits: it cannot wrap)
 *   c     = the number of near neighbours, 0 .. 8
 *   bridged: for one of the four opposite pairs (W/E, N/S, NW/SE, NE/SW) whose two pixels both exist and are valid (not 0),
 *            (d_a + t < d and d + t < d_b) or (d_b + t < d and d + t < d_a)
 * The classes, tested in this order: EMPTY d == 0 -> 0; LONE c < min_support -> 0; BRIDGE bridge != 0 and bridged -> 0; otherwise KEPT
 * -> d.  So a pixel that lies more than t from valid pixels on both sides of it, on opposite sides in depth, always goes (a mixed pixel
 * at a depth discontinuity), and a surface whose step from pixel to pixel is at most t loses nothing to BRIDGE.  slope lets t grow with
 * the depth: a tread seen at a grazing angle steps from image row to image row in proportion to its depth.  The optional class byte is
 * SSD_EDGE_KEPT / _EMPTY / _LONE / _BRIDGE; per frame one exact record whose four counts add up to the pixel count. */
#define SSD_EDGE_KEPT 0
#define SSD_EDGE_EMPTY 1
#define SSD_EDGE_LONE 2
#define SSD_EDGE_BRIDGE 3
#define SSD_EDGE_SLOPE 0             /* the default slope, fixed by measurement (profiles/depth_edges_accuracy.txt) */
typedef struct
{
  int32_t min_support;          /* 0 .. 8; 0 switches the LONE test off */
  int32_t bridge;               /* 0 switches the BRIDGE test off */
  int32_t tol;                  /* 0 .. 65535, raw units */
  int32_t slope;                /* 0 .. 4096, in 1 / 4096 of the pixel's own depth */
} ssd_depth_edge_rule;
typedef struct
{
  int64_t n_kept, n_empty, n_lone, n_bridge;
  int64_t sum_support;          /* the sum of c over kept pixels */
  int64_t reserved[3];
} ssd_depth_edge_stats;         /* 64 bytes */
/* host only: min_support = 2, bridge = 1, tol = SSD_FUSE_TOL, slope = SSD_EDGE_SLOPE.  SSD_E_ARG: null */
int ssd_depth_edge_default_rule(ssd_depth_edge_rule *rule);
/* host only, no GPU needed: the rule over ONE packed frame.  rule NULL: the defaults; out: width * height values; cls (may be NULL): as
 * many bytes; stats: the frame's record.  frame and out must not overlap.  SSD_E_ARG: a null pointer, width or height not positive, a
 * rule outside 0 <= min_support <= 8, 0 <= tol <= 65535, 0 <= slope <= 4096. */
int ssd_depth_edges_host(int width, int height, const uint16_t *frame, const ssd_depth_edge_rule *rule, uint16_t *out,
                         uint8_t *cls /* may be NULL */, ssd_depth_edge_stats *stats);
/* The pass (k_depth_edges) over depth frames resident in device memory, on the caller's stream, in order, without synchronising: the
 * contract of ssd_enqueue_depth_fuse - no detection workspace, nothing ssd_fetch* reads is touched, no intrinsics or calibration needed;
 * calls on different streams run in call order.  Filtered frame i goes to d_out + i * out_stride_bytes, its class bytes (d_cls may be
 * NULL) to d_cls + i * cls_stride_bytes, byte for byte ssd_depth_edges_host's.  A depth-input enqueue on the same stream may read d_out
 * with no host wait in between, and d_frames may be what ssd_enqueue_depth_fuse wrote on that stream.  The records
 * (max_frames_per_batch on the device and pinned) are made on the first call and counted in ssd_workspace_bytes from then on.
 * SSD_E_ARG before anything is launched or copied: a null handle, input or output; nframes outside 1 .. max_frames_per_batch; a rule
 * out of range; frames or output off 2-byte alignment or a stride that holds no frame; a class stride below a frame's bytes (width *
 * height) with more than one frame; ANY overlap of the output or class range with the input range (a stencil in place is a race). */
int ssd_enqueue_depth_edges(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                            const ssd_depth_edge_rule *rule /* NULL: the defaults */, void *d_out, size_t out_stride_bytes,
                            uint8_t *d_cls /* may be NULL */, size_t cls_stride_bytes);
/* waits for the last ssd_enqueue_depth_edges and hands over its frames' records; nframes <= its */
int ssd_fetch_depth_edges(ssd_handle *h, ssd_depth_edge_stats *out, int nframes, void *stream);
/* the device time of the last pass, the zeroing in front of it and the copy of its records behind it included (0 when timing was off for it) */
int ssd_get_depth_edges_time(ssd_handle *h, float *ms);
/* depth frames in host memory (pinned or pageable): every frame is filtered on the device and the filtered frame is detected, slice by
 * slice through the staging buffers of ssd_process_depth_host.  results: nframes records, byte for byte ssd_process_depth_host's over
 * ssd_depth_edges_host's output; filtered (may be NULL): nframes packed frames; stats (may be NULL): as many records. */
int ssd_process_depth_host_edges(ssd_handle *h, const uint16_t *depth, int nframes, const ssd_depth_edge_rule *rule,
                                 ssd_frame_result *results, uint16_t *filtered /* may be NULL */, ssd_depth_edge_stats *stats /* may be NULL */);

/* ---- depth warp: the frame another pose would have seen, so that frames of a moving camera can be fused ---------
 * A view takes the source camera's coordinates to the target camera's (p_dst = r p_src + t, r row-major) and names the SOURCE frame's
 * intrinsics; the target's intrinsics dst are one ssd_intrinsics per call.  For the source pixel (u, v) with sample d, no FMA anywhere:
 *   1. d == 0: EMPTY.
 *   2. (x, y, z) in float, bit-equal to ssd_deproject_host under src: dm = d * depth_units, x = dm * ((u - ppx) / fx), y likewise, z = dm.
 *   3. in doubles, row sums left to right, then the translation: X = ((r0 x + r1 y) + r2 z) + t0, Y and Z likewise.
 *   4. !(Z > 0): BEHIND.
 *   5. q = floor(Z / double(dst.depth_units) + 0.5); !(q >= 1 && q <= 65535): RANGE.
 *   6. uf = (X / Z) * double(dst.fx) + double(dst.ppx), vf likewise with fy and ppy; a = floor(uf + 0.5), b = floor(vf + 0.5);
 *      a >= 0 && a < width && b >= 0 && b < height is tested in doubles before any conversion (a NaN fails it).  Not inside: OUTSIDE.
 *   7. otherwise LANDED on the target pixel (a, b) with the value q.
 * The output pixel is the smallest q that landed on it - the nearest surface wins -, 0 where none landed: the minimum is commutative, so
 * the frame does not depend on any order.  One sample, one pixel: no splat.  The identity view with src == dst gives the input back
 * byte for byte.  Per frame one exact record: the five classes add up to the pixel count, n_filled counts the output pixels that are
 * not 0 (n_landed - n_filled samples shared a pixel with a nearer one).  Output frame i is source frame i under view i; the pass knows
 * no groups - ssd_enqueue_depth_fuse behind it does. */
typedef struct
{
  double r[9];                  /* source camera -> target camera, row-major rotation */
  double t[3];                  /* ... and translation, metres */
  ssd_intrinsics src;           /* the source frame's intrinsics */
  int32_t reserved[1];
} ssd_depth_warp_view;          /* 120 bytes */
typedef struct
{
  int64_t n_empty, n_behind, n_range, n_outside, n_landed;
  int64_t n_filled;             /* output pixels that are not 0 */
  int64_t reserved[2];
} ssd_depth_warp_stats;         /* 64 bytes */
/* host only: the view between two cameras whose calibrations share one external world.  With e = T p + c a camera's affine map from
 * camera coordinates to the external world (a and b, then r2 and t2 on x and y, world_z on z), r = T_dst^-1 T_src and t = T_dst^-1
 * (c_src - c_dst); the inverse by cofactors, in doubles; out->src = src->intr.  SSD_E_ARG: null; src without (valid) intrinsics; a
 * non-finite entry; |det T_dst| < 1e-9 (a calibration has |det| = 1). */
int ssd_depth_warp_view_between(const ssd_camera *src, const ssd_camera *dst, ssd_depth_warp_view *out);
/* host only, no GPU needed: the rule over ONE packed frame.  out: width * height values; stats: the frame's record.  frame and out must
 * not overlap.  SSD_E_ARG: a null pointer, width or height not positive, a view with a non-finite entry or invalid intrinsics, dst
 * invalid. */
int ssd_depth_warp_host(int width, int height, const uint16_t *frame, const ssd_depth_warp_view *view, const ssd_intrinsics *dst,
                        uint16_t *out, ssd_depth_warp_stats *stats);
/* The pass (k_depth_warp) over depth frames resident in device memory, on the caller's stream, in order, without synchronising: the
 * contract of ssd_enqueue_depth_fuse - no detection workspace, nothing ssd_fetch* reads is touched, the handle's intrinsics and
 * calibration are not read; calls on different streams run in call order.  views: HOST memory, nframes entries, restated and copied
 * during the call.  Warped frame i goes to d_out + i * out_stride_bytes, byte for byte ssd_depth_warp_host's; the pass zeroes the
 * frames' own bytes first and writes no other byte.  ssd_enqueue_depth_fuse, ssd_enqueue_depth_edges or a depth-input enqueue on the
 * same stream may read d_out with no host wait in between.  The records and the views' table (max_frames_per_batch of each on the
 * device and pinned) are made on the first call and counted in ssd_workspace_bytes from then on; a handle that never calls this
 * allocates, creates and launches nothing for it.
 * The 16-bit output is written by compare-and-swap on the aligned 32-bit word that holds a pixel, so SSD_E_ARG, before anything is
 * launched or copied, also for: d_out or out_stride_bytes no multiple of 4; width * height odd.  And for: a null handle, frames, views,
 * dst or output; nframes outside 1 .. max_frames_per_batch; frames off 2-byte alignment or a stride that holds no frame; ANY overlap
 * of the output and input ranges; a view with a non-finite entry or invalid intrinsics; dst invalid. */
int ssd_enqueue_depth_warp(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                           const ssd_depth_warp_view *views /* HOST, nframes */, const ssd_intrinsics *dst, void *d_out,
                           size_t out_stride_bytes);
/* waits for the last ssd_enqueue_depth_warp and hands over its frames' records; nframes <= its */
int ssd_fetch_depth_warp(ssd_handle *h, ssd_depth_warp_stats *out, int nframes, void *stream);
/* the device time of the last pass: the zeroing in front of it and the copy of its records behind it included, the views' upload not
 * (0 when timing was off for it) */
int ssd_get_depth_warp_time(ssd_handle *h, float *ms);
/* depth frames in host memory (pinned or pageable) of a moving camera, disjoint groups of n: frame i is warped under views[i] into the
 * view dst - which must equal the intrinsics the handle detects under (ssd_set_intrinsics) -, every n warped frames are fused
 * (fuse_rule NULL: the defaults for n) and the fused frame is detected, slice by slice through the staging buffers of
 * ssd_process_depth_host.  results: nframes / n records, byte for byte ssd_process_depth_host's over ssd_depth_fuse_host's over
 * ssd_depth_warp_host's output; fused (may be NULL): nframes / n packed frames; warp_stats (may be NULL): nframes records; fuse_stats
 * (may be NULL): nframes / n.  SSD_E_ARG: as ssd_process_depth_host_fused, width * height odd, a bad view, dst not the handle's. */
int ssd_process_depth_host_warp_fused(ssd_handle *h, const uint16_t *depth, int nframes, int n, const ssd_depth_warp_view *views,
                                      const ssd_intrinsics *dst, const ssd_depth_fuse_rule *fuse_rule,
                                      ssd_frame_result *results /* nframes / n */, uint16_t *fused /* may be NULL */,
                                      ssd_depth_warp_stats *warp_stats /* may be NULL */, ssd_depth_fuse_stats *fuse_stats /* may be NULL */);

/* ---- depth fill: the holes and the one-pixel see-through that the forward warp leaves, closed from ONE frame ------
 * A frame is width x height 16-bit depth samples; a pixel outside the frame is the sample 0.  The decision for the pixel with sample d is
 * taken from the INPUT frame alone, never from another pixel's output: the result does not depend on order.  Integers only.  The four
 * opposite pairs (a, b) of its neighbours are taken in the order W/E, N/S, NW/SE, NE/SW:
 *   lo = min(a, b), hi = max(a, b), t = min(65535, tol + ((lo * slope) >> 12))      (32 bits)
 *   agrees: a != 0 and b != 0 and hi - lo <= t
 *   m     = (a + b + 1) >> 1                      (= lo + ((hi - lo + 1) >> 1): it fits 16 bits and lies in lo .. hi)
 *   covers: agrees and hi + t < d                 (32 bits, cannot wrap)
 * The classes, tested in this order: EMPTY d == 0 and fewer than min_pairs agreeing pairs -> 0; FILLED d == 0 otherwise -> the m of the
 * agreeing pair with the smallest hi - lo, the first in the order above on a tie; COVERED d != 0, cover != 0 and at least cover covering
 * pairs -> the m of the covering pair with the smallest hi - lo, the first on a tie (a background sample seen through a one-pixel crack
 * of a nearer surface); otherwise KEPT -> d.  So a sample is only ever put between two samples that agree on opposite sides of the
 * pixel, never nearer than both or farther than both: a rim is not fattened.  With cover 0 a frame without zeros comes back byte for
 * byte.  The optional class byte is SSD_FILL_KEPT / _EMPTY / _FILLED / _COVERED; per frame one exact record whose four counts add up to
 * the pixel count. */
#define SSD_FILL_KEPT 0
#define SSD_FILL_EMPTY 1
#define SSD_FILL_FILLED 2
#define SSD_FILL_COVERED 3
typedef struct
{
  int32_t min_pairs;            /* 1 .. 4: the agreeing pairs a hole needs */
  int32_t cover;                /* 0 .. 4: the covering pairs a valid pixel needs to be replaced; 0 switches the COVERED test off */
  int32_t tol;                  /* 0 .. 65535, raw units */
  int32_t slope;                /* 0 .. 4096, in 1 / 4096 of the pair's lower sample */
} ssd_depth_fill_rule;          /* 16 bytes */
typedef struct
{
  int64_t n_kept, n_empty, n_filled, n_covered;
  int64_t sum_pairs;            /* the agreeing pairs of FILLED pixels plus the covering pairs of COVERED pixels */
  int64_t sum_spread;           /* the hi - lo of every pair used: per FILLED or COVERED pixel, that of the pair whose m it took */
  int64_t reserved[2];
} ssd_depth_fill_stats;         /* 64 bytes */
/* host only: min_pairs = 1, cover = 1, tol = SSD_FUSE_TOL, slope = 0.  SSD_E_ARG: null */
int ssd_depth_fill_default_rule(ssd_depth_fill_rule *rule);
/* host only, no GPU needed: the rule over ONE packed frame.  rule NULL: the defaults; out: width * height values; cls (may be NULL): as
 * many bytes; stats: the frame's record.  frame and out must not overlap.  SSD_E_ARG: a null pointer, width or height not positive, a
 * rule outside 1 <= min_pairs <= 4, 0 <= cover <= 4, 0 <= tol <= 65535, 0 <= slope <= 4096. */
int ssd_depth_fill_host(int width, int height, const uint16_t *frame, const ssd_depth_fill_rule *rule, uint16_t *out,
                        uint8_t *cls /* may be NULL */, ssd_depth_fill_stats *stats);
/* The pass (k_depth_fill) over depth frames resident in device memory, on the caller's stream, in order, without synchronising: the
 * contract of ssd_enqueue_depth_edges - no detection workspace, nothing ssd_fetch* reads is touched, no intrinsics or calibration needed;
 * calls on different streams run in call order.  Filled frame i goes to d_out + i * out_stride_bytes, its class bytes (d_cls may be
 * NULL) to d_cls + i * cls_stride_bytes, byte for byte ssd_depth_fill_host's.  d_frames may be what ssd_enqueue_depth_warp wrote on
 * that stream, and ssd_enqueue_depth_fuse, ssd_enqueue_depth_edges or a depth-input enqueue on it may read d_out, with no host wait in
 * between.  The records (max_frames_per_batch on the device and pinned) are made on the first call and counted in ssd_workspace_bytes
 * from then on; a handle that never calls this allocates, creates and launches nothing for it.
 * SSD_E_ARG before anything is launched or copied: a null handle, input or output; nframes outside 1 .. max_frames_per_batch; a rule
 * out of range; frames or output off 2-byte alignment or a stride that holds no frame; a class stride below a frame's bytes (width *
 * height) with more than one frame; ANY overlap of the output or class range with the input range (a stencil in place is a race). */
int ssd_enqueue_depth_fill(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                           const ssd_depth_fill_rule *rule /* NULL: the defaults */, void *d_out, size_t out_stride_bytes,
                           uint8_t *d_cls /* may be NULL */, size_t cls_stride_bytes);
/* waits for the last ssd_enqueue_depth_fill and hands over its frames' records; nframes <= its */
int ssd_fetch_depth_fill(ssd_handle *h, ssd_depth_fill_stats *out, int nframes, void *stream);
/* the device time of the last pass, the zeroing in front of it and the copy of its records behind it included (0 when timing was off for it) */
int ssd_get_depth_fill_time(ssd_handle *h, float *ms);
/* depth frames in host memory (pinned or pageable): every frame is filled on the device and the filled frame is detected, slice by
 * slice through the staging buffers of ssd_process_depth_host.  results: nframes records, byte for byte ssd_process_depth_host's over
 * ssd_depth_fill_host's output; filled (may be NULL): nframes packed frames; stats (may be NULL): as many records. */
int ssd_process_depth_host_fill(ssd_handle *h, const uint16_t *depth, int nframes, const ssd_depth_fill_rule *rule,
                                ssd_frame_result *results, uint16_t *filled /* may be NULL */, ssd_depth_fill_stats *stats /* may be NULL */);
/* ssd_process_depth_host_warp_fused with the fill between the warp and the fusion: frame i is warped under views[i], the warped frame
 * filled (fill_rule NULL: the defaults), every n filled frames fused and the fused frame detected.  results: nframes / n records, byte
 * for byte ssd_process_depth_host's over ssd_depth_fuse_host's over ssd_depth_fill_host's over ssd_depth_warp_host's output; fused (may
 * be NULL): nframes / n packed frames; warp_stats and fill_stats (may be NULL): nframes records each; fuse_stats (may be NULL): nframes
 * / n.  SSD_E_ARG: as ssd_process_depth_host_warp_fused, a fill rule out of range. */
int ssd_process_depth_host_warp_fill_fused(ssd_handle *h, const uint16_t *depth, int nframes, int n, const ssd_depth_warp_view *views,
                                           const ssd_intrinsics *dst, const ssd_depth_fill_rule *fill_rule,
                                           const ssd_depth_fuse_rule *fuse_rule, ssd_frame_result *results /* nframes / n */,
                                           uint16_t *fused /* may be NULL */, ssd_depth_warp_stats *warp_stats /* may be NULL */,
                                           ssd_depth_fill_stats *fill_stats /* may be NULL */,
                                           ssd_depth_fuse_stats *fuse_stats /* may be NULL */);

/* stage selector for profiling / roofline measurement: runs only the chosen stage(s) of the pipeline */
#define SSD_STAGE_HIST 1       /* K1: transform + crop + bin + histogram */
#define SSD_STAGE_PEAKS 2
#define SSD_STAGE_RASTER 4     /* K2 */
#define SSD_STAGE_OUTLINE 8    /* K3 */
#define SSD_STAGE_QUADS 16
#define SSD_STAGE_INQUAD 32    /* K4 */
#define SSD_STAGE_FINAL 64     /* K5 */
#define SSD_STAGE_ALL 127
int ssd_enqueue_stages(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream, int stages);

/* Per-stage device time of the last enqueue, measured with HIP events recorded on the stream the kernels
 * run on: ms[0..6] = hist, peaks, raster, outline, quads, inquad, final.  Enable before enqueueing. */
#define SSD_TIMING_SLOTS 64
int ssd_set_timing(ssd_handle *h, int enable);
int ssd_get_stage_times(ssd_handle *h, float ms[7]);
/* the same for an earlier enqueue: back = 0 is the last, 1 the one before, ... (< SSD_TIMING_SLOTS),
 * so a timed loop can read all its steps after one final synchronisation */
int ssd_get_stage_times_back(ssd_handle *h, int back, float ms[7]);
/* single-pass batches (section "Batches" below) run one kernel in front of the seven stages, k_predict: its time for the same enqueue
 * (0 when the enqueue did not run it) */
int ssd_get_predict_time_back(ssd_handle *h, int back, float *ms);
/* the label kernel's time for the same enqueue (0 when that enqueue wrote no labels) */
int ssd_get_labels_time_back(ssd_handle *h, int back, float *ms);
/* its twin for the riser labels' kernel, which runs behind the event that closes the label kernel's time (0 when that enqueue
 * marked nothing: riser labels or risers off, or no labels written) */
int ssd_get_riser_labels_time_back(ssd_handle *h, int back, float *ms);

/* Stairs::serialize(): returns the text length, or SSD_E_CAP. A frame whose status has SSD_ST_THROW
 * serialises to the empty string (the reference process terminates instead of printing). */
int ssd_serialize(const ssd_frame_result *r, char *buf, size_t cap);

/* ---- intermediates for parity tests ---------------------------------------- */
typedef struct
{
  int32_t peak_bin, bin_lo, bin_hi;     /* Plateau::height and the chosen pair */
  int32_t eff_lo, eff_hi;               /* bins that actually feed this plateau (after earlier plateaus took theirs) */
  int32_t n_points;
  int32_t is_step, outline_found, valid;
  int32_t n_scans_right, n_scans_left;
  int32_t scans_right[SSD_MAX_SCANS][3];
  int32_t scans_left[SSD_MAX_SCANS][3];
  int32_t n_edge_pts[4];
  int32_t line[4][3];
  double bounds[4][2][2];
  double base_line[3];
  int32_t vedge_found[2];
  int32_t n_vpts[2];
  int32_t vpts[2][SSD_MAX_EDGE_PTS][2];
  int32_t best_pt[2][2];
  double vline[2][3];
  int32_t corner_found[4];
  double quad_img[8];
  double quad_world[8];
  int32_t quad_err;
  int32_t n_in_quad;
  int64_t sum_z_fix;                    /* sum of round(z * 2^40) over the in-quad points */
  double mean_z;
} ssd_debug_plateau;

typedef struct
{
  int32_t status;
  int32_t n_nonzero, n_inrange, n_oob;
  int32_t n_bins, min_height, min_img_y_extent;
  uint32_t hist[SSD_MAX_BINS];
  int32_t n_peaks;
  int32_t peaks[SSD_MAX_PLATEAUS];
  int32_t n_plateaus, first_step, ground_ind, first_valid_ind;
  double ground_quad_world[8];
  int32_t ground_quad_err;
  int32_t ground_n_in_quad;
  double ground_mean_z;
  int32_t ground_front_valid;
  int32_t ground_n_pts;
  int32_t ground_pts[SSD_MAX_SCANS][2];
  int32_t ground_line[3];
  double ground_front_img[4];
  ssd_debug_plateau plateaus[SSD_MAX_PLATEAUS];
} ssd_debug_frame;

/* Enables debug capture for subsequent enqueues (costs memory and time; off by default).  enable = 1: the records below and
 * the raw / closed images (for which the whole ground image is rastered, not only the pixel strips the bottom scan reads);
 * enable = 2: the records only — the kernels run exactly as without capture and report their intermediates; 0: off. */
int ssd_set_debug(ssd_handle *h, int enable);
/* Copies the debug record of frame `frame` of the last batch. */
int ssd_get_debug(ssd_handle *h, int frame, ssd_debug_frame *out);
/* Raw (pre-close) and closed plateau images of the last batch as H x W bytes (0 / 0xff), like the
 * reference's cv::Mat.  step_slot = index among the step plateaus, or -1 for the ground image.
 * Only valid when capture with images (ssd_set_debug(h, 1)) was on for the batch. */
int ssd_get_debug_image(ssd_handle *h, int frame, int step_slot, int closed, uint8_t *out);

/* pinned (page-locked) host memory for frames handed to ssd_process_host / ssd_process_depth_host.  hipHostMalloc places it on the
 * NUMA node nearest to the calling thread's current device (the runtime's default policy), so on a two-socket node allocate it from
 * the thread that feeds that GPU, after ssd_bind_thread_to_device. */
int ssd_host_alloc(size_t bytes, void **ptr);
int ssd_host_free(void *ptr);

/* plain device-memory helpers so that hosts without a HIP binding can stage frames */
int ssd_device_count(void);
int ssd_device_alloc(int device, size_t bytes, void **d_ptr);
int ssd_device_free(int device, void *d_ptr);
int ssd_device_upload(int device, void *d_dst, const void *src, size_t bytes);
int ssd_device_download(int device, void *dst, const void *d_src, size_t bytes);
int ssd_device_sync(int device);

/* ---- identity and locality of a device (hosts with several GPUs and sockets; SURVEY.md section 8(e): one host thread per GPU) ----
 * pci_bus_id "dddd:bb:dd.f" and uuid identify the physical GPU (a scaling run proves its N devices distinct with them);
 * numa_node / cpu_list = the NUMA node the GPU hangs off and that node's CPUs as sysfs names them
 * (/sys/bus/pci/devices/<id>/numa_node, local_cpulist); -1 / "" where the platform does not say. */
typedef struct
{
  char pci_bus_id[32];
  char uuid[40];
  int32_t numa_node;
  int32_t n_local_cpus;
  char cpu_list[256];
} ssd_device_info;
int ssd_device_info_get(int device, ssd_device_info *out);
/* Binds the CALLING host thread to the CPUs local to `device` (sched_setaffinity on the thread), so that the thread that feeds
 * a GPU — and the pinned staging memory it allocates afterwards, placed by first touch — sit on the GPU's socket: what the
 * host-fed path needs on a two-socket 8-GPU node (frames resident in HBM do not care).  Returns the number of CPUs bound,
 * 0 when the platform names none (affinity left as it was), or a negative SSD_E_* code. */
int ssd_bind_thread_to_device(int device);

#ifdef __cplusplus
}
#endif

#endif /* SSD_HIP_H_ */
