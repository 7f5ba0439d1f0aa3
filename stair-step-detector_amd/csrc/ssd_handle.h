/*
 * ssd_handle.h — the state behind an ssd_handle (private to the library; the test-hook library reads it to copy
 * a frame's raw device state out).
 */
#ifndef SSD_HANDLE_H_
#define SSD_HANDLE_H_

#include "ssd_device.h"
#include "ssd_owned.h"
#include "ssd_chunks.h"                     /* ssd_tuning: the launch-geometry constants of a handle, beside the chunk rules that read them */
#include <cstring>
#include <string>
#include <vector>

namespace ssd { struct GroundPrior; }          /* ssd_ground.h */
namespace ssd { struct PoseTarget; }           /* ssd_pose.h */

/* The events around an optional pass (k_labels, k_riser_labels, k_surface_moments) of the timed enqueues: a ring of SSD_TIMING_SLOTS pairs,
 * all of them or none, and whether the enqueue of a slot ran the pass between its pair */
struct ssd_timed_pass
{
  std::vector<ssd::Event> ev;               /* SSD_TIMING_SLOTS x 2, or empty */
  bool timed[SSD_TIMING_SLOTS] = {};
  hipError_t make() { return ev.empty() ? ssd::make_events(ev, 2 * SSD_TIMING_SLOTS, hipEventDefault) : hipSuccess; }   /* on first use */
  void begin(int slot, hipStream_t s) { (void)hipEventRecord(ev[2 * slot], s); }
  void end(int slot, hipStream_t s) { (void)hipEventRecord(ev[2 * slot + 1], s); }
  /* the pass's milliseconds at that slot, once it has run; *ms left as it is where the slot's enqueue did not time the pass */
  hipError_t elapsed(int slot, float *ms)
  {
    if(!timed[slot] || ev.empty())
      return hipSuccess;
    const hipError_t e = hipEventSynchronize(ev[2 * slot + 1]);
    return e != hipSuccess ? e : hipEventElapsedTime(ms, ev[2 * slot], ev[2 * slot + 1]);
  }
};

/* A pass the handle keeps in call order (the ground fit, the trimmed refit, the clearance pass, the tread grid: DESIGN.md section 7o):
 * the event behind the last call and the stream it ran on, so that a call on another stream goes behind it and the last call's event
 * covers every call so far; and, for the passes that time, the events around the last call's timed span.  Only pass_open, pass_start,
 * pass_close, pass_wait and pass_time (ssd_capi.hip) touch it */
struct ssd_ordered_pass
{
  ssd::Event done;                          /* behind the last call, made on the first one */
  hipStream_t lastStream = nullptr;         /* the stream of the last call (a switch is ordered by `done`) */
  bool haveLast = false;                    /* there was one */
  std::vector<ssd::Event> ev;               /* both or none: around the timed span of a timed call, made on the first one */
  bool timed = false;                       /* the last call was timed */
};

/* The per-frame (or per-group) records of a stand-alone frame pass: F of them on the device, where the kernel
 * adds into them, and pinned, where the call's last step copies them; the pass's order record; how many the last call wrote.  Made on the
 * pass's first call; one set, used in call order, nothing of the lanes is touched.  Only records_prepare, records_zero, records_finish,
 * records_wait and records_fetch (ssd_capi.hip) touch it */
template<typename Rec>
struct ssd_pass_records
{
  ssd::DeviceBuf<Rec> d;
  ssd::PinnedBuf<Rec> h;
  ssd_ordered_pass pass;
  int count = 0;
};

/* A table the caller's arguments are restated into on the pinned side and sent to the device during the call (section 7u): the event lies
 * behind the copy, and the next call waits for it before it rewrites the pinned side.  Only table_prepare, table_wait and table_send
 * (ssd_capi.hip) touch the event */
template<typename T>
struct ssd_upload_table
{
  ssd::DeviceBuf<T> d;
  ssd::PinnedBuf<T> h;
  ssd::Event copied;
  bool sent = false;                        /* the event has been recorded */
};

/* One complete workspace of a handle: everything a batch in flight owns on the device.  A handle has `depth` of them
 * (ssd_config::batches_in_flight); successive enqueues take them in turn, each on the lane's own stream, so that the launches
 * of one batch fill the gaps the one-block-per-frame kernels of the others leave. */
struct ssd_lane
{
  ssd::DeviceBuf<ssd::FrameState> dState;
  ssd::DeviceBuf<unsigned long long> dStepImg;
  ssd::DeviceBuf<unsigned long long> dGroundImg;
  ssd::DeviceBuf<int> dFallback;            /* single pass: kFallbackList + F ints: frames listed for k_raster, frames without step plateaus, the list */
  ssd::DeviceBuf<unsigned long long> dPlaneImg;   /* single pass: [F][kMaxPlanes] bit images, one per candidate height bin (null: the handle never runs it) */
  uint2 *dTileMasks = nullptr;             /* per cell (64 points): which groups of 4 height bins occur; K1 -> K2, K4, K6 */
  ssd::DeviceBuf<uint2> dTileMasksBase;    /* the allocation dTileMasks lies in (the tools' placement hooks put the records elsewhere in a larger one) */
  size_t recordSlack = 0;                   /* bytes of that allocation beyond the records (0 unless a tools hook allocated it) */
  ssd::Stream stream;                       /* the lane's own stream (depth > 1 only; depth 1 runs on the caller's stream) */
  ssd::Event in;                            /* recorded on the caller's stream at the enqueue: the lane's work starts behind it */
  ssd::Event done;                          /* recorded behind the lane's last enqueue */
  hipStream_t lastStream = nullptr;         /* depth 1: the stream of the previous call (a switch is ordered by `done`) */
  bool haveLast = false;
  /* cameras batches (ssd_enqueue_cameras): the batch's index frame -> camera, F ints each, made on the lane's first such batch */
  ssd::DeviceBuf<int> dCamIndex;
  ssd::PinnedBuf<int> hCamIndex;            /* pinned: the caller's array is copied here during the call */
  ssd::Event camCopied;                     /* behind the copy pinned -> device: the slot may be written again */
  bool stepImagesDirty = false, groundImageDirty = false;   /* a partial run rastered without the stage that consumes (and clears) the bits */
  int dirtyFrames = 0;                      /* leading FrameStates whose K1 accumulators may be non-zero (k_peaks clears them) */
};

constexpr int kMaxLanes = 8;

struct ssd_handle
{
  int device = 0;
  ssd_config cfg{};
  ssd::Params P{};
  ssd_tuning tune{};
  int F = 0;                      /* max frames per batch */
  size_t imgWords = 0;            /* 64-bit words per bit image */
  int depth = 1;                  /* lanes in use */
  ssd_lane lane[kMaxLanes];
  int lastLane = 0;               /* the lane of the last enqueue (debug capture, test hooks, riser fetch read it) */
  unsigned long long laneTurn = 0;
  bool lastPinned = false;        /* the last enqueue was held in lane 0 (debug capture, risers, partial stages) */
  size_t tileMaskStride = 0;      /* cell records per frame */
  size_t recordBytes = 0;         /* one workspace's cell records */
  ssd::DeviceBuf<float> dDepthMaps;         /* xmap[W] then ymap[H] (ssd_set_intrinsics) */
  ssd_intrinsics intr{};
  bool haveIntr = false;
  /* result slots (max(2, depth)), used in turn by the enqueues that run the last stage: the device -> pinned-host copy of
   * a batch's results is part of its enqueue, so that the next batches can be enqueued before the results are read */
  int nSlots = 2;
  ssd::DeviceBuf<ssd_frame_result> dResults;   /* nSlots x F */
  ssd::PinnedBuf<ssd_frame_result> hResults;   /* nSlots x F, pinned */
  ssd_frame_result *hResultsDev = nullptr;  /* the same memory as the kernels address it (small batches write it directly) */
  ssd::Event resultsReady[kMaxLanes];
  int resultsFrames[kMaxLanes] = {};
  int resultsLane[kMaxLanes] = {};
  unsigned long long finalCount = 0;        /* enqueues that produced results */
  ssd::DeviceBuf<ssd_frame_risers> dRisers; /* vertical faces (extension), allocated by ssd_set_risers */
  ssd::PinnedBuf<ssd_frame_risers> hRisers; /* pinned */
  /* ssd_process_host / ssd_process_depth_host: two device staging buffers, a copy and a compute stream (ssd_capi.hip) */
  ssd::DeviceBuf<void> ingestBuf[2];
  size_t ingestCap = 0;                     /* bytes per buffer */
  ssd::Stream ingestCopy, ingestCompute;
  ssd::Stream ingestCopy2;                  /* the second half of a large slice: two copy engines (round 6) */
  ssd::Event ingestCopied[2], ingestConsumed[2];
  ssd::Event ingestCopied2[2];
  /* risers of a host-fed batch, slice by slice (the device buffer holds one enqueue's) */
  ssd::PinnedBuf<ssd_frame_risers> hRisersBatch;   /* pinned */
  int hRisersBatchCap = 0, hRisersBatchFrames = 0;
  /* riser moments (ssd_set_riser_moments): made on the first enable, so a handle that never asks holds none of
   * them.  Single like the riser buffer (enqueues with risers on all run in the first workspace); a host-fed batch collects them slice
   * by slice as hRisersBatch does */
  bool riserMoments = false;
  ssd::DeviceBuf<ssd_frame_moments> dRiserMoments;   /* F records */
  ssd::PinnedBuf<ssd_frame_moments> hRiserMoments;   /* pinned */
  ssd::PinnedBuf<ssd_frame_moments> hRiserMomentsBatch;   /* pinned */
  int hRiserMomentsBatchCap = 0, hRiserMomentsBatchFrames = 0;
  int riserMomentsFrames = 0;               /* frames whose riser moments the last enqueue gathered (0: none) */
  /* riser labels (ssd_set_riser_labels): a switch and the events around k_riser_labels of a timed enqueue, made on
   * the first enable; no buffer - the kernel writes into the caller's labels */
  bool riserLabels = false;
  ssd_timed_pass riserLabelsPass;
  ssd::DeviceBuf<ssd::DebugFrame> dDebug;
  ssd::DeviceBuf<unsigned long long> dDebugImg;
  int debug = 0;                  /* 0 off, 1 records + images (the whole ground image is rastered for it), 2 records only */
  int lastFrames = 0;
  /* single pass (k_hist rasters the step plateaus itself): -1 = whenever a call qualifies (whole pipeline, a batch of at least
   * kSinglePassMinPoints points, vertex input, geometry), 0 = never, 1 = whenever the geometry allows; sabotage: k_predict's (test
   * hooks set both) */
  int singlePassMode = -1, singlePassSabotage = 0;
  int planePool = 0;               /* planes k_predict may hand out per batch (plane_pool_size(F), what each workspace holds; a test hook lowers it) */
  bool lastSinglePass = false;    /* the last enqueue ran it */
  ssd::PinnedBuf<int> hFallback;  /* pinned, two per result slot: frames of that batch k_raster had to do, frames without step plateaus (copied with the results) */
  int resultsFallback[kMaxLanes] = {};      /* -1: that slot's batch ran two passes; 0: count on its way; 1: seen by ssd_fetch_back */
  int singlePassBackoff = 0;      /* qualifying batches still to run two passes after a batch the predictor did not cover */
  size_t bytes = 0;               /* what ssd_workspace_bytes reports: the ledger of the buffers allocated with it (ssd_owned.h) */
  /* per-stage timing: a ring of event sets, one per enqueue, so that a timed loop never has to synchronise */
  bool timing = false;
  std::vector<ssd::Event> ev;     /* kTimingSlots x 8 */
  std::vector<ssd::Event> evPredict;   /* SSD_TIMING_SLOTS, made with ev: recorded in front of k_predict (single-pass enqueues) */
  bool predictTimed[SSD_TIMING_SLOTS] = {};
  /* per-pixel labels (ssd_enqueue_labels & co.): made on first use, so a handle that never labels holds none of them */
  ssd_timed_pass labelsPass;                /* around k_labels of a timed enqueue */
  ssd::DeviceBuf<unsigned char> labelStage[2];   /* ssd_process_*_host_labels: a slice's labels, double-buffered */
  size_t labelStageCap = 0;                 /* bytes per buffer */
  ssd::Stream labelsCopy;                   /* their copies to the host */
  ssd::Event labelsCopied[2];
  /* surface moments (ssd_enqueue_surface_moments & co.): the events around k_surface_moments of a timed enqueue, made on the first one;
   * the host entry point stages a slice's records in labelStage and copies them out on labelsCopy, as labels are */
  ssd_timed_pass surfacePass;
  unsigned long long enqueueCount = 0;
  unsigned long long timedFrom = 0;
  /* the camera table (ssd_set_cameras; empty: none).  camParams are make_params()' as they were made; the device records also
   * carry what a call decides for the whole handle (debug capture's groundFull, the riser settings): camCallKey is what the
   * records on the device were made for, and an enqueue that finds another uploads them again behind the batches in flight */
  std::vector<ssd::Params> camParams;
  std::vector<unsigned char> camHasIntr;
  std::vector<float> camDepthUnits;
  ssd::DeviceBuf<ssd::CameraRec> dCams;
  ssd::DeviceBuf<float> dCamMaps;           /* per camera xmap[W] then ymap[H] */
  bool camsNeedChecks = false;              /* some camera needs_checks(): its batches run the CHECKS instantiations */
  unsigned long long camCallKey = ~0ull;
  double camCallTol = 0.0;
  /* the stand-alone frame passes, each made on its first call, so a handle that never runs one holds nothing of it.
   * The ground fit (section 7c): a record per frame (the kernel's kGroundSums int64), never timed; the priors, F of them (the pinned sides of
   * this pass alone are not counted as workspace) */
  ssd_pass_records<ssd_ground_moments> ground;
  ssd_upload_table<ssd::GroundPrior> groundPriors;
  std::vector<ssd_calibration> groundPriorCal;   /* the last call's priors, one or one per frame: what ssd_fetch_ground_fit solves against */
  /* the trimmed surface refit (ssd_enqueue_surface_refit; ssd_enqueue_cameras_surface_refit, section 7h).  What the
   * last enqueue was, so that a refit can be held to it: wholeKind 0 = none / a partial run / a failed one / one withdrawn by
   * ssd_set_intrinsics (kind 1) or ssd_set_cameras (kind 2), 1 = a whole run under the handle's calibration, 2 = a cameras batch (its
   * index stays in its workspace's dCamIndex until the next cameras batch takes that workspace) */
  int wholeKind = 0;
  bool wholeDepth = false;                  /* its input was 16-bit depth */
  const void *wholeFrames = nullptr;        /* its frames and their stride */
  size_t wholeStride = 0;
  const ssd_frame_result *wholeResults = nullptr;   /* its result records as the kernels address them (the slot k_final wrote) */
  /* the gates of a call, made on the first one, so a handle that never refits holds none of them.  One set, like the ground fit's */
  ssd_upload_table<ssd_frame_gates> refitGates;   /* F; the caller's gates are copied through it, or k_surface_gates writes the device side */
  ssd_ordered_pass refitPass;              /* a switch of streams is ordered by it: the device gates are single */
  /* the camera fold (ssd_enqueue_cameras_surface_refit_folded, ssd_process_host_cameras_drift): SSD_MAX_CAMERAS
   * records, made on the first call of either.  One set: the refit orders its users as it orders the device gates' */
  ssd::DeviceBuf<ssd_camera_fold> dCamFold;
  /* the tread clearance pass (ssd_enqueue_clearance): events only, made on the first call - the pass writes the
   * caller's buffers and owns none.  Passes on different streams are ordered by clearPass, so that the last one's event covers all */
  ssd_ordered_pass clearPass;
  /* the tread grid pass (ssd_enqueue_tread_grid): events only, as the clearance pass's, made on the first call */
  ssd_ordered_pass gridPass;
  /* ssd_process_host_tread_grid: a slice's records where the label staging buffers do not hold them (a record is 52.5 KB, more than
   * the width * height bytes of a small frame that those are sized by); made on first use, not counted as workspace like those */
  ssd::DeviceBuf<ssd_frame_tread_grid> gridStage;
  int gridStageFrames = 0;
  /* the stair map pass (ssd_enqueue_stair_map): the caller's maps (SSD_MAX_STAIR_MAPS records) and the batch's index
   * frame -> map (F ints), made on the first call and counted as workspace.  One set, like the refit's gates: mapPass orders the passes
   * that read it */
  ssd_upload_table<ssd_stair_map> stairMaps;
  ssd_upload_table<int> mapIndex;
  ssd_ordered_pass mapPass;
  /* ssd_process_host_stair_map: the records its slices accumulate into (SSD_MAX_STAIR_MAPS of them), made on its first call; staging
   * like gridStage, not counted as workspace */
  ssd::DeviceBuf<ssd_frame_tread_grid> mapStage;
  /* the stair pose (section 7q): a record per frame; the call's targets as the kernel reads them (SSD_MAX_STAIR_MAPS) and its index
   * frame -> target (F ints); all counted as workspace */
  ssd_pass_records<ssd_stair_pose_moments> pose;
  ssd_upload_table<ssd::PoseTarget> poseTargetsUp;
  ssd_upload_table<int> poseIndexUp;
  std::vector<ssd_stair_pose_target> poseTargets;   /* the last call's targets and index: what ssd_fetch_stair_pose folds and solves against */
  std::vector<int> poseIndex;
  /* the depth fusion (section 7s): a record per group; the depth edge filter (section 7t): a record per frame; counted as workspace */
  ssd_pass_records<ssd_depth_fuse_stats> fuse;
  ssd_pass_records<ssd_depth_edge_stats> edge;
  /* ssd_process_depth_host_fused, ssd_process_depth_host_edges: a slice's fused or filtered frames, which its detection reads (section 7u:
   * why one buffer does for both); made on first use, staging like gridStage, not counted as workspace */
  ssd::DeviceBuf<unsigned char> depthStage;
  size_t depthStageCap = 0;
  /* the depth warp (section 7v): a record per frame and the call's views, one per frame; counted as workspace */
  ssd_pass_records<ssd_depth_warp_stats> warp;
  ssd_upload_table<ssd_depth_warp_view> warpViews;
  /* ssd_process_depth_host_warp_fused: a slice's warped frames, which its fusion reads into depthStage; staging like depthStage, not
   * counted as workspace */
  ssd::DeviceBuf<unsigned char> warpStage;
  size_t warpStageCap = 0;
  /* the depth fill (section 7w): a record per frame; counted as workspace */
  ssd_pass_records<ssd_depth_fill_stats> fill;
  /* ssd_process_depth_host_warp_fill_fused: a slice's filled frames between warpStage and the fusion (the fill cannot run in place);
   * managed exactly like warpStage, not counted as workspace */
  ssd::DeviceBuf<unsigned char> fillStage;
  size_t fillStageCap = 0;
};

/* The single pass's planes - dPlaneImg and dFallback of every workspace and the pinned hFallback, zeroed - for ALL workspaces of the
 * handle or for none (ssd_create, ssd_set_single_pass, the test hook ssd_test_single_pass; here because the hook library does not link
 * the product).  cap: what the planes of all workspaces together may take (the caller's reading of SSD_MAX_PLANE_BYTES, ~0ull: no
 * bound); a handle that would cross it counts as one whose allocation failed.  counted: the planes go into `bytes` (the hook's do
 * not).  On failure the handle is as it was, and `why` says what did not fit. */
inline hipError_t planes_make(ssd_handle *h, unsigned long long cap, bool counted, std::string &why)
{
  const size_t planeBytes = static_cast<size_t>(ssd::plane_pool_size(h->F, h->P.nPoints)) * h->imgWords * 8;
  const size_t listBytes = sizeof(int) * (ssd::kFallbackList + static_cast<size_t>(h->F)), counterBytes = sizeof(int) * 2 * kMaxLanes;
  if(static_cast<unsigned long long>(h->depth) * planeBytes > cap)
  {
    why = "SSD_MAX_PLANE_BYTES = " + std::to_string(cap) + " < " + std::to_string(static_cast<unsigned long long>(h->depth) * planeBytes);
    return hipErrorOutOfMemory;
  }
  ssd::DeviceBuf<unsigned long long> planes[kMaxLanes];
  ssd::DeviceBuf<int> lists[kMaxLanes];
  ssd::PinnedBuf<int> counters;
  hipError_t e = hipSuccess;
  for(int k = 0; k < h->depth && e == hipSuccess; k++)
  {
    e = planes[k].alloc(planeBytes, counted ? &h->bytes : nullptr);
    if(e == hipSuccess) e = lists[k].alloc(listBytes);
    if(e == hipSuccess) e = hipMemset(planes[k], 0, planeBytes);
    if(e == hipSuccess) e = hipMemset(lists[k], 0, listBytes);
    if(e != hipSuccess)
      why = std::string("hipMalloc of ") + std::to_string(planeBytes) + " bytes for workspace " + std::to_string(k) + ": " + hipGetErrorString(e);
  }
  if(e == hipSuccess && !h->hFallback && (e = counters.alloc(counterBytes)) != hipSuccess)
    why = "hipHostMalloc of the work lists' counters failed";
  if(e != hipSuccess)
  {
    (void)hipGetLastError();                   /* the failed allocation's error is not the handle's */
    return e;
  }
  if(counters)
  {
    std::memset(counters, 0, counterBytes);
    h->hFallback = std::move(counters);
  }
  for(int k = 0; k < h->depth; k++)
  {
    h->lane[k].dPlaneImg = std::move(planes[k]);
    h->lane[k].dFallback = std::move(lists[k]);
  }
  return hipSuccess;
}

/* ... and given back: every workspace's (hFallback stays: the counts of batches not yet fetched are read from it) */
inline void planes_drop(ssd_handle *h)
{
  for(ssd_lane &L : h->lane)
  {
    L.dPlaneImg.reset();
    L.dFallback.reset();
  }
}

#endif /* SSD_HANDLE_H_ */
