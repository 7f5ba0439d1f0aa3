/*
 * ssd_capi.hip — the half of the C ABI of libssd_hip.so that runs on a handle (see include/ssd_hip.h for the
 * reference interface each entry point replaces).  Owns the device workspace,
 * sequences the kernels of ssd_kernels.hip on one HIP stream, never touches
 * the CPU oracle: if no HIP device is present every compute entry fails with
 * SSD_E_NODEVICE.  The entry points that need no handle, no stream and no HIP
 * call - configuration, calibrations, host statements, solvers, folds - are
 * ssd_host.cpp's, plain C++; ssd_host.h holds what the two files share.  Those that
 * call HIP without a handle are ssd_capi_device.cpp's; ssd_capi.h holds HIP_TRY and
 * hip_fail for both, and the layers of this file.
 */
#include "ssd_launch.h"
#include "ssd_handle.h"
#include "ssd_chunks.h"
#include "ssd_capi.h"
#include "ssd_prexy.h"
#include "ssd_ground.h"
#include "ssd_pose.h"
#include "ssd_fuse.h"
#include "ssd_edges.h"
#include "ssd_warp.h"
#include "ssd_fill.h"
#include "ssd_refit.h"
#include "ssd_clearance.h"
#include "ssd_treadgrid.h"
#include "ssd_solve.h"
#include "ssd_fold.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

using namespace ssd;

namespace
{

/* the riser pass's records and the riser moments': a zeroed device buffer (counted) and its pinned mirror, both or neither */
template<typename T>
hipError_t make_records(ssd_handle *h, DeviceBuf<T> &dev, PinnedBuf<T> &pinned, size_t bytes)
{
  DeviceBuf<T> d;
  PinnedBuf<T> p;
  hipError_t e = d.alloc(bytes, &h->bytes);
  if(e == hipSuccess) e = hipMemset(d, 0, bytes);
  if(e == hipSuccess) e = p.alloc(bytes);
  if(e != hipSuccess)
    return e;
  dev = std::move(d);
  pinned = std::move(p);
  return hipSuccess;
}

/* a pinned buffer of one record per frame of a host batch (the device buffer holds one enqueue's), grown to nframes */
template<typename T>
int grow_pinned_batch(ssd_handle *h, PinnedBuf<T> &buf, int &cap, int nframes)
{
  if(cap >= nframes)
    return SSD_OK;
  HIP_TRY(hipStreamSynchronize(h->ingestCompute));
  buf.reset();
  cap = 0;
  HIP_TRY(buf.alloc(sizeof(T) * static_cast<size_t>(nframes)));
  cap = nframes;
  return SSD_OK;
}

#ifdef SSD_TUNING
/* tools builds only (see ssd_tuning, ssd_handle.h): overrides from the environment, read once per handle */
int env_int(const char *name, int dflt)
{
  const char *v = std::getenv(name);
  return v && *v ? std::atoi(v) : dflt;
}
void tuning_from_env(ssd_tuning &t)
{
  t.chunkPoints = env_int("SSD_CHUNK_POINTS", t.chunkPoints);
  t.targetBlocks = env_int("SSD_TARGET_BLOCKS", t.targetBlocks);
  t.k1BlocksPerFrame = env_int("SSD_K1_BLOCKS_PER_FRAME", t.k1BlocksPerFrame);
  t.k24MinBlocks = env_int("SSD_K24_MIN_BLOCKS", t.k24MinBlocks);
  t.k24TallBlocks = env_int("SSD_K24_TALL_BLOCKS", t.k24TallBlocks);
  t.k2ChunkTiles = env_int("SSD_K2_CHUNK_TILES", t.k2ChunkTiles);
  t.k4ChunkTiles = env_int("SSD_K4_CHUNK_TILES", t.k4ChunkTiles);
  t.winShift = env_int("SSD_WIN_SHIFT", 0);
  t.winShiftGround = env_int("SSD_WIN_SHIFT_G", 0);
  t.recordPad = env_int("SSD_RECORD_PAD", t.recordPad);
  t.fuseGroupFastest = env_int("SSD_FUSE_GROUP_FASTEST", t.fuseGroupFastest);
}
#endif

/* ssd_config::batches_in_flight = 0 resolves to ONE workspace: every call on the caller's stream, in stream order — the contract
 * every caller may rely on without reading further (enqueue, then refill the frames on the same stream: ordered).  Overlap is
 * opt-in (round 4; round 3 resolved 0 to three workspaces for batches, which silently took that order away): a caller that
 * enqueues ahead of its fetches asks for kOverlapDepth and keeps its frames untouched until their results were fetched.
 * XGA, frames/s with 1 / 2 / 3 / 4 / 5 / 6 / 8 batches in flight (tools/depths.py, profiles/r03_depths.json: three and six sit
 * better than four and five; six buys 2-5 % over three for twice the memory):
 *   1024 frames per call 272 k / 290 k / 301 k / 294 k / 298 k / 307 k / 310 k      256: 237 k / 286 k / 306 k / 295 k / 303 k / 314 k / 306 k
 *     64: 188 k / 248 k / 270 k / 251 k / 268 k / 284 k / 270 k                      32: 140 k / 225 k / 253 k / 215 k / 244 k / 256 k / 246 k
 *     16:  94 k / 165 k / 214 k / 170 k / 203 k / 228 k / 206 k                       8:  59 k / 107 k / 140 k / 114 k / 130 k / 144 k / 135 k
 * bench.py and detect-stairs-amd ask for SSD_BATCHES_IN_FLIGHT_THROUGHPUT (ssd_hip.h) explicitly. */
constexpr int kOverlapDepth = SSD_BATCHES_IN_FLIGHT_THROUGHPUT;

} // namespace


extern "C"
{

static int make_params(const ssd_config &c, const ssd_calibration &k, Params &P)
{
  /* height: a pixel key's row field is 13 bits and "inside the wave's LDS window" is one subtraction on the key
   * (ssd_kernels.hip, window_hit): a window anchored within its own height (<= 128 rows) of row 8192 would take pixels of
   * the next image slot for its own */
  if(c.width <= 0 || c.height <= 0 || c.width > 8192 || c.height > 8064)
    return fail(SSD_E_ARG, "config: resolution out of range (width <= 8192, height <= 8064)");
  if(!(c.x_max > c.x_min) || !(c.y_max > c.y_min) || !(c.z_max > c.z_min) || !(c.height_interval > 0))
    return fail(SSD_E_ARG, "config: empty measuring range");
  P.W = c.width; P.H = c.height;
  P.W64 = (c.width + 63) / 64;
  P.nPoints = c.width * c.height;
  for(int i = 0; i < 9; i++) P.pt.a[i] = k.a[i];
  for(int i = 0; i < 3; i++) P.pt.b[i] = k.b[i];
  for(int i = 0; i < 4; i++) P.r2[i] = k.r2[i];
  P.t2[0] = k.t2[0]; P.t2[1] = k.t2[1];
  P.worldZ = k.world_z;
  P.xMin = c.x_min; P.xMax = c.x_max; P.yMin = c.y_min; P.yMax = c.y_max; P.zMin = c.z_min; P.zMax = c.z_max;
  /* ProcessingConfiguration / Projection2D, pointcloud.cpp:60-106 */
  P.pt.recip = 1.0 / c.height_interval;
  P.minHeight = static_cast<uint16_t>((c.min_height_above_ground - c.z_min) * P.pt.recip);
  P.minImgYExtent = static_cast<int>(c.min_step_depth * c.height / (c.y_max - c.y_min));
  P.xToImage = c.width / (c.x_max - c.x_min);
  P.yToImage = c.height / (c.y_max - c.y_min);
  P.xToWorld = 1 / P.xToImage;
  P.yToWorld = 1 / P.yToImage;
  P.xyRatio = P.xToImage / P.yToImage;
  const size_t nBins = static_cast<size_t>((c.z_max - c.z_min) * P.pt.recip) + 1;   /* pointcloud.cpp:196 */
  if(nBins < 3 || nBins > SSD_MAX_BINS)
    return fail(SSD_E_ARG, "config: histogram needs 3.." + std::to_string(SSD_MAX_BINS) + " bins");
  P.nBins = static_cast<int>(nBins);
  /* mean z is accumulated as a sum of round(z * 2^40) in int64 through a magic-constant add that is exact only for
   * |z| < 2048 (ssd_kernels.hip, z_plus_magic_bits), and the sum over a frame's points must stay below 2^63 */
  {
    const double zAbs = std::fmax(std::fabs(c.z_min), std::fabs(c.z_max));
    if(!(zAbs < 2048.0) || !(zAbs * static_cast<double>(c.width) * static_cast<double>(c.height) < 8388608.0))
      return fail(SSD_E_ARG, "config: max(|z_min|, |z_max|) must be < 2048 m and max|z| * width * height < 2^23 (fixed-point mean z)");
  }
  if(c.max_step_plateaus < 1 || c.max_step_plateaus > SSD_MAX_STEP_IMAGES)
    return fail(SSD_E_ARG, "config: max_step_plateaus out of range");
  P.maxStepImages = c.max_step_plateaus;
  P.pt.xMin = c.x_min; P.pt.xMax = c.x_max; P.pt.yMin = c.y_min; P.pt.yMax = c.y_max; P.pt.zMin = c.z_min; P.pt.zMax = c.z_max;
  P.pt.boxX = 256.0 / (c.x_max - c.x_min);
  P.pt.boxY = 256.0 / (c.y_max - c.y_min);
  P.pt.nPoints = P.nPoints;
  P.pt.nBins = P.nBins;
  P.pre = make_pre_xy(P.pt);                  /* the single-precision pre-filter's constants (ssd_prexy.h; used by ssd_prefilter.h) */
  P.px.xToImage = P.xToImage; P.px.yToImage = P.yToImage;
  P.px.W = P.W; P.px.H = P.H; P.px.W64 = P.W64;
  P.px.maxStepImages = P.maxStepImages;
  P.px.cellCols = (c.width + kCellHost / 2) / kCellHost > 0 ? (c.width + kCellHost / 2) / kCellHost : 1;
  make_pre_pixel(P.pt, P.pre, P.px);          /* K1's candidates: the pixel in single precision first (ssd_prexy.h) */
  P.risers = 0; P.riserMinSupport = 1; P.riserTol = 0.0;
  P.heightInterval = c.height_interval;
  /* Shape of the waves' write-combining windows (ssd_kernels.hip, WaveWindow).  A wave walks down one cell column —
   * 64 camera pixels wide, which is 60 .. 110 pixels of the top-down image depending on the range — so the window is
   * tall and narrow: 64 rows x 4 words up to XGA, 32 rows x 8 words above (measured, tools/exp.sh: XGA raster 1.52 ms
   * with 32 x 8, 1.00 ms with 64 x 4, 2.23 ms with 16 x 16; FHD stress 1.04 ms with 32 x 8, 1.24 ms with 64 x 4).  The
   * ground image of k_inquad is denser (the camera looks steeply down on it): 32 x 8.  When a camera row is not a
   * whole number of cells the columns drift sideways from row to row: a window as wide as the image row then. */
  P.px.winShift = P.W64 <= 16 ? 2 : 3;
  P.px.winShiftGround = 3;
  if(c.width % kCellHost != 0 && P.W64 <= 32)
  {
    while((1 << P.px.winShift) < P.W64)
      P.px.winShift++;
    P.px.winShiftGround = P.px.winShift;
  }
  if((c.width - 1) / 25 + 2 > SSD_MAX_SCANS)
    return fail(SSD_E_ARG, "config: width needs more scan columns than SSD_MAX_SCANS");
  /* k_outline keeps one vertical-edge probe row per 10 image rows (detectEdge, segmentation.cpp:681-706) in LDS arrays of
   * SSD_MAX_EDGE_PTS; the reference has no cap, so a taller image could give a step a different vertical edge */
  if((c.height - 1) / 10 + 1 > SSD_MAX_EDGE_PTS)
    return fail(SSD_E_ARG, "config: height needs more vertical-edge probe rows than SSD_MAX_EDGE_PTS");
  return SSD_OK;
}

int ssd_create(const ssd_config *cfg, const ssd_calibration *cal, int device, ssd_handle **out)
{
  if(!cfg || !cal || !out)
    return fail(SSD_E_ARG, "ssd_create: null argument");
  *out = nullptr;
  if(cfg->max_frames_per_batch < 1 || cfg->max_frames_per_batch > 65535)
    return fail(SSD_E_ARG, "ssd_create: max_frames_per_batch out of range");
  int depth = cfg->batches_in_flight;
  if(depth < 0 || depth > kMaxLanes)
    return fail(SSD_E_ARG, "ssd_create: batches_in_flight must be 0 (automatic) .. " + std::to_string(kMaxLanes));
  if(depth == 0)
    depth = 1;                                  /* strict stream order unless the caller asks for overlap (see above) */
  static_assert(kOverlapDepth >= 2 && kOverlapDepth <= kMaxLanes, "SSD_BATCHES_IN_FLIGHT_THROUGHPUT out of range");
  Params P{};
  const int rc = make_params(*cfg, *cal, P);
  if(rc)
    return rc;
  const int nDev = ssd_device_count();
  if(nDev <= 0)
    return fail(SSD_E_NODEVICE, "ssd_create: no HIP device (the HIP path is mandatory; there is no CPU fallback)");
  if(device < 0 || device >= nDev)
    return fail(SSD_E_ARG, "ssd_create: device index out of range");
  HIP_TRY(hipSetDevice(device));

  ssd_handle *h = new ssd_handle();
  h->device = device;
  h->cfg = *cfg;
  h->cfg.batches_in_flight = depth;
  h->P = P;
#ifdef SSD_TUNING
  tuning_from_env(h->tune);
  if(h->tune.winShift >= 1 && h->tune.winShift <= 6) h->P.px.winShift = h->tune.winShift;
  if(h->tune.winShiftGround >= 1 && h->tune.winShiftGround <= 6) h->P.px.winShiftGround = h->tune.winShiftGround;
#endif
  h->F = cfg->max_frames_per_batch;
  h->depth = depth;
  h->nSlots = depth > 2 ? depth : 2;
  h->imgWords = static_cast<size_t>(P.H) * P.W64;
  const size_t stepBytes = static_cast<size_t>(h->F) * P.maxStepImages * h->imgWords * 8;
  const size_t groundBytes = static_cast<size_t>(h->F) * h->imgWords * 8;
  /* the planes of the single pass, for handles whose batches can qualify (ssd_launch.h) */
  const size_t planeBytes = single_pass_geometry(P.W, P.H) && single_pass_batch(h->F, P.nPoints)
                            ? static_cast<size_t>(plane_pool_size(h->F, h->P.nPoints)) * h->imgWords * 8 : 0;
  h->planePool = static_cast<int>(plane_pool_size(h->F, h->P.nPoints));
#define HIP_TRY_H(expr)                                                                                 \
  do                                                                                                    \
  {                                                                                                     \
    const hipError_t e_ = (expr);                                                                       \
    if(e_ != hipSuccess)                                                                                \
    {                                                                                                   \
      ssd_destroy(h);                                                                                   \
      return hip_fail(e_, #expr ": ");                                                                  \
    }                                                                                                   \
  } while(0)
  h->tileMaskStride = (static_cast<size_t>(P.nPoints) + kTileHost - 1) / kTileHost * (kTileHost / kCellHost)      /* cell records per frame */
                      + static_cast<size_t>(h->tune.recordPad);
  const size_t maskBytes = h->tileMaskStride * sizeof(uint2) * h->F;
  h->recordBytes = maskBytes;
  for(int k = 0; k < depth; k++)
  {
    ssd_lane &L = h->lane[k];
    HIP_TRY_H(L.dState.alloc(sizeof(FrameState) * h->F, &h->bytes));
    HIP_TRY_H(L.dStepImg.alloc(stepBytes, &h->bytes));
    HIP_TRY_H(L.dGroundImg.alloc(groundBytes, &h->bytes));
    HIP_TRY_H(L.dTileMasksBase.alloc(maskBytes, &h->bytes));
    L.dTileMasks = L.dTileMasksBase;
    HIP_TRY_H(L.in.create(hipEventDisableTiming));
    HIP_TRY_H(L.done.create(hipEventDisableTiming));
    if(depth > 1)
      HIP_TRY_H(L.stream.create(hipStreamNonBlocking));
    HIP_TRY_H(hipMemset(L.dState, 0, sizeof(FrameState) * h->F));
    HIP_TRY_H(hipMemset(L.dStepImg, 0, stepBytes));
    HIP_TRY_H(hipMemset(L.dGroundImg, 0, groundBytes));
  }
  const size_t resBytes = sizeof(ssd_frame_result) * h->F * h->nSlots;
  HIP_TRY_H(h->dResults.alloc(resBytes, &h->bytes));
  HIP_TRY_H(h->hResults.alloc(resBytes));
  std::memset(h->hResults, 0, resBytes);
  HIP_TRY_H(hipHostGetDevicePointer(reinterpret_cast<void **>(&h->hResultsDev), h->hResults, 0));
  for(int k = 0; k < h->nSlots; k++)
    HIP_TRY_H(h->resultsReady[k].create(hipEventDisableTiming));
  HIP_TRY_H(hipMemset(h->dResults, 0, resBytes));
  /* The planes of the single pass are an optimisation (results are the same without them): when they do not fit beside the
   * rest - a larger batch, more workspaces, memory shared with the caller's frames - the handle gives up the planes of ALL its
   * workspaces and runs two passes, as ssd_set_single_pass(h, 0) would; it does not fail.  They are taken LAST,
   * behind everything the handle cannot do without: a device with room for the planes but not for what
   * followed them used to fail the whole handle.  SSD_MAX_PLANE_BYTES (environment) bounds what a handle may take for the planes
   * of all its workspaces together - for a GPU shared with other tenants; a workspace whose planes would cross it counts as one
   * whose allocation failed.  Why a handle has no planes is kept for ssd_last_error() (ssd_create still returns SSD_OK). */
  if(planeBytes)
  {
    unsigned long long cap = ~0ull;
    if(const char *e = std::getenv("SSD_MAX_PLANE_BYTES"))
      cap = std::strtoull(e, nullptr, 10);
    std::string why;
    if(planes_make(h, cap, true, why) != hipSuccess)
    {
      (void)fail(SSD_OK, "ssd_create: no planes for the single pass (" + why + "): the handle runs two passes");
      h->singlePassMode = 0;
    }
  }
  HIP_TRY_H(hipDeviceSynchronize());
#undef HIP_TRY_H
  *out = h;
  return SSD_OK;
}

int ssd_destroy(ssd_handle *h)
{
  if(!h)
    return SSD_OK;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();               /* nothing of this handle is in flight any more (lanes run on their own streams) */
  delete h;                                    /* every resource is a member that frees itself (ssd_owned.h) */
  return SSD_OK;
}

size_t ssd_workspace_bytes(const ssd_handle *h)
{
  return h ? h->bytes : 0;
}

int ssd_set_single_pass(ssd_handle *h, int enable)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_set_single_pass: null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());            /* the planes of batches in flight are in use */
  if(!enable)
  {
    planes_drop(h);
    h->singlePassMode = 0;
    return SSD_OK;
  }
  if(single_pass_geometry(h->P.W, h->P.H) && single_pass_batch(h->F, h->P.nPoints))
  {
    if(!h->lane[0].dPlaneImg)
    {
      unsigned long long cap = ~0ull;
      if(const char *ev = std::getenv("SSD_MAX_PLANE_BYTES"))
        cap = std::strtoull(ev, nullptr, 10);
      std::string why;
      const hipError_t e = planes_make(h, cap, true, why);
      if(e != hipSuccess)
      {
        /* asked for explicitly, so said loudly - but the handle stays whole: on two passes, with no plane of any workspace */
        h->singlePassMode = 0;
        return fail(hip_error_code(e), std::string("ssd_set_single_pass: ") + hipGetErrorString(e) + " (the handle stays on two passes)");
      }
    }
    HIP_TRY(hipDeviceSynchronize());
  }
  h->singlePassMode = -1;
  h->singlePassBackoff = 0;
  return SSD_OK;
}

int ssd_set_debug(ssd_handle *h, int enable)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_set_debug: null handle");
  HIP_TRY(hipSetDevice(h->device));
  const bool wantImages = enable != 0 && enable != 2;
  if(enable && (!h->dDebug || (wantImages && !h->dDebugImg)))
  {
    /* the records always; the image buffer (F x (images + 1) x 2 whole images) only for capture WITH images — and then both
     * or neither: a failed second allocation must not leave the first behind as "debug is set up" */
    const size_t imgBytes = static_cast<size_t>(h->F) * (h->P.maxStepImages + 1) * 2 * h->imgWords * 8;
    DeviceBuf<DebugFrame> d;
    DeviceBuf<unsigned long long> di;
    hipError_t e = h->dDebug ? hipSuccess : d.alloc(sizeof(DebugFrame) * h->F, &h->bytes);
    if(e == hipSuccess && wantImages && !h->dDebugImg)
      e = di.alloc(imgBytes, &h->bytes);
    if(e != hipSuccess)
      return hip_fail(e, "ssd_set_debug: ");
    if(d) h->dDebug = std::move(d);
    if(di) h->dDebugImg = std::move(di);
  }
  h->debug = enable == 0 ? 0 : enable == 2 ? 2 : 1;
  return SSD_OK;
}

int ssd_set_risers(ssd_handle *h, int enable, double tolerance, int min_support)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_set_risers: null handle");
  if(enable && (!(tolerance > 0.0) || tolerance > 1.0 || min_support < 1))
    return fail(SSD_E_ARG, "ssd_set_risers: tolerance must be in (0, 1] m, min_support >= 1");
  HIP_TRY(hipSetDevice(h->device));
  if(enable && (!h->dRisers || !h->hRisers))
  {
    const hipError_t e = make_records(h, h->dRisers, h->hRisers, sizeof(ssd_frame_risers) * h->F);
    if(e != hipSuccess)
      return hip_fail(e, "ssd_set_risers: ");
  }
  h->P.risers = enable ? 1 : 0;
  if(enable)
  {
    h->P.riserTol = tolerance;
    h->P.riserMinSupport = min_support;
  }
  return SSD_OK;
}

int ssd_fetch_risers(ssd_handle *h, ssd_frame_risers *out, int nframes, void *stream)
{
  if(!h || !out)
    return fail(SSD_E_ARG, "ssd_fetch_risers: null argument");
  if(!h->P.risers || !h->dRisers)
    return fail(SSD_E_ARG, "ssd_fetch_risers: call ssd_set_risers(h, 1, ...) before the enqueue");
  HIP_TRY(hipSetDevice(h->device));
  if(h->hRisersBatchFrames > 0)
  {
    /* the last call was ssd_process_host / ssd_process_depth_host: its risers were collected slice by slice */
    if(nframes < 1 || nframes > h->hRisersBatchFrames)
      return fail(SSD_E_ARG, "ssd_fetch_risers: nframes exceeds what the last call processed");
    HIP_TRY(hipStreamSynchronize(h->ingestCompute));
    std::memcpy(out, h->hRisersBatch, sizeof(ssd_frame_risers) * nframes);
    return SSD_OK;
  }
  if(nframes < 1 || nframes > h->lastFrames)
    return fail(SSD_E_ARG, "ssd_fetch_risers: nframes exceeds what the last enqueue processed");
  /* the riser buffer is single: enqueues with risers on all run in lane 0, whose `done` event covers the last one */
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipStreamWaitEvent(s, h->lane[h->lastLane].done, 0));
  HIP_TRY(hipMemcpyAsync(h->hRisers, h->dRisers, sizeof(ssd_frame_risers) * nframes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::memcpy(out, h->hRisers, sizeof(ssd_frame_risers) * nframes);
  return SSD_OK;
}

int ssd_set_riser_moments(ssd_handle *h, int enable)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_set_riser_moments: null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());            /* the batches in flight keep the kernel they were enqueued with */
  if(enable && (!h->dRiserMoments || !h->hRiserMoments))
  {
    const hipError_t e = make_records(h, h->dRiserMoments, h->hRiserMoments, sizeof(ssd_frame_moments) * h->F);
    if(e != hipSuccess)
      return hip_fail(e, "ssd_set_riser_moments: ");
  }
  h->riserMoments = enable != 0;
  return SSD_OK;
}

int ssd_fetch_riser_moments(ssd_handle *h, ssd_frame_moments *out, int nframes, void *stream)
{
  if(!h || !out)
    return fail(SSD_E_ARG, "ssd_fetch_riser_moments: null argument");
  HIP_TRY(hipSetDevice(h->device));
  if(h->hRiserMomentsBatchFrames > 0)
  {
    /* the last call was a host-fed batch: its riser moments were collected slice by slice */
    if(nframes < 1 || nframes > h->hRiserMomentsBatchFrames)
      return fail(SSD_E_ARG, "ssd_fetch_riser_moments: nframes exceeds what the last call processed");
    HIP_TRY(hipStreamSynchronize(h->ingestCompute));
    std::memcpy(out, h->hRiserMomentsBatch, sizeof(ssd_frame_moments) * nframes);
    return SSD_OK;
  }
  if(h->riserMomentsFrames < 1 || !h->dRiserMoments || !h->hRiserMoments)
    return fail(SSD_E_ARG, "ssd_fetch_riser_moments: the last pass gathered none (ssd_set_risers and ssd_set_riser_moments before the enqueue)");
  if(nframes < 1 || nframes > h->riserMomentsFrames)
    return fail(SSD_E_ARG, "ssd_fetch_riser_moments: nframes exceeds what the last enqueue processed");
  /* single like the riser buffer: enqueues with risers on all run in lane 0, whose `done` event covers the last one */
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipStreamWaitEvent(s, h->lane[h->lastLane].done, 0));
  HIP_TRY(hipMemcpyAsync(h->hRiserMoments, h->dRiserMoments, sizeof(ssd_frame_moments) * nframes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::memcpy(out, h->hRiserMoments, sizeof(ssd_frame_moments) * nframes);
  return SSD_OK;
}

static int timed_pass_make(ssd_timed_pass &pass, const char *who);

int ssd_set_riser_labels(ssd_handle *h, int enable)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_set_riser_labels: null handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());            /* the batches in flight keep the labels they were enqueued for */
  if(enable)
  {
    const int rc = timed_pass_make(h->riserLabelsPass, "hipEventCreate (riser labels): ");
    if(rc) return rc;
  }
  h->riserLabels = enable != 0;
  return SSD_OK;
}

int ssd_set_timing(ssd_handle *h, int enable)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_set_timing: null handle");
  HIP_TRY(hipSetDevice(h->device));
  if(enable && h->ev.empty())
  {
    /* the stages' events and k_predict's, all of them before anything is handed to the handle: a failure leaves it as it was (no
     * half-made set that a later call would take for complete) */
    std::vector<Event> ev, pred;
    hipError_t rc = make_events(ev, static_cast<size_t>(SSD_TIMING_SLOTS) * 8, hipEventDefault);
    if(rc != hipSuccess)
      return fail(SSD_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(rc));
    rc = make_events(pred, SSD_TIMING_SLOTS, hipEventDefault);
    if(rc != hipSuccess)
      return fail(SSD_E_HIP, "hipEventCreate (predict)");
    h->ev.swap(ev);
    h->evPredict.swap(pred);
  }
  h->timing = enable != 0;
  h->timedFrom = h->enqueueCount;
  return SSD_OK;
}

static constexpr int kDirectResultFrames = 64;
static int cameras_upload(ssd_handle *h, unsigned long long key, double tol);
/* what a call decides for the whole handle and the cameras' device records carry (ssd_handle::camCallKey) */
static unsigned long long cameras_call_key(const Params &P)
{
  return static_cast<unsigned long long>(P.px.groundFull != 0) | static_cast<unsigned long long>(P.risers != 0) << 1
         | static_cast<unsigned long long>(static_cast<unsigned int>(P.riserMinSupport)) << 2;
}

/* the events of an optional pass (ssd_timed_pass), on its first use */
static int timed_pass_make(ssd_timed_pass &pass, const char *who)
{
  const hipError_t rc = pass.make();
  return rc == hipSuccess ? SSD_OK : fail(SSD_E_HIP, std::string(who) + hipGetErrorString(rc));
}

/* The Batch (ssd_launch.h) of a call on workspace L: the frames as the kernels take them, the handle's deprojection, the workspace's
 * per-frame state.  P: the constants of the call (the handle's, or a copy the call has adjusted), which must outlive the record. */
static Batch make_batch(const ssd_handle *h, const Params &P, ssd_lane &L, const void *d_frames, size_t frame_stride_bytes, int nframes, bool depthInput,
                        hipStream_t s, const CameraSel *cams)
{
  return Batch{ P, static_cast<const float *>(d_frames), depthInput ? frame_stride_bytes / 2 : frame_stride_bytes / 4, depthInput,
                DepthSrc{ h->dDepthMaps, h->dDepthMaps ? h->dDepthMaps + P.W : nullptr, h->intr.depth_units, P.W, P.H, depth_row_magic(P.W, P.H) },
                L.dState, L.dTileMasks, h->tileMaskStride, nframes, s, cams };
}

/* ---- enqueue_impl and its steps, in the order of events ------------------------------------------------------------------------------ */

/* the argument refusals, in front of anything that touches the device or the handle */
static int check_enqueue_args(const ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, int stages, bool depthInput,
                              const uint16_t *camOf, const ssd_frame_moments *moments)
{
  if(!h || !d_xyz)
    return fail(SSD_E_ARG, "ssd_enqueue: null argument");
  if(moments && stages != SSD_STAGE_ALL)
    return fail(SSD_E_ARG, "ssd_enqueue_surface_moments: partial runs have no surface moments");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, "ssd_enqueue: nframes must be 1..max_frames_per_batch");
  const size_t frameBytes = static_cast<size_t>(h->P.nPoints) * (depthInput ? 2 : 12);
  if(depthInput)
  {
    if(!camOf && !h->haveIntr)
      return fail(SSD_E_ARG, "ssd_enqueue_depth: call ssd_set_intrinsics first");
    if(frame_stride_bytes < frameBytes || frame_stride_bytes % 8 != 0 || (reinterpret_cast<uintptr_t>(d_xyz) & 7u) != 0 || h->P.W % 4 != 0)
      return fail(SSD_E_ARG, "ssd_enqueue_depth: frames must be 8-byte aligned, stride a multiple of 8, width a multiple of 4");
  }
  else
  {
    if(frame_stride_bytes < frameBytes || frame_stride_bytes % 4 != 0)
      return fail(SSD_E_ARG, "ssd_enqueue: frame stride smaller than a frame or not a multiple of 4");
    if((reinterpret_cast<uintptr_t>(d_xyz) & 3u) != 0)
      return fail(SSD_E_ARG, "ssd_enqueue: frame pointer must be 4-byte aligned");
  }
  return SSD_OK;
}

/* The stream a call on workspace L runs on, in s: enqueue_impl's rule and follow_enter's.  A handle with one workspace runs on the
 * caller's stream (a switch of streams is ordered by the lane's event: the workspace is single-buffered).  With several, the call runs
 * on the lane's own stream behind an event recorded on the caller's stream now: it starts after the work the caller's stream holds, but
 * the caller's stream does not wait for it */
static int lane_stream(ssd_handle *h, ssd_lane &L, hipStream_t caller, hipStream_t &s)
{
  s = caller;
  if(h->depth == 1)
  {
    if(L.haveLast && s != L.lastStream)
      HIP_TRY(hipStreamWaitEvent(s, L.done, 0));
  }
  else
  {
    HIP_TRY(hipEventRecord(L.in, s));
    s = L.stream;
    HIP_TRY(hipStreamWaitEvent(s, L.in, 0));
  }
  return SSD_OK;
}

/* Which workspace, and its stream (lane_stream).  Successive batches take the workspaces in turn (ssd_fetch* / ssd_stream_wait wait for
 * them).  Debug capture, the riser pass and partial runs (ssd_enqueue_stages) own single buffers / leave state behind for the next
 * call: they stay in lane 0 (`pinned`). */
static int take_workspace(ssd_handle *h, bool pinned, hipStream_t caller, int &li, hipStream_t &s)
{
  li = h->depth == 1 || pinned ? 0 : static_cast<int>(h->laneTurn++ % static_cast<unsigned long long>(h->depth));
  const int rc = lane_stream(h, h->lane[li], caller, s);
  if(rc) return rc;
  /* the single debug / riser buffers: a pinned call after free-running ones (or the other way round) must not overtake
   * what the other lanes still hold — rare (a switch of mode), so simply wait for all of them */
  if(h->depth > 1 && pinned != h->lastPinned)
    for(int k = 0; k < h->depth; k++)
      if(k != li && h->lane[k].haveLast)
        HIP_TRY(hipStreamWaitEvent(s, h->lane[k].done, 0));
  h->lastPinned = pinned;
  return SSD_OK;
}

/* A cameras batch: the index goes through the workspace's pinned slot to its device array, on the batch's stream in front of its
 * kernels (the caller's array is free when this call returns; the slot is free once the previous copy out of it has run). */
static int send_camera_index(ssd_handle *h, ssd_lane &L, const Params &P, const uint16_t *camOf, int nframes, hipStream_t s, CameraSel &camSel)
{
  if(!h->dCams || !L.dCamIndex || !L.hCamIndex || !L.camCopied)
    return fail(SSD_E_HIP, "ssd_enqueue_cameras: the camera table is incomplete (internal)");
  if(cameras_call_key(P) != h->camCallKey || P.riserTol != h->camCallTol)
  {
    const int rcUp = cameras_upload(h, cameras_call_key(P), P.riserTol);
    if(rcUp) return rcUp;
  }
  HIP_TRY(hipEventSynchronize(L.camCopied));
  for(int i = 0; i < nframes; i++)
    L.hCamIndex[i] = camOf[i];
  HIP_TRY(hipMemcpyAsync(L.dCamIndex, L.hCamIndex, sizeof(int) * static_cast<size_t>(nframes), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(L.camCopied, s));
  camSel = CameraSel{ h->dCams, L.dCamIndex, h->camsNeedChecks };
  return SSD_OK;
}

/* The single pass: K1 rasters the step plateaus while it counts, into planes of the height bins k_predict expects them in;
 * k_peaks checks that against the complete histogram, frame by frame, and k_raster does the frames it does not cover.  Only
 * the whole pipeline in one call (the planes are set in the first stage and consumed in the fourth), only batches.  The planes
 * of a call that runs it, null for one that runs two passes. */
static unsigned long long *single_pass_planes(ssd_handle *h, ssd_lane &L, int nPoints, int stages, int nframes, bool depthInput)
{
  unsigned long long *planeImg = nullptr;
  /* (not on 16-bit depth input: K1 is bound by instruction issue there, not by the bytes a second pass would re-read - k_raster
   * reads a sixth of them -, and the raster's instructions cost K1 what k_raster took: 384.6 k against 386.8 k frames/s) */
  if(L.dPlaneImg && stages == SSD_STAGE_ALL && h->singlePassMode != 0 && (h->singlePassMode == 1 || (single_pass_batch(nframes, nPoints) && !depthInput)))
  {
    if(h->singlePassMode == 1 || h->singlePassBackoff == 0)
      planeImg = L.dPlaneImg;
    else
      h->singlePassBackoff--;                            /* see ssd_fetch_back */
  }
  return planeImg;
}

/* the timing slot of this enqueue: which optional passes it times, their events on the first timed enqueue that runs them */
static int timing_slots(ssd_handle *h, bool timing, int timingSlot, bool labels, bool moments, bool riserLabels)
{
  if(labels && timing)
  {
    /* the label kernel's events, on the first timed enqueue that labels */
    const int rcEv = timed_pass_make(h->labelsPass, "hipEventCreate (labels): ");
    if(rcEv) return rcEv;
  }
  h->labelsPass.timed[timingSlot] = labels && timing;
  if(moments && timing)
  {
    const int rcEv = timed_pass_make(h->surfacePass, "hipEventCreate (surface moments): ");
    if(rcEv) return rcEv;
  }
  h->surfacePass.timed[timingSlot] = moments && timing;
  h->riserLabelsPass.timed[timingSlot] = riserLabels && timing;
  return SSD_OK;
}

/* what enqueue_impl has decided for the call, beside what the Batch holds (constants, frames, stream): read by the chain and by the
 * book-keeping behind it */
struct EnqueueCall
{
  ChunkPlan chunks;
  int stages;
  unsigned long long *planeImg;                  /* the single pass's planes; null: two passes */
  unsigned char *labels;
  size_t labelStride;
  ssd_frame_moments *moments;
  bool riserMoments, riserLabels;
};

/* the result slot the next enqueue that runs the last stage takes, and its records as k_final addresses them: a few frames go straight
 * into the pinned side (run_chain) */
static int result_slot(const ssd_handle *h)
{
  return static_cast<int>(h->finalCount % static_cast<unsigned long long>(h->nSlots));
}
static bool results_direct(const ssd_handle *h, int nframes)
{
  return nframes <= kDirectResultFrames && h->hResultsDev != nullptr;
}
static ssd_frame_result *result_records(ssd_handle *h, int nframes, int slot)
{
  return (results_direct(h, nframes) ? h->hResultsDev : h->dResults) + static_cast<size_t>(slot) * h->F;
}

/* the kernels of the chosen stages on the batch's stream, in order */
static void run_chain(ssd_handle *h, ssd_lane &L, const Batch &B, const EnqueueCall &c, bool marks)
{
  const Params &P = B.P;
  hipStream_t s = B.s;
  const int stages = c.stages, nframes = B.nframes, chunk = c.chunks.chunk, timingSlot = static_cast<int>(h->enqueueCount % SSD_TIMING_SLOTS);
  unsigned long long *planeImg = c.planeImg;
  DebugFrame *dbg = h->debug ? h->dDebug : nullptr;
  unsigned long long *dbgImg = h->debug == 1 ? h->dDebugImg : nullptr;
  int evi = timingSlot * 8;
  auto mk = [&]() { if(marks) (void)hipEventRecord(h->ev[evi++], s); };
  if(planeImg)
  {
    /* k_predict in front of the seven stages, timed by itself (ssd_get_predict_time_back) */
    if(marks) (void)hipEventRecord(h->evPredict[timingSlot], s);
    launch_predict(B, L.dFallback, h->planePool, h->singlePassSabotage);
  }
  mk();
  if(stages & SSD_STAGE_HIST)
    launch_hist(B, c.chunks.hist, planeImg);
  mk();
  if(stages & SSD_STAGE_PEAKS)
    launch_peaks(B, dbg, planeImg ? L.dFallback : nullptr);
  mk();
  if(stages & SSD_STAGE_RASTER)
    launch_raster(B, c.chunks.raster, L.dStepImg, planeImg ? L.dFallback : nullptr);
  mk();
  if(stages & SSD_STAGE_OUTLINE)
    launch_outline(B, L.dStepImg, planeImg, dbg, dbgImg);
  mk();
  if(stages & SSD_STAGE_QUADS)
    launch_quads(B, dbg);
  mk();
  if(stages & SSD_STAGE_INQUAD)
    launch_inquad(B, c.chunks.inquad, L.dGroundImg);
  mk();
  /* The results leave with the batch, into this enqueue's pinned slot (event for ssd_fetch / ssd_fetch_back).  A few frames:
   * k_final stores them there itself — a kilobyte per frame of posted writes, visible to the host once the event has
   * fired — instead of a device-to-host copy command behind the kernel (single frame: one command less in the chain).
   * Batches go through device memory and one copy: a megabyte of scattered stores over PCIe would hold k_final's blocks. */
  if(stages & SSD_STAGE_FINAL)
  {
    launch_final(B, L.dGroundImg, result_records(h, nframes, result_slot(h)), dbg, dbgImg);
    if(P.risers && c.riserMoments)
    {
      /* the riser fit: k_riser_moments in place of k_risers - one walk, both results; the records are zeroed in front of it, it only adds */
      (void)hipMemsetAsync(h->dRiserMoments, 0, sizeof(ssd_frame_moments) * static_cast<size_t>(nframes), s);
      launch_riser_moments(B, chunk, h->dRisers, h->dRiserMoments);
    }
    else if(P.risers)
      launch_risers(B, chunk, h->dRisers);
  }
  mk();
  /* per-pixel labels: behind the seven stages (and their timing), in front of the batch's completion event */
  if(c.labels)
  {
    if(marks) h->labelsPass.begin(timingSlot, s);
    launch_labels(B, chunk, c.labels, c.labelStride);
    if(marks) h->labelsPass.end(timingSlot, s);
    /* the riser labels: behind k_labels (which has written every byte) and behind the riser pass above, outside k_labels' timing */
    if(c.riserLabels)
    {
      if(marks) h->riserLabelsPass.begin(timingSlot, s);
      launch_riser_labels(B, chunk, c.labels, c.labelStride);
      if(marks) h->riserLabelsPass.end(timingSlot, s);
    }
  }
  /* per-surface moments: likewise; the records are zeroed on the batch's stream in front of the kernel, which only adds */
  if(c.moments)
  {
    if(marks) h->surfacePass.begin(timingSlot, s);
    (void)hipMemsetAsync(c.moments, 0, sizeof(ssd_frame_moments) * static_cast<size_t>(nframes), s);
    launch_surface_moments(B, chunk, c.moments);
    if(marks) h->surfacePass.end(timingSlot, s);
  }
}

/* the book-keeping behind the chain: the results on their way to the pinned slot with their event, the lane's completion event, what
 * the workspace and the handle remember of the call - and, for a whole run, what a follow-on pass may be held to */
static int close_enqueue(ssd_handle *h, ssd_lane &L, const Batch &B, const EnqueueCall &c, const void *d_xyz, size_t frame_stride_bytes, bool cameras)
{
  hipStream_t s = B.s;
  const int stages = c.stages, nframes = B.nframes, slot = result_slot(h), li = static_cast<int>(&L - h->lane);
  if(stages & SSD_STAGE_HIST)
    L.dirtyFrames = nframes;
  if(stages & SSD_STAGE_FINAL)
  {
    if(!results_direct(h, nframes))
      HIP_TRY(hipMemcpyAsync(h->hResults + static_cast<size_t>(slot) * h->F, h->dResults + static_cast<size_t>(slot) * h->F,
                             sizeof(ssd_frame_result) * nframes, hipMemcpyDeviceToHost, s));
    /* single pass: how many frames k_raster had to do travels with the results (ssd_fetch_back adapts to it) */
    h->resultsFallback[slot] = -1;
    if(c.planeImg && h->hFallback)
    {
      HIP_TRY(hipMemcpyAsync(h->hFallback + 2 * slot, L.dFallback, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
      h->resultsFallback[slot] = 0;
    }
    HIP_TRY(hipEventRecord(h->resultsReady[slot], s));
    h->resultsFrames[slot] = nframes;
    h->resultsLane[slot] = li;
    h->finalCount++;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(L.done, s));
  if((stages & SSD_STAGE_PEAKS) && nframes >= L.dirtyFrames)
    L.dirtyFrames = 0;
  L.lastStream = s;
  L.haveLast = true;
  /* a raster without its consumer leaves bits behind; the consumer clears what it read */
  if(stages & SSD_STAGE_RASTER) L.stepImagesDirty = true;
  if(stages & SSD_STAGE_OUTLINE) L.stepImagesDirty = false;
  if(stages & SSD_STAGE_INQUAD) L.groundImageDirty = true;
  if(stages & SSD_STAGE_FINAL) L.groundImageDirty = false;
  h->lastFrames = nframes;
  h->lastLane = li;
  h->hRisersBatchFrames = 0;
  h->riserMomentsFrames = c.riserMoments ? nframes : 0;
  h->hRiserMomentsBatchFrames = 0;
  h->enqueueCount++;
  if(stages == SSD_STAGE_ALL)
  {
    h->wholeKind = cameras ? 2 : 1;
    h->wholeDepth = B.depthInput;
    h->wholeFrames = d_xyz;
    h->wholeStride = frame_stride_bytes;
    h->wholeResults = result_records(h, nframes, slot);   /* where k_final left its records */
  }
  return SSD_OK;
}

/* camOf (host, nframes entries; ssd_enqueue_cameras has checked them): a cameras batch - frame i takes camera camOf[i] of the table;
 * moments (device, nframes records): the surface moments of the batch (of a cameras batch too: each frame under its own camera) */
static int enqueue_impl(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream, int stages, bool depthInput,
                        unsigned char *labels = nullptr, size_t labelStride = 0, const uint16_t *camOf = nullptr, ssd_frame_moments *moments = nullptr)
{
  int rc = check_enqueue_args(h, d_xyz, frame_stride_bytes, nframes, stages, depthInput, camOf, moments);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  h->wholeKind = 0;                            /* what a refit may be held to (ssd_enqueue_surface_refit): set again when this call has gone out whole */
  Params P = h->P;
  P.px.groundFull = h->debug == 1 ? 1 : 0;     /* image capture compares the whole ground image; otherwise only what k_final reads is rastered */
  const bool pinned = h->debug != 0 || P.risers || stages != SSD_STAGE_ALL;
  int li = 0;
  hipStream_t s = nullptr;
  rc = take_workspace(h, pinned, static_cast<hipStream_t>(stream), li, s);
  if(rc) return rc;
  ssd_lane &L = h->lane[li];
  CameraSel camSel{};
  const CameraSel *cams = nullptr;
  if(camOf)
  {
    rc = send_camera_index(h, L, P, camOf, nframes, s, camSel);
    if(rc) return rc;
    cams = &camSel;
  }
  const Batch B = make_batch(h, P, L, d_xyz, frame_stride_bytes, nframes, depthInput, s, cams);
  const ChunkPlan chunks = chunk_plan(h->tune, P.nPoints, nframes);
  unsigned long long *planeImg = single_pass_planes(h, L, P.nPoints, stages, nframes, depthInput);
  /* the optional device buffers the kernels dereference without a test of their own: a handle that lacks one
   * fails here, loudly, instead of faulting on the device at a null address */
  if(planeImg && !L.dFallback)
    return fail(SSD_E_HIP, "ssd_enqueue: the single pass's planes without their work list (internal)");
  if(depthInput && !cams && (!B.depth.xmap || !B.depth.ymap))
    return fail(SSD_E_HIP, "ssd_enqueue_depth: the deprojection maps are missing (ssd_set_intrinsics did not complete)");
  if(!L.dState || !L.dStepImg || !L.dGroundImg || !L.dTileMasks)
    return fail(SSD_E_HIP, "ssd_enqueue: the handle's workspace is incomplete (internal)");
  h->lastSinglePass = planeImg != nullptr;
  h->predictTimed[h->enqueueCount % SSD_TIMING_SLOTS] = planeImg != nullptr;
  const bool timing = h->timing && !h->ev.empty();
  const int timingSlot = static_cast<int>(h->enqueueCount % SSD_TIMING_SLOTS);
  /* riser moments: whole runs only (ssd_enqueue_stages takes none), and only with the riser pass they ride on */
  const bool riserMoments = P.risers && h->riserMoments && h->dRiserMoments && h->dRisers && stages == SSD_STAGE_ALL;
  /* riser labels: only where labels are written, and only with the riser pass (k_final refreshes wantedRisers / riserOfBin only then) */
  const bool riserLabels = labels != nullptr && P.risers && h->riserLabels && !h->riserLabelsPass.ev.empty() && stages == SSD_STAGE_ALL;
  rc = timing_slots(h, timing, timingSlot, labels != nullptr, moments != nullptr, riserLabels);
  if(rc) return rc;

  const int slot = result_slot(h);
  if((stages & SSD_STAGE_FINAL) && h->depth > 1 && h->resultsLane[slot] != li && h->lane[h->resultsLane[slot]].haveLast)
    HIP_TRY(hipStreamWaitEvent(s, h->lane[h->resultsLane[slot]].done, 0));     /* the slot's previous writer was another lane */
  const EnqueueCall call{ chunks, stages, planeImg, labels, labelStride, moments, riserMoments, riserLabels };

  /* (A call of a few frames replayed from a captured HIP graph — one submission instead of seven launches — was measured in
   * round 3 and is slower on ROCm 7.2: one resident XGA frame 100 -> 200 us per ssd_enqueue + ssd_fetch, eight frames 134 ->
   * 158 us.  The code left the product in round 4; git history of this file has it.) */
  {
    /* bits a partial run (ssd_enqueue_stages) left behind: wiped before the stage that would raster on top of them — not
     * before a call that only CONSUMES them (the continuation of that partial run: k_outline / k_final read and clear) */
    if(L.stepImagesDirty && (stages & SSD_STAGE_RASTER))
    {
      HIP_TRY(hipMemsetAsync(L.dStepImg, 0, static_cast<size_t>(h->F) * P.maxStepImages * h->imgWords * 8, s));
      L.stepImagesDirty = false;
    }
    if(L.groundImageDirty && (stages & SSD_STAGE_INQUAD))
    {
      HIP_TRY(hipMemsetAsync(L.dGroundImg, 0, static_cast<size_t>(h->F) * h->imgWords * 8, s));
      L.groundImageDirty = false;
    }
    if(stages & SSD_STAGE_HIST)
    {
      /* No memset of the state in front of a call: K1 only needs its accumulators zero, and k_peaks — their one reader —
       * clears them as it takes them (everything else in FrameState is written before it is read).  Only after a call that
       * ran K1 without k_peaks (ssd_enqueue_stages), or one that failed half way, the state is zeroed here. */
      if(L.dirtyFrames > 0)
        HIP_TRY(hipMemsetAsync(L.dState, 0, sizeof(FrameState) * L.dirtyFrames, s));
      if(h->debug && h->dDebug)
        HIP_TRY(hipMemsetAsync(h->dDebug, 0, sizeof(DebugFrame) * nframes, s));
    }
    run_chain(h, L, B, call, timing);
  }
  return close_enqueue(h, L, B, call, d_xyz, frame_stride_bytes, camOf != nullptr);
}

int ssd_enqueue_stages(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream, int stages)
{
  return enqueue_impl(h, d_xyz, frame_stride_bytes, nframes, stream, stages, false);
}

int ssd_enqueue(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream)
{
  return enqueue_impl(h, d_xyz, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, false);
}

int ssd_enqueue_depth(ssd_handle *h, const void *d_depth, size_t frame_stride_bytes, int nframes, void *stream)
{
  return enqueue_impl(h, d_depth, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, true);
}

static int check_labels_dest(const ssd_handle *h, const char *who, const uint8_t *d_labels, size_t label_stride_bytes)
{
  if(!h || !d_labels)
    return fail(SSD_E_ARG, std::string(who) + ": null argument");
  if(label_stride_bytes < static_cast<size_t>(h->P.nPoints))
    return fail(SSD_E_ARG, std::string(who) + ": label stride smaller than width * height");
  return SSD_OK;
}

int ssd_enqueue_labels(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream,
                       uint8_t *d_labels, size_t label_stride_bytes)
{
  const int rc = check_labels_dest(h, "ssd_enqueue_labels", d_labels, label_stride_bytes);
  if(rc) return rc;
  return enqueue_impl(h, d_xyz, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, false, d_labels, label_stride_bytes);
}

int ssd_enqueue_depth_labels(ssd_handle *h, const void *d_depth, size_t frame_stride_bytes, int nframes, void *stream,
                             uint8_t *d_labels, size_t label_stride_bytes)
{
  const int rc = check_labels_dest(h, "ssd_enqueue_depth_labels", d_labels, label_stride_bytes);
  if(rc) return rc;
  return enqueue_impl(h, d_depth, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, true, d_labels, label_stride_bytes);
}

int ssd_enqueue_surface_moments(ssd_handle *h, const void *d_xyz, size_t frame_stride_bytes, int nframes, void *stream, ssd_frame_moments *d_out)
{
  if(!h || !d_out)
    return fail(SSD_E_ARG, "ssd_enqueue_surface_moments: null argument");
  return enqueue_impl(h, d_xyz, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, false, nullptr, 0, nullptr, d_out);
}

int ssd_enqueue_depth_surface_moments(ssd_handle *h, const void *d_depth, size_t frame_stride_bytes, int nframes, void *stream, ssd_frame_moments *d_out)
{
  if(!h || !d_out)
    return fail(SSD_E_ARG, "ssd_enqueue_depth_surface_moments: null argument");
  return enqueue_impl(h, d_depth, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, true, nullptr, 0, nullptr, d_out);
}

int ssd_set_intrinsics(ssd_handle *h, const ssd_intrinsics *intr)
{
  if(!h || !intr || !(intr->fx != 0.0f) || !(intr->fy != 0.0f) || !(intr->depth_units > 0.0f))
    return fail(SSD_E_ARG, "ssd_set_intrinsics: bad argument");
  HIP_TRY(hipSetDevice(h->device));
  std::vector<float> maps;
  depth_maps(*intr, h->P.W, h->P.H, maps);
  if(!h->dDepthMaps)
    HIP_TRY(h->dDepthMaps.alloc(maps.size() * 4));
  /* depth batches still running (on the lanes' non-blocking streams, which a null-stream copy does not wait for) read the maps
   * in K1, K2 and K4: let every lane finish before they change */
  for(int k = 0; k < h->depth; k++)
    if(h->lane[k].haveLast)
      HIP_TRY(hipEventSynchronize(h->lane[k].done));
  HIP_TRY(hipMemcpy(h->dDepthMaps, maps.data(), maps.size() * 4, hipMemcpyHostToDevice));
  h->intr = *intr;
  h->haveIntr = true;
  h->wholeKind = 0;                            /* a refit would deproject with other maps than the enqueue it follows did */
  return SSD_OK;
}

/* The getters of a timed enqueue's times: their arguments, and the ring slot of the enqueue at `back` (0 is the last one, 1 the one
 * before, ...: at most SSD_TIMING_SLOTS - 1 back, and not before timing was switched on) */
static int timed_slot(ssd_handle *h, int back, const void *out, const char *who, int *slot)
{
  if(!h || !out)
    return fail(SSD_E_ARG, std::string(who) + ": null");
  if(!h->timing || h->ev.empty() || back < 0 || back >= SSD_TIMING_SLOTS ||
     h->enqueueCount < static_cast<unsigned long long>(back) + 1 || h->enqueueCount - 1 - back < h->timedFrom)
    return fail(SSD_E_ARG, std::string(who) + ": no timed enqueue at that position");
  HIP_TRY(hipSetDevice(h->device));
  *slot = static_cast<int>((h->enqueueCount - 1 - back) % SSD_TIMING_SLOTS);
  return SSD_OK;
}

/* ... of an optional pass: 0 for an enqueue that did not run it; waits for that enqueue's pass */
static int timed_pass_back(ssd_handle *h, int back, float *ms, const char *who, ssd_timed_pass ssd_handle::*pass)
{
  int slot = 0;
  const int rc = timed_slot(h, back, ms, who, &slot);
  if(rc) return rc;
  *ms = 0.0f;
  HIP_TRY((h->*pass).elapsed(slot, ms));
  return SSD_OK;
}

/* milliseconds of the 7 stages of a timed enqueue; waits for that enqueue */
int ssd_get_stage_times_back(ssd_handle *h, int back, float ms[7])
{
  int slot = 0;
  const int rc = timed_slot(h, back, ms, "ssd_get_stage_times", &slot);
  if(rc) return rc;
  const int base = slot * 8;
  HIP_TRY(hipEventSynchronize(h->ev[base + 7]));
  for(int i = 0; i < 7; i++)
    HIP_TRY(hipEventElapsedTime(&ms[i], h->ev[base + i], h->ev[base + i + 1]));
  return SSD_OK;
}

/* k_predict's time, the kernel in front of the seven stages of a single-pass batch (0 for an enqueue that did not run it): one event,
 * ended by the first of the stages' */
int ssd_get_predict_time_back(ssd_handle *h, int back, float *ms)
{
  int slot = 0;
  const int rc = timed_slot(h, back, ms, "ssd_get_predict_time_back", &slot);
  if(rc) return rc;
  *ms = 0.0f;
  if(!h->predictTimed[slot])
    return SSD_OK;
  HIP_TRY(hipEventSynchronize(h->ev[slot * 8 + 7]));
  HIP_TRY(hipEventElapsedTime(ms, h->evPredict[slot], h->ev[slot * 8]));
  return SSD_OK;
}

/* k_labels' time for the same enqueue (0 for an enqueue that wrote no labels) */
int ssd_get_labels_time_back(ssd_handle *h, int back, float *ms)
{
  return timed_pass_back(h, back, ms, "ssd_get_labels_time_back", &ssd_handle::labelsPass);
}

/* k_riser_labels' time for the same enqueue (0 for an enqueue that marked nothing) */
int ssd_get_riser_labels_time_back(ssd_handle *h, int back, float *ms)
{
  return timed_pass_back(h, back, ms, "ssd_get_riser_labels_time_back", &ssd_handle::riserLabelsPass);
}

/* k_surface_moments' time (with the memset in front of it) for the same enqueue (0 for an enqueue that gathered none) */
int ssd_get_surface_moments_time_back(ssd_handle *h, int back, float *ms)
{
  return timed_pass_back(h, back, ms, "ssd_get_surface_moments_time_back", &ssd_handle::surfacePass);
}

int ssd_get_stage_times(ssd_handle *h, float ms[7])
{
  return ssd_get_stage_times_back(h, 0, ms);
}

int ssd_fetch_back(ssd_handle *h, ssd_frame_result *results, int nframes, int back)
{
  if(!h || !results)
    return fail(SSD_E_ARG, "ssd_fetch: null argument");
  if(back < 0 || back >= h->nSlots || h->finalCount < static_cast<unsigned long long>(back) + 1)
    return fail(SSD_E_ARG, "ssd_fetch: no enqueue at that position (back = 0: the last one, 1: the one before, .. < max(2, batches_in_flight))");
  const int slot = static_cast<int>((h->finalCount - 1 - back) % static_cast<unsigned long long>(h->nSlots));
  if(nframes < 1 || nframes > h->resultsFrames[slot])
    return fail(SSD_E_ARG, "ssd_fetch: nframes exceeds what that enqueue processed");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipEventSynchronize(h->resultsReady[slot]));
  std::memcpy(results, h->hResults + static_cast<size_t>(slot) * h->F, sizeof(ssd_frame_result) * nframes);
  /* The single pass pays when there are step plateaus to raster and its predictor covers them.  A batch of which k_raster had to
   * do more than half of the frames (scenes without a sharp peak per tread, or far more treads than planes), or of which fewer
   * than a quarter of the frames had a step plateau at all (no stairs in sight: k_predict and K1's idle raster code cost 7 % and
   * k_raster would have had nothing to do anyway), says the input is of the other kind: the next kSinglePassBackoff qualifying
   * batches run two passes, then one batch probes again.  Results do not depend on it. */
  if(h->resultsFallback[slot] == 0)
  {
    h->resultsFallback[slot] = 1;                       /* counted once */
    const int listed = h->hFallback[2 * slot], frames = h->resultsFrames[slot], withSteps = frames - h->hFallback[2 * slot + 1];
    if(2 * listed > frames || 4 * withSteps < frames)
      h->singlePassBackoff = kSinglePassBackoff;
  }
  return SSD_OK;
}

int ssd_stream_wait(ssd_handle *h, int back, void *stream)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_stream_wait: null handle");
  if(back < 0 || back >= h->nSlots || h->finalCount < static_cast<unsigned long long>(back) + 1)
    return fail(SSD_E_ARG, "ssd_stream_wait: no enqueue at that position");
  const int slot = static_cast<int>((h->finalCount - 1 - back) % static_cast<unsigned long long>(h->nSlots));
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->resultsReady[slot], 0));
  return SSD_OK;
}

int ssd_batches_in_flight(const ssd_handle *h)
{
  return h ? h->depth : 0;
}

int ssd_fetch(ssd_handle *h, ssd_frame_result *results, int nframes, void *stream)
{
  (void)stream;                  /* the copy was enqueued with the batch; its event is what is waited for */
  return ssd_fetch_back(h, results, nframes, 0);
}

/* ---- frames in host memory: double-buffered ingest ----------------------------------------------------------------
 * A camera-fed product is host-fed: frames arrive in host memory and cross PCIe once (9.4 MB per XGA vertex frame,
 * 1.6 MB as 16-bit depth).  The batch is cut into slices of at most kIngestFrames frames; slice c + 1 is copied into the
 * other of two device staging buffers on a copy stream while the kernels of slice c run on a compute stream, and the
 * results of slice c - 1 are read (they travelled with their enqueue).  Source memory obtained from ssd_host_alloc is
 * pinned: its copies are true DMA; pageable memory goes through the runtime's own staging (the call then blocks in
 * the copy while the GPU computes the previous slice). */
static const int kIngestFrames = 32;

static int ingest_prepare(ssd_handle *h, size_t sliceBytes)
{
  if(!h->ingestCopy)
  {
    /* the three streams and six events are one group, the two buffers another (ssd_owned.h): SliceFeed finds all of a group or none */
    Stream s[3];
    Event ev[6];
    hipError_t e = hipSuccess;
    for(Stream &x : s)
      if(e == hipSuccess) e = x.create(hipStreamNonBlocking);
    for(Event &x : ev)
      if(e == hipSuccess) e = x.create(hipEventDisableTiming);
    if(e != hipSuccess)
      return fail(SSD_E_HIP, std::string("the host feed's streams and events: ") + hipGetErrorString(e));
    h->ingestCopy = std::move(s[0]); h->ingestCopy2 = std::move(s[1]); h->ingestCompute = std::move(s[2]);
    for(int k = 0; k < 2; k++)
    {
      h->ingestCopied[k] = std::move(ev[k]); h->ingestCopied2[k] = std::move(ev[2 + k]); h->ingestConsumed[k] = std::move(ev[4 + k]);
    }
  }
  if(h->ingestCap < sliceBytes)
  {
    HIP_TRY(hipDeviceSynchronize());
    for(int k = 0; k < 2; k++)
      h->ingestBuf[k].reset();
    h->ingestCap = 0;
    DeviceBuf<void> buf[2];
    hipError_t e = buf[0].alloc(sliceBytes);
    if(e == hipSuccess) e = buf[1].alloc(sliceBytes);
    if(e != hipSuccess)
      return fail(SSD_E_HIP, std::string("the host feed's staging buffers: ") + hipGetErrorString(e));
    h->ingestBuf[0] = std::move(buf[0]); h->ingestBuf[1] = std::move(buf[1]);
    h->ingestCap = sliceBytes;
  }
  return SSD_OK;
}

/* The frames of a host batch: packed where the caller holds them, at devFrameBytes apart in a staging buffer.  The pipeline keeps a depth
 * frame's device stride a multiple of 8 bytes (four elements; a vertex frame is one of 4 as it is); the ground fit's kernel loads 16 bytes
 * wide, so there every frame starts on such a boundary. */
struct HostFrames
{
  bool depth;
  size_t srcFrameBytes, devFrameBytes;
};
enum FrameUser { kForPipeline, kForGroundFit };

static HostFrames host_frames(const ssd_handle *h, int input, FrameUser user)
{
  const bool depth = input == SSD_INPUT_DEPTH16;
  const size_t src = static_cast<size_t>(h->P.nPoints) * (depth ? 2 : 12);
  const size_t align = user == kForGroundFit ? 16 : depth ? 8 : 4;
  return HostFrames{ depth, src, (src + align - 1) / align * align };
}

/* the device frames of a stand-alone frame pass (the ground fit, the stair pose), refused under the enqueue's name: the pointer and the
 * stride on an element's boundary, and with more than one frame a stride that holds a frame */
static int check_device_frames(const ssd_handle *h, const char *who, const void *d_frames, size_t frame_stride_bytes, int nframes, int input)
{
  const size_t unit = input == SSD_INPUT_DEPTH16 ? 2 : 4, frameBytes = host_frames(h, input, kForGroundFit).srcFrameBytes;
  if(reinterpret_cast<size_t>(d_frames) % unit != 0 || frame_stride_bytes % unit != 0 || (nframes > 1 && frame_stride_bytes < frameBytes))
    return fail(SSD_E_ARG, std::string(who) + ": frames must be aligned to their element and the stride must hold a frame");
  return SSD_OK;
}

/* the refusals of a cameras batch (include/ssd_hip.h), before anything is launched or copied */
static int check_cameras(const ssd_handle *h, const char *who, const uint16_t *camOf, int nframes, int input)
{
  if(!camOf)
    return fail(SSD_E_ARG, std::string(who) + ": null camera_of_frame");
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, std::string(who) + ": input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  if(h->camParams.empty())
    return fail(SSD_E_ARG, std::string(who) + ": the handle has no camera table (ssd_set_cameras)");
  for(int i = 0; i < nframes; i++)
  {
    if(camOf[i] >= h->camParams.size())
      return fail(SSD_E_ARG, std::string(who) + ": frame " + std::to_string(i) + " names camera " + std::to_string(camOf[i]) + " of " + std::to_string(h->camParams.size()));
    if(input == SSD_INPUT_DEPTH16 && !h->camHasIntr[camOf[i]])
      return fail(SSD_E_ARG, std::string(who) + ": depth input of frame " + std::to_string(i) + " names camera " + std::to_string(camOf[i]) + ", which has no intrinsics");
  }
  return SSD_OK;
}

/* The refusals every ssd_process_*host* entry point begins with, before anything is launched or copied.  `pointers`: the handle, the frames
 * and whatever else that entry point cannot do without are there.  Then what the frames are read under: the handle's calibration (depth
 * needs its intrinsics), the camera table (check_cameras), or priors of the call's own, which the caller checks behind this. */
enum HostCal { kHandleCal, kCameraTable, kOwnPriors };

static int check_host_batch(const ssd_handle *h, const char *who, bool pointers, int nframes, int input, HostCal cal, const uint16_t *camOf = nullptr)
{
  if(!pointers || nframes < 1)
    return fail(SSD_E_ARG, std::string(who) + ": bad argument");
  if(cal == kCameraTable)
    return check_cameras(h, who, camOf, nframes, input);
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, std::string(who) + ": input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  if(cal == kHandleCal && input == SSD_INPUT_DEPTH16 && !h->haveIntr)
    return fail(SSD_E_ARG, std::string(who) + ": call ssd_set_intrinsics first");
  return SSD_OK;
}

/* One host batch on its way through ingestBuf[2]: everything about getting slice c into buffer c & 1, nothing about what is done with it.
 * stage(c) issues the copy on ingestCopy (the second half of a large slice on ingestCopy2) with ingestCopied / ingestCopied2 behind it;
 * ready(c) makes ingestCompute wait for those; consumed(c, s) records ingestConsumed on the stream the slice's last reader ran on, and
 * from slice 2 on stage() makes the copy streams wait for it before they write the buffer again.  A body calls stage(c) at the top of
 * its own iteration - or one slice ahead, in front of a step that blocks -, then ready(c), its kernels, consumed(c, ...).  Between calls
 * nothing is owed: every entry point returns with its last slice's results read, which is behind that slice's kernels. */
struct SliceFeed
{
  ssd_handle *h;
  HostFrames f;
  const void *frames;
  int nframes;
  int slice = 0;                              /* frames per slice */
  int staged = 0;                             /* slices whose copy has gone out */
  bool split[2] = { false, false };           /* the slice in that buffer went over in two halves */

  int prepare()
  {
    slice = h->F < kIngestFrames ? h->F : kIngestFrames;
    return ingest_prepare(h, static_cast<size_t>(slice) * f.devFrameBytes);
  }
  int slices() const { return (nframes - 1) / slice + 1; }
  int first(int c) const { return c * slice; }
  int count(int c) const { return nframes - first(c) < slice ? nframes - first(c) : slice; }

  /* slice c's copy; nothing if it has gone out already or the batch has no such slice */
  int stage(int c)
  {
    if(c < staged || c >= slices())
      return SSD_OK;
    const int k = c & 1, n = count(c);
    const unsigned char *src = static_cast<const unsigned char *>(frames) + static_cast<size_t>(first(c)) * f.srcFrameBytes;
    /* A slice of 16 MB and more goes over in two halves on two copy streams: one copy of a pinned source runs on ONE copy engine, at 42 GB/s
     * on the boxes of rounds 5 and 6, while the runtime's own staging of a pageable source reached 55 (bench.py: host_fed, both
     * orders, two warm-up calls) - the pinned source was the slower one. */
    const size_t bytes = static_cast<size_t>(n) * f.srcFrameBytes, half = (bytes / 2) & ~static_cast<size_t>(4095);
    const bool packed = f.srcFrameBytes == f.devFrameBytes;
    split[k] = packed && half >= (static_cast<size_t>(8) << 20);
    if(c >= 2)
    {
      HIP_TRY(hipStreamWaitEvent(h->ingestCopy, h->ingestConsumed[k], 0));        /* the readers of slice c - 2 are through with this buffer */
      if(split[k])
        HIP_TRY(hipStreamWaitEvent(h->ingestCopy2, h->ingestConsumed[k], 0));
    }
    if(split[k])
    {
      HIP_TRY(hipMemcpyAsync(static_cast<unsigned char *>(h->ingestBuf[k].get()) + half, src + half, bytes - half, hipMemcpyHostToDevice, h->ingestCopy2));
      HIP_TRY(hipEventRecord(h->ingestCopied2[k], h->ingestCopy2));
    }
    if(packed)
      HIP_TRY(hipMemcpyAsync(h->ingestBuf[k], src, split[k] ? half : bytes, hipMemcpyHostToDevice, h->ingestCopy));
    else
      HIP_TRY(hipMemcpy2DAsync(h->ingestBuf[k], f.devFrameBytes, src, f.srcFrameBytes, f.srcFrameBytes, n, hipMemcpyHostToDevice, h->ingestCopy));
    HIP_TRY(hipEventRecord(h->ingestCopied[k], h->ingestCopy));
    staged = c + 1;
    return SSD_OK;
  }

  /* slice c, staged before: its buffer, first frame and count, with ingestCompute behind its copy */
  int ready(int c, const void *&buf, int &at, int &n)
  {
    const int k = c & 1;
    if(split[k])
      HIP_TRY(hipStreamWaitEvent(h->ingestCompute, h->ingestCopied2[k], 0));
    HIP_TRY(hipStreamWaitEvent(h->ingestCompute, h->ingestCopied[k], 0));
    buf = h->ingestBuf[k];
    at = first(c);
    n = count(c);
    return SSD_OK;
  }

  /* whatever read slice c's buffer ends on stream s with what s holds now */
  int consumed(int c, hipStream_t s)
  {
    HIP_TRY(hipEventRecord(h->ingestConsumed[c & 1], s));
    return SSD_OK;
  }
};

extern "C++"
{
/* The host-fed loop of a stand-alone frame pass (the ground fit, the stair pose: no whole run in front, one set of records in pinned
 * memory).  Per slice: its copy; collect(first, n) of the slice before - its kernel ran beside this slice's copy, and the records are one
 * set, read before this slice's kernel writes them -; enqueue(buf, first, n) on ingestCompute; consumed.  Then the last slice's collect */
template<class Enqueue, class Collect>
static int process_host_frames(ssd_handle *h, SliceFeed &feed, Enqueue enqueue, Collect collect)
{
  const int last = feed.slices() - 1;
  for(int c = 0; c <= last; c++)
  {
    const void *buf;
    int at, n;
    int rc = feed.stage(c);
    if(!rc && c >= 1) rc = collect(feed.first(c - 1), feed.count(c - 1));
    if(!rc) rc = feed.ready(c, buf, at, n);
    if(!rc) rc = enqueue(buf, at, n);
    if(!rc) rc = feed.consumed(c, h->ingestCompute);
    if(rc) return rc;
  }
  return collect(feed.first(last), feed.count(last));
}

} // extern "C++"

/* the labels of the host entry points: two device buffers of a slice's labels and the stream that copies them out */
static int labels_prepare(ssd_handle *h, size_t sliceBytes)
{
  if(!h->labelsCopy)
  {
    Stream copy;
    Event copied[2];
    hipError_t e = copy.create(hipStreamNonBlocking);
    if(e == hipSuccess) e = copied[0].create(hipEventDisableTiming);
    if(e == hipSuccess) e = copied[1].create(hipEventDisableTiming);
    if(e != hipSuccess)
      return fail(SSD_E_HIP, std::string("the staged output's stream and events: ") + hipGetErrorString(e));
    h->labelsCopy = std::move(copy); h->labelsCopied[0] = std::move(copied[0]); h->labelsCopied[1] = std::move(copied[1]);
  }
  if(h->labelStageCap < sliceBytes)
  {
    /* the buffers' users are this handle's: label kernels on its lanes' streams, their copies on labelsCopy */
    for(int k = 0; k < h->depth; k++)
      if(h->lane[k].haveLast)
        HIP_TRY(hipEventSynchronize(h->lane[k].done));
    HIP_TRY(hipStreamSynchronize(h->labelsCopy));
    for(int k = 0; k < 2; k++)
      h->labelStage[k].reset();
    h->labelStageCap = 0;
    DeviceBuf<unsigned char> buf[2];
    hipError_t e = buf[0].alloc(sliceBytes);
    if(e == hipSuccess) e = buf[1].alloc(sliceBytes);
    if(e != hipSuccess)
      return fail(SSD_E_HIP, std::string("the staged output's buffers: ") + hipGetErrorString(e));
    h->labelStage[0] = std::move(buf[0]); h->labelStage[1] = std::move(buf[1]);
    h->labelStageCap = sliceBytes;
  }
  return SSD_OK;
}

/* What a slice leaves in labelStage[c & 1] beside its results, and where it goes: a byte per point for enqueue_impl's `labels`, or one
 * ssd_frame_moments per frame for its `moments` - the same staging buffers, copy stream and events either way.  host == nullptr: nothing. */
struct StagedOut
{
  enum Kind { kLabels, kMoments } kind;
  void *host;
  size_t frameBytes;
};
static StagedOut staged_labels(const ssd_handle *h, uint8_t *labels)
{
  return StagedOut{ StagedOut::kLabels, labels, static_cast<size_t>(h->P.nPoints) };
}
static StagedOut staged_moments(ssd_frame_moments *moments)
{
  return StagedOut{ StagedOut::kMoments, moments, sizeof(ssd_frame_moments) };
}

/* arguments checked by the callers (check_host_batch) */
static int process_host_impl(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                             const StagedOut &out = StagedOut{}, const uint16_t *camOf = nullptr)
{
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForPipeline), frames, nframes };
  int rc = feed.prepare();
  if(rc) return rc;
  if(out.host)
  {
    rc = labels_prepare(h, static_cast<size_t>(feed.slice) * out.frameBytes);
    if(rc) return rc;
  }
  /* whatever path leaves this call, no copy into the caller's memory is still on its way afterwards */
  struct CopiesDone
  {
    hipStream_t s;
    ~CopiesDone() { if(s) (void)hipStreamSynchronize(s); }
  } copiesDone{ out.host ? h->labelsCopy : nullptr };
  /* slice c, enqueued `back` enqueues ago, from its staging buffer to the caller's memory, behind its kernels */
  auto copyOut = [&](int c, int back)
  {
    int r = ssd_stream_wait(h, back, h->labelsCopy);
    if(r) return r;
    HIP_TRY(hipMemcpyAsync(static_cast<unsigned char *>(out.host) + static_cast<size_t>(feed.first(c)) * out.frameBytes, h->labelStage[c & 1],
                           static_cast<size_t>(feed.count(c)) * out.frameBytes, hipMemcpyDeviceToHost, h->labelsCopy));
    HIP_TRY(hipEventRecord(h->labelsCopied[c & 1], h->labelsCopy));
    return SSD_OK;
  };
  const bool risers = h->P.risers && h->dRisers, riserMoments = risers && h->riserMoments && h->dRiserMoments;
  if(risers)
    rc = grow_pinned_batch(h, h->hRisersBatch, h->hRisersBatchCap, nframes);
  if(!rc && riserMoments)
    rc = grow_pinned_batch(h, h->hRiserMomentsBatch, h->hRiserMomentsBatchCap, nframes);
  if(rc) return rc;
  const int last = feed.slices() - 1;
  for(int c = 0; c <= last; c++)
  {
    const int k = c & 1;
    const void *buf;
    int at, n;
    rc = feed.stage(c);
    if(!rc) rc = feed.ready(c, buf, at, n);
    if(rc) return rc;
    if(out.host && c >= 2)
      HIP_TRY(hipStreamWaitEvent(h->ingestCompute, h->labelsCopied[k], 0));      /* what slice c - 2 staged has left this buffer */
    rc = enqueue_impl(h, buf, feed.f.devFrameBytes, n, h->ingestCompute, SSD_STAGE_ALL, feed.f.depth,
                      out.host && out.kind == StagedOut::kLabels ? h->labelStage[k] : nullptr, out.frameBytes,
                      camOf ? camOf + at : nullptr,                                 /* a slice takes its part of the index */
                      out.host && out.kind == StagedOut::kMoments ? reinterpret_cast<ssd_frame_moments *>(h->labelStage[k].get()) : nullptr);
    if(rc) return rc;
    /* "Consumed" is the end of the slice's kernels — on the stream they ran on (with several workspaces the lane's own; the
     * compute stream itself only orders a slice behind its copy, so the slices of a handle with several workspaces overlap
     * like any other batches: making the compute stream wait for every slice — round 3 — had serialised them). */
    if(risers)
    {
      /* the riser buffer is single (enqueues with risers on all run in the first workspace): its copy follows the slice */
      rc = ssd_stream_wait(h, 0, h->ingestCompute);
      if(rc) return rc;
      HIP_TRY(hipMemcpyAsync(h->hRisersBatch + at, h->dRisers, sizeof(ssd_frame_risers) * n, hipMemcpyDeviceToHost, h->ingestCompute));
      if(riserMoments)
        HIP_TRY(hipMemcpyAsync(h->hRiserMomentsBatch + at, h->dRiserMoments, sizeof(ssd_frame_moments) * n, hipMemcpyDeviceToHost, h->ingestCompute));
    }
    rc = feed.consumed(c, risers ? h->ingestCompute : h->lane[h->lastLane].lastStream);
    if(rc) return rc;
    if(c >= 1)
    {
      if(out.host)
      {
        rc = copyOut(c - 1, 1);
        if(rc) return rc;
      }
      rc = ssd_fetch_back(h, results + feed.first(c - 1), feed.count(c - 1), 1);
      if(rc) return rc;
    }
  }
  if(out.host)
  {
    rc = copyOut(last, 0);
    if(rc) return rc;
  }
  rc = ssd_fetch_back(h, results + feed.first(last), feed.count(last), 0);
  if(rc) return rc;
  if(out.host)
    HIP_TRY(hipStreamSynchronize(h->labelsCopy));
  h->hRisersBatchFrames = risers ? nframes : 0;
  h->hRiserMomentsBatchFrames = riserMoments ? nframes : 0;
  return SSD_OK;
}

int ssd_process_host(ssd_handle *h, const float *xyz, int nframes, ssd_frame_result *results)
{
  const int rc = check_host_batch(h, "ssd_process_host", h && xyz && results, nframes, SSD_INPUT_VERTICES, kHandleCal);
  return rc ? rc : process_host_impl(h, xyz, nframes, SSD_INPUT_VERTICES, results);
}

int ssd_process_depth_host(ssd_handle *h, const uint16_t *depth, int nframes, ssd_frame_result *results)
{
  const int rc = check_host_batch(h, "ssd_process_depth_host", h && depth && results, nframes, SSD_INPUT_DEPTH16, kHandleCal);
  return rc ? rc : process_host_impl(h, depth, nframes, SSD_INPUT_DEPTH16, results);
}

int ssd_process_host_labels(ssd_handle *h, const float *xyz, int nframes, ssd_frame_result *results, uint8_t *labels)
{
  const int rc = check_host_batch(h, "ssd_process_host_labels", h && xyz && results && labels, nframes, SSD_INPUT_VERTICES, kHandleCal);
  return rc ? rc : process_host_impl(h, xyz, nframes, SSD_INPUT_VERTICES, results, staged_labels(h, labels));
}

int ssd_process_depth_host_labels(ssd_handle *h, const uint16_t *depth, int nframes, ssd_frame_result *results, uint8_t *labels)
{
  const int rc = check_host_batch(h, "ssd_process_depth_host_labels", h && depth && results && labels, nframes, SSD_INPUT_DEPTH16, kHandleCal);
  return rc ? rc : process_host_impl(h, depth, nframes, SSD_INPUT_DEPTH16, results, staged_labels(h, labels));
}

/* ---- per-frame calibration: the camera table (include/ssd_hip.h) ------------------------------- */

static void cameras_free(ssd_handle *h)
{
  for(ssd_lane &L : h->lane)
  {
    L.dCamIndex.reset(); L.hCamIndex.reset(); L.camCopied.reset();
  }
  h->dCams.reset();
  h->dCamMaps.reset();
  h->camParams.clear(); h->camHasIntr.clear(); h->camDepthUnits.clear();
  h->camsNeedChecks = false;
  h->camCallKey = ~0ull;
}

/* The device records: each camera's Params as make_params() made them, with what a call decides for the whole handle (as
 * enqueue_impl does to its copy of the handle's Params), and the camera's DepthSrc.  Batches in flight read the table: they finish first. */
static int cameras_upload(ssd_handle *h, unsigned long long key, double tol)
{
  for(int k = 0; k < h->depth; k++)
    if(h->lane[k].haveLast)
      HIP_TRY(hipEventSynchronize(h->lane[k].done));
  const size_t n = h->camParams.size();
  std::vector<CameraRec> recs(n);
  const int W = h->P.W, H = h->P.H;
  for(size_t i = 0; i < n; i++)
  {
    CameraRec &R = recs[i];
    std::memset(&R, 0, sizeof(R));
    R.P = h->camParams[i];
    R.P.px.winShift = h->P.px.winShift;          /* the handle's (a tools build may have forced them) */
    R.P.px.winShiftGround = h->P.px.winShiftGround;
    R.P.px.groundFull = static_cast<int>(key & 1u);
    R.P.risers = h->P.risers;
    R.P.riserMinSupport = h->P.riserMinSupport;
    R.P.riserTol = tol;
    float *maps = h->camHasIntr[i] ? h->dCamMaps + i * (static_cast<size_t>(W) + H) : nullptr;
    R.D = DepthSrc{ maps, maps ? maps + W : nullptr, h->camDepthUnits[i], W, H, depth_row_magic(W, H) };
  }
  HIP_TRY(hipMemcpy(h->dCams, recs.data(), sizeof(CameraRec) * n, hipMemcpyHostToDevice));
  h->camCallKey = key;
  h->camCallTol = tol;
  return SSD_OK;
}

int ssd_set_cameras(ssd_handle *h, const ssd_camera *cams, int ncams)
{
  if(!h)
    return fail(SSD_E_ARG, "ssd_set_cameras: null handle");
  if(ncams < 0 || ncams > SSD_MAX_CAMERAS)
    return fail(SSD_E_ARG, "ssd_set_cameras: ncams must be 0.." + std::to_string(SSD_MAX_CAMERAS));
  if(ncams > 0 && !cams)
    return fail(SSD_E_ARG, "ssd_set_cameras: null table");
  /* every camera through make_params() first: a bad one leaves the handle's table as it was */
  std::vector<Params> params(static_cast<size_t>(ncams));
  bool anyIntr = false, checks = false;
  for(int i = 0; i < ncams; i++)
  {
    params[i] = Params{};
    const int rc = make_params(h->cfg, cams[i].cal, params[i]);
    if(rc) return rc;
    if(cams[i].has_intrinsics)
    {
      const ssd_intrinsics &in = cams[i].intr;
      if(!(in.fx != 0.0f) || !(in.fy != 0.0f) || !(in.depth_units > 0.0f))
        return fail(SSD_E_ARG, "ssd_set_cameras: bad intrinsics of camera " + std::to_string(i));
      anyIntr = true;
    }
    checks = checks || needs_checks(params[i]);
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());            /* batches in flight read the table and the lanes' indices */
  if(h->wholeKind == 2)
    h->wholeKind = 0;                          /* a refit of the last cameras batch would read another table, index array and maps */
  cameras_free(h);
  if(ncams == 0)
    return SSD_OK;
  const int W = h->P.W, H = h->P.H;
  const size_t recBytes = sizeof(CameraRec) * static_cast<size_t>(ncams);
  const size_t mapBytes = anyIntr ? static_cast<size_t>(ncams) * (static_cast<size_t>(W) + H) * sizeof(float) : 0;
  const size_t indexBytes = sizeof(int) * static_cast<size_t>(h->F);
  /* the table, its maps and every workspace's index as one group: a failure leaves the handle with no table, as cameras_free left it */
  auto bad = [&](hipError_t e, const char *what) { return hip_fail(e, std::string("ssd_set_cameras: ") + what + ": "); };
  DeviceBuf<CameraRec> dCams;
  DeviceBuf<float> dCamMaps;
  DeviceBuf<int> dIndex[kMaxLanes];
  PinnedBuf<int> hIndex[kMaxLanes];
  Event copied[kMaxLanes];
  hipError_t e = dCams.alloc(recBytes, &h->bytes);
  if(e != hipSuccess) return bad(e, "hipMalloc of the table");
  if(mapBytes)
  {
    e = dCamMaps.alloc(mapBytes, &h->bytes);
    if(e != hipSuccess) return bad(e, "hipMalloc of the deprojection maps");
    std::vector<float> all(mapBytes / sizeof(float), 0.0f), maps;
    for(int i = 0; i < ncams; i++)
      if(cams[i].has_intrinsics)
      {
        depth_maps(cams[i].intr, W, H, maps);
        std::memcpy(all.data() + static_cast<size_t>(i) * (static_cast<size_t>(W) + H), maps.data(), maps.size() * sizeof(float));
      }
    e = hipMemcpy(dCamMaps, all.data(), mapBytes, hipMemcpyHostToDevice);
    if(e != hipSuccess) return bad(e, "upload of the deprojection maps");
  }
  for(int k = 0; k < h->depth; k++)
  {
    e = dIndex[k].alloc(indexBytes, &h->bytes);
    if(e == hipSuccess) e = hIndex[k].alloc(indexBytes);
    if(e == hipSuccess) e = copied[k].create(hipEventDisableTiming);
    if(e != hipSuccess) return bad(e, "a workspace's index");
  }
  h->dCams = std::move(dCams);
  h->dCamMaps = std::move(dCamMaps);
  for(int k = 0; k < h->depth; k++)
  {
    ssd_lane &L = h->lane[k];
    L.dCamIndex = std::move(dIndex[k]); L.hCamIndex = std::move(hIndex[k]); L.camCopied = std::move(copied[k]);
  }
  h->camParams.swap(params);
  h->camHasIntr.resize(static_cast<size_t>(ncams));
  h->camDepthUnits.resize(static_cast<size_t>(ncams));
  for(int i = 0; i < ncams; i++)
  {
    h->camHasIntr[i] = cams[i].has_intrinsics ? 1 : 0;
    h->camDepthUnits[i] = cams[i].has_intrinsics ? cams[i].intr.depth_units : 0.0f;
  }
  h->camsNeedChecks = checks;
  Params P = h->P;
  P.px.groundFull = h->debug == 1 ? 1 : 0;
  const int rc = cameras_upload(h, cameras_call_key(P), P.riserTol);
  if(rc)
    cameras_free(h);
  return rc;
}

int ssd_camera_count(const ssd_handle *h)
{
  return h ? static_cast<int>(h->camParams.size()) : 0;
}

int ssd_enqueue_cameras(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                        const uint16_t *camera_of_frame, int input, uint8_t *d_labels, size_t label_stride_bytes)
{
  if(!h || !d_frames)
    return fail(SSD_E_ARG, "ssd_enqueue_cameras: null argument");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, "ssd_enqueue_cameras: nframes must be 1..max_frames_per_batch");
  int rc = check_cameras(h, "ssd_enqueue_cameras", camera_of_frame, nframes, input);
  if(rc) return rc;
  if(d_labels)
  {
    rc = check_labels_dest(h, "ssd_enqueue_cameras", d_labels, label_stride_bytes);
    if(rc) return rc;
  }
  return enqueue_impl(h, d_frames, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, input == SSD_INPUT_DEPTH16, d_labels, d_labels ? label_stride_bytes : 0,
                      camera_of_frame);
}

int ssd_enqueue_cameras_surface_moments(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                                        const uint16_t *camera_of_frame, int input, ssd_frame_moments *d_out)
{
  if(!h || !d_frames || !d_out)
    return fail(SSD_E_ARG, "ssd_enqueue_cameras_surface_moments: null argument");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, "ssd_enqueue_cameras_surface_moments: nframes must be 1..max_frames_per_batch");
  const int rc = check_cameras(h, "ssd_enqueue_cameras_surface_moments", camera_of_frame, nframes, input);
  if(rc) return rc;
  return enqueue_impl(h, d_frames, frame_stride_bytes, nframes, stream, SSD_STAGE_ALL, input == SSD_INPUT_DEPTH16, nullptr, 0, camera_of_frame, d_out);
}

int ssd_process_host_cameras(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                             ssd_frame_result *results, uint8_t *labels)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras", h && frames && results, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_impl(h, frames, nframes, input, results, staged_labels(h, labels), camera_of_frame);
}

/* the calibration a set of kernel constants was made from (make_params), as the constants hold it */
static ssd_calibration calibration_of(const Params &P)
{
  ssd_calibration c;
  for(int i = 0; i < 9; i++) c.a[i] = P.pt.a[i];
  for(int i = 0; i < 3; i++) c.b[i] = P.pt.b[i];
  for(int i = 0; i < 4; i++) c.r2[i] = P.r2[i];
  c.t2[0] = P.t2[0]; c.t2[1] = P.t2[1];
  c.world_z = P.worldZ;
  return c;
}

/* the calibration ssd_create gave the handle */
static ssd_calibration handle_calibration(const ssd_handle *h)
{
  return calibration_of(h->P);
}

/* frame i's: its camera's in a cameras batch (camOf, checked by check_cameras), the handle's otherwise */
static ssd_calibration frame_calibration(const ssd_handle *h, const uint16_t *camOf, int i)
{
  return camOf ? calibration_of(h->camParams[camOf[i]]) : handle_calibration(h);
}

/* the caller's records, or - it asked for none, the solve needs them - a vector of the call's own */
static ssd_frame_moments *moments_or_own(ssd_frame_moments *callers, std::vector<ssd_frame_moments> &own, int nframes)
{
  if(callers)
    return callers;
  own.resize(static_cast<size_t>(nframes));
  return own.data();
}

/* both host entry points of the surface fit, their refusals behind them: the batch with its moments staged out, then the solve */
static int process_host_surfaces_impl(ssd_handle *h, const void *frames, int nframes, const uint16_t *camOf, int input, ssd_frame_result *results,
                                      ssd_frame_moments *moments, int min_points, ssd_frame_surfaces *out)
{
  std::vector<ssd_frame_moments> own;
  moments = moments_or_own(moments, own, nframes);
  int rc = process_host_impl(h, frames, nframes, input, results, staged_moments(moments), camOf);
  for(int i = 0; i < nframes && !rc; i++)
  {
    const ssd_calibration cal = frame_calibration(h, camOf, i);
    rc = ssd_surface_fit_solve(moments + i, &cal, min_points, out + i);
  }
  return rc;
}

int ssd_process_host_surfaces(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                              ssd_frame_moments *moments, int min_points, ssd_frame_surfaces *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_surfaces", h && frames && results && out, nframes, input, kHandleCal);
  return rc ? rc : process_host_surfaces_impl(h, frames, nframes, nullptr, input, results, moments, min_points, out);
}

/* ---- trimmed surface refit (include/ssd_hip.h) ---------------------------------------------------------- */

/* where a pass's gates come from */
struct GateSource
{
  const ssd_frame_gates *host;                   /* the caller's gates, host memory: copied through the pinned buffer - or */
  const ssd_frame_moments *dPrev;                /* records in device memory, solved by k_surface_gates on the pass's stream (section 7i) */
  int minPoints;                                 /* ... under this rule */
  double kSigma, gateMin;
  bool cameraGate;                               /* ... and the ground gates overlaid with each camera's folded plane (section 7j), */
  int foldMinPoints;                             /* solved under this one */
};

/* the fold buffer of ssd_enqueue_cameras_surface_refit_folded and ssd_process_host_cameras_drift, on the first call of either: one record
 * per camera a table can hold, so that ssd_set_cameras never has to remake it.  One per handle, like the device gates */
static int fold_prepare(ssd_handle *h)
{
  if(h->dCamFold)
    return SSD_OK;
  const hipError_t e = h->dCamFold.alloc(sizeof(ssd_camera_fold) * static_cast<size_t>(SSD_MAX_CAMERAS), &h->bytes);
  return e == hipSuccess ? SSD_OK : hip_fail(e, "the camera fold's buffer: ");
}

/* ---- passes the handle keeps in call order (ssd_ordered_pass) ---------------------------------------------- */

/* the record's events, on first use: the one behind a call, and for a timed call the two around its span (on failure the record is as it was) */
static int pass_make(ssd_ordered_pass &p, bool timing, const std::string &me)
{
  if(!p.done)
  {
    Event done;
    const hipError_t e = done.create(hipEventDisableTiming);
    if(e != hipSuccess)
      return hip_fail(e, me + ": its event: ");
    p.done = std::move(done);
  }
  if(timing && p.ev.empty())
    HIP_TRY(make_events(p.ev, 2, hipEventDefault));
  return SSD_OK;
}

/* a call on stream s: on another stream than the call before it goes behind that one, so that calls run in the order they were made and
 * the last call's event covers every call so far */
static int pass_open(ssd_ordered_pass &p, hipStream_t s, bool timing, const std::string &me)
{
  const int rc = pass_make(p, timing, me);
  if(rc) return rc;
  if(p.haveLast && s != p.lastStream)
    HIP_TRY(hipStreamWaitEvent(s, p.done, 0));
  p.haveLast = true;
  p.lastStream = s;
  return SSD_OK;
}

/* where the timed span of a timed call starts */
static int pass_start(ssd_ordered_pass &p, hipStream_t s, bool timing)
{
  if(timing) HIP_TRY(hipEventRecord(p.ev[0], s));
  return SSD_OK;
}

/* ... and the call's end */
static int pass_close(ssd_ordered_pass &p, hipStream_t s, bool timing)
{
  if(timing) HIP_TRY(hipEventRecord(p.ev[1], s));
  p.timed = timing;
  HIP_TRY(hipEventRecord(p.done, s));
  return SSD_OK;
}

/* the host waits for the last call (ssd_fetch_*; `none`: the refusal where there was no call); p: null with a null handle */
static int pass_wait(ssd_handle *h, ssd_ordered_pass *p, const char *who, const char *none)
{
  if(!h)
    return fail(SSD_E_ARG, std::string(who) + ": null handle");
  if(!p->haveLast)
    return fail(SSD_E_ARG, std::string(who) + ": " + none);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipEventSynchronize(p->done));
  return SSD_OK;
}
static int pass_wait(ssd_handle *h, ssd_ordered_pass ssd_handle::*pass, const char *who, const char *none)
{
  return pass_wait(h, h ? &(h->*pass) : nullptr, who, none);
}

/* the milliseconds of the last call's timed span, 0 where it was not timed (ssd_get_*_time; enqueue: the pass's entry point, for the refusal) */
static int pass_time(ssd_handle *h, ssd_ordered_pass *pass, const char *who, const char *enqueue, float *ms)
{
  if(!h || !ms)
    return fail(SSD_E_ARG, std::string(who) + ": null");
  ssd_ordered_pass &p = *pass;
  if(!p.haveLast)
    return fail(SSD_E_ARG, std::string(who) + ": no " + enqueue + " yet");
  *ms = 0.0f;
  if(!p.timed)
    return SSD_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipEventSynchronize(p.ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, p.ev[0], p.ev[1]));
  return SSD_OK;
}
static int pass_time(ssd_handle *h, ssd_ordered_pass ssd_handle::*pass, const char *who, const char *enqueue, float *ms)
{
  return pass_time(h, h ? &(h->*pass) : nullptr, who, enqueue, ms);
}

/* ---- stand-alone frame passes: their records and their uploaded tables (ssd_pass_records, ssd_upload_table) ---- */

extern "C++"
{
/* the records' two buffers for F of them, on the pass's first call; countPinned: the pinned side goes into the workspace's bytes too */
template<class Rec>
static int records_prepare(ssd_handle *h, ssd_pass_records<Rec> &r, bool countPinned, const char *enqueue)
{
  if(r.d)
    return SSD_OK;
  const size_t bytes = sizeof(Rec) * static_cast<size_t>(h->F);
  DeviceBuf<Rec> d;
  PinnedBuf<Rec> hh;
  hipError_t e = d.alloc(bytes, &h->bytes);
  if(e == hipSuccess) e = hh.alloc(bytes, countPinned ? &h->bytes : nullptr);
  if(e != hipSuccess)
    return hip_fail(e, std::string(enqueue) + ": its buffers: ");
  r.d = std::move(d); r.h = std::move(hh);
  return SSD_OK;
}

/* n records zeroed on the stream, in front of the kernel that adds into them */
template<class Rec>
static int records_zero(ssd_pass_records<Rec> &r, int n, hipStream_t s)
{
  HIP_TRY(hipMemsetAsync(r.d, 0, sizeof(Rec) * static_cast<size_t>(n), s));
  return SSD_OK;
}

/* ... and behind it: the launch's error, the n records on their way to the pinned side, the call's end */
template<class Rec>
static int records_finish(ssd_pass_records<Rec> &r, int n, hipStream_t s, bool timing)
{
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(r.h, r.d, sizeof(Rec) * static_cast<size_t>(n), hipMemcpyDeviceToHost, s));
  r.count = n;
  return pass_close(r.pass, s, timing);
}

/* what a fetch begins with: the refusals (unit: what n counts, "frame" or "group"), then the host waits for the last call; the first n
 * records then stand in r.h */
template<class Rec>
static int records_wait(ssd_handle *h, ssd_pass_records<Rec> ssd_handle::*recs, const void *out, int n, const char *who, const char *enqueue, const char *unit)
{
  if(!h || !out)
    return fail(SSD_E_ARG, std::string(who) + ": null argument");
  ssd_pass_records<Rec> &r = h->*recs;
  if(!r.pass.haveLast || n < 1 || n > r.count)
    return fail(SSD_E_ARG, std::string(who) + ": n" + unit + "s must be 1..the " + unit + "s of the last " + enqueue);
  return pass_wait(h, &r.pass, who, "");
}

/* a whole fetch: the first n records of the last call, copied out */
template<class Rec>
static int records_fetch(ssd_handle *h, ssd_pass_records<Rec> ssd_handle::*recs, Rec *out, int n, const char *who, const char *enqueue, const char *unit)
{
  const int rc = records_wait(h, recs, out, n, who, enqueue, unit);
  if(rc) return rc;
  std::memcpy(out, (h->*recs).h, sizeof(Rec) * static_cast<size_t>(n));
  return SSD_OK;
}

/* a table's two buffers for n entries and its event, on first use; countPinned as records_prepare's */
template<class T>
static int table_prepare(ssd_handle *h, ssd_upload_table<T> &t, size_t n, bool countPinned, const char *enqueue)
{
  if(t.d)
    return SSD_OK;
  ssd_upload_table<T> made;
  hipError_t e = made.d.alloc(sizeof(T) * n, &h->bytes);
  if(e == hipSuccess) e = made.h.alloc(sizeof(T) * n, countPinned ? &h->bytes : nullptr);
  if(e == hipSuccess) e = made.copied.create(hipEventDisableTiming);
  if(e != hipSuccess)
    return hip_fail(e, std::string(enqueue) + ": its buffers: ");
  t = std::move(made);
  return SSD_OK;
}

/* before the pinned side is rewritten: the previous call's copy of it has gone over */
template<class T>
static int table_wait(ssd_upload_table<T> &t)
{
  if(t.sent)
    HIP_TRY(hipEventSynchronize(t.copied));
  return SSD_OK;
}

/* the first n entries to the device on the stream.  Alone only for the first table of a call that sends two, in front of the second one's
 * table_send on the same stream: that event lies behind both copies, and the call waits for it alone (an event of its own costs the call
 * microseconds) */
template<class T>
static int table_copy(ssd_upload_table<T> &t, size_t n, hipStream_t s)
{
  HIP_TRY(hipMemcpyAsync(t.d, t.h, sizeof(T) * n, hipMemcpyHostToDevice, s));
  return SSD_OK;
}

/* ... and the event behind them */
template<class T>
static int table_send(ssd_upload_table<T> &t, size_t n, hipStream_t s)
{
  const int rc = table_copy(t, n, s);
  if(rc) return rc;
  HIP_TRY(hipEventRecord(t.copied, s));
  t.sent = true;
  return SSD_OK;
}
} // extern "C++"

/* What a pass behind the handle's last whole enqueue is held to - the refit (section 7g, 7h), the clearance pass (section 7m) and the tread
 * grid (section 7n) alike: `cameras` = behind a whole cameras batch (wholeKind 2), under the table and the index that batch left in its
 * workspace; otherwise behind a whole run under the handle's calibration (wholeKind 1).  verb: what the pass does to the enqueue, oneCal /
 * cams: the entry points of either kind, for the messages; needResults: the pass reads the batch's result records. */
struct BehindWhole
{
  const char *verb, *oneCal, *cams;
  bool needResults;
};

/* what the entry of such a pass hands to its launches */
struct FollowPass
{
  ssd_lane *L;                                   /* the workspace of the batch */
  hipStream_t s;                                 /* the stream the pass runs on */
  bool timing;                                   /* this call is timed */
  CameraSel camSel;                              /* (B points into it) */
  std::optional<Batch> B;                        /* set by follow_enter */
  int chunk;                                     /* the labels' */
};

extern "C++"
{
/* The entry of a pass behind the handle's last whole enqueue, the pass's own refusals behind it.  The refusals (SSD_E_ARG, or SSD_E_HIP
 * for a handle that is not whole, before anything is launched or copied), the record's events on first use, then the stream: the caller's
 * with one workspace (a switch of streams is ordered by the lane's event), the lane's own with several (behind what the caller's stream
 * holds now, as an enqueue is).  `first(s)`, if any, is the pass's own first-use work and waits, in front of pass_open on that stream. */
template<class First>
static int follow_enter(ssd_handle *h, const std::string &me, const BehindWhole &w, ssd_ordered_pass ssd_handle::*pass, bool cameras, const void *d_frames,
                        size_t frame_stride_bytes, int nframes, void *stream, int input, FollowPass &f, First first)
{
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, me + ": input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  const bool depthInput = input == SSD_INPUT_DEPTH16;
  if(cameras)
  {
    if(h->wholeKind == 1)
      return fail(SSD_E_ARG, me + ": the last enqueue was a one-calibration batch, not a cameras batch (" + w.oneCal + " " + w.verb + "s those)");
    if(h->wholeKind != 2)
      return fail(SSD_E_ARG, me + ": no whole cameras enqueue to " + w.verb + " (none yet, the last one was a partial run, or ssd_set_cameras withdrew it)");
  }
  else
  {
    if(depthInput && !h->haveIntr)
      return fail(SSD_E_ARG, me + ": depth input: call ssd_set_intrinsics first");
    if(h->wholeKind == 2)
      return fail(SSD_E_ARG, me + ": the last enqueue was a cameras batch (" + w.cams + " " + w.verb + "s those)");
    if(h->wholeKind != 1)
      return fail(SSD_E_ARG, me + ": no whole enqueue to " + w.verb + " (none yet, or the last one was a partial run)");
  }
  if(nframes != h->lastFrames)
    return fail(SSD_E_ARG, me + ": nframes is not the last enqueue's");
  if(depthInput != h->wholeDepth || d_frames != h->wholeFrames || frame_stride_bytes != h->wholeStride)
    return fail(SSD_E_ARG, me + ": input, frames or stride are not the last enqueue's");
  ssd_lane &L = h->lane[h->lastLane];
  if(!L.haveLast || !L.dState || !L.dTileMasks || (!cameras && depthInput && !h->dDepthMaps) || (cameras && (!h->dCams || !L.dCamIndex)))
    return fail(SSD_E_HIP, me + ": the handle's workspace is incomplete (internal)");
  if(w.needResults && !h->wholeResults)
    return fail(SSD_E_HIP, me + ": the last enqueue's result records are missing (internal)");
  HIP_TRY(hipSetDevice(h->device));
  f.L = &L;
  f.timing = h->timing && !h->ev.empty();
  int rc = pass_make(h->*pass, f.timing, me);
  if(rc) return rc;
  rc = lane_stream(h, L, static_cast<hipStream_t>(stream), f.s);       /* (L.haveLast: refused above otherwise) */
  if(rc) return rc;
  rc = first(f.s);
  if(!rc) rc = pass_open(h->*pass, f.s, f.timing, me);
  if(rc) return rc;
  /* a cameras batch: the table as the batch read it, the index where the batch's own copy left it */
  f.camSel = CameraSel{ h->dCams, L.dCamIndex, h->camsNeedChecks };
  f.B.emplace(make_batch(h, h->P, L, d_frames, frame_stride_bytes, nframes, depthInput, f.s, cameras ? &f.camSel : nullptr));
  f.chunk = chunk_plan(h->tune, h->P.nPoints, nframes).chunk;
  return SSD_OK;
}

} // extern "C++"

/* ... and its exit, behind the pass's last launch.  The workspace is in use until here: whatever takes it next, on whichever stream, goes
 * behind the pass */
static int follow_leave(ssd_handle *h, ssd_ordered_pass ssd_handle::*pass, const FollowPass &f)
{
  const int rc = pass_close(h->*pass, f.s, f.timing);
  if(rc) return rc;
  HIP_TRY(hipEventRecord(f.L->done, f.s));
  f.L->lastStream = f.s;
  return SSD_OK;
}

static int no_first_use(hipStream_t) { return SSD_OK; }

static const BehindWhole kRefitBehind{ "refit", "ssd_enqueue_surface_refit", "ssd_enqueue_cameras_surface_refit", false };

/* all refit entry points */
static int refit_enqueue_impl(ssd_handle *h, const char *who, bool cameras, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                              int input, const GateSource &gates, ssd_frame_moments *d_out)
{
  const std::string me(who);
  if(!h || !d_frames || (!gates.host && !gates.dPrev) || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  if(gates.dPrev)
  {
    const int rule = check_gate_rule(who, gates.kSigma, gates.gateMin);
    if(rule) return rule;
  }
  ssd_ordered_pass &P = h->refitPass;
  FollowPass f;
  /* The device gates are one set, which is why the refit is an ordered pass: on another stream than the previous pass's (another
   * workspace's, or the caller changed streams) this call goes behind that pass, which still reads them - so refits run in the order of
   * their calls, whatever workspace they follow.  Its own: the buffers, and the pinned gates of the previous call gone over */
  int rc = follow_enter(h, me, kRefitBehind, &ssd_handle::refitPass, cameras, d_frames, frame_stride_bytes, nframes, stream, input, f, [&](hipStream_t)
  {
    int own = table_prepare(h, h->refitGates, static_cast<size_t>(h->F), true, "ssd_enqueue_surface_refit");
    if(!own && gates.cameraGate) own = fold_prepare(h);
    if(!own && gates.host) own = table_wait(h->refitGates);
    return own;
  });
  if(rc) return rc;
  ssd_lane &L = *f.L;
  hipStream_t s = f.s;
  if(gates.host)
  {
    std::memcpy(h->refitGates.h, gates.host, sizeof(ssd_frame_gates) * static_cast<size_t>(nframes));
    rc = table_send(h->refitGates, static_cast<size_t>(nframes), s);
    if(!rc) rc = pass_start(P, s, f.timing);
    if(rc) return rc;
  }
  else
  {
    /* the gates on the device, in front of the zeroing (d_prev may be d_out): no copy, no wait; the pass's time includes the kernel */
    rc = pass_start(P, s, f.timing);
    if(rc) return rc;
    launch_surface_gates(gates.dPrev, nframes, gates.minPoints, gates.kSigma, gates.gateMin, h->refitGates.d, s);
    HIP_TRY(hipGetLastError());
    if(gates.cameraGate)
    {
      /* section 7j: the fold of the same records under the batch's own index and the table's count, then each camera's plane over its
       * frames' ground gates.  The fold buffer is single like the gates, and ordered with them */
      const int ncams = static_cast<int>(h->camParams.size());
      launch_camera_fold(gates.dPrev, L.dCamIndex, nframes, ncams, false, h->dCamFold, s);
      HIP_TRY(hipGetLastError());
      launch_camera_ground_gates(gates.dPrev, L.dCamIndex, nframes, h->dCamFold, ncams, gates.foldMinPoints, gates.kSigma, gates.gateMin, h->refitGates.d, s);
      HIP_TRY(hipGetLastError());
    }
  }
  HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(ssd_frame_moments) * static_cast<size_t>(nframes), s));
  launch_surface_refit(*f.B, f.chunk, h->refitGates.d, d_out);
  HIP_TRY(hipGetLastError());
  return follow_leave(h, &ssd_handle::refitPass, f);
}

int ssd_enqueue_surface_refit(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                              int input, const ssd_frame_gates *gates, ssd_frame_moments *d_out)
{
  return refit_enqueue_impl(h, "ssd_enqueue_surface_refit", false, d_frames, frame_stride_bytes, nframes, stream, input,
                            GateSource{ gates, nullptr, 0, 0.0, 0.0, false, 0 }, d_out);
}

int ssd_enqueue_cameras_surface_refit(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                                      int input, const ssd_frame_gates *gates, ssd_frame_moments *d_out)
{
  return refit_enqueue_impl(h, "ssd_enqueue_cameras_surface_refit", true, d_frames, frame_stride_bytes, nframes, stream, input,
                            GateSource{ gates, nullptr, 0, 0.0, 0.0, false, 0 }, d_out);
}

/* ---- surface gates on the device (include/ssd_hip.h) ---------------------------------------------------- */

int ssd_enqueue_surface_gates(ssd_handle *h, const ssd_frame_moments *d_moments, int nframes, void *stream, int min_points, double k_sigma,
                              double gate_min, ssd_frame_gates *d_gates)
{
  if(!h || !d_moments || !d_gates)
    return fail(SSD_E_ARG, "ssd_enqueue_surface_gates: null argument");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, "ssd_enqueue_surface_gates: nframes must lie in 1 .. max_frames_per_batch");
  const int rc = check_gate_rule("ssd_enqueue_surface_gates", k_sigma, gate_min);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  launch_surface_gates(d_moments, nframes, min_points, k_sigma, gate_min, d_gates, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SSD_OK;
}

int ssd_enqueue_surface_refit_device(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                     const ssd_frame_moments *d_prev, int min_points, double k_sigma, double gate_min, ssd_frame_moments *d_out)
{
  return refit_enqueue_impl(h, "ssd_enqueue_surface_refit_device", false, d_frames, frame_stride_bytes, nframes, stream, input,
                            GateSource{ nullptr, d_prev, min_points, k_sigma, gate_min, false, 0 }, d_out);
}

int ssd_enqueue_cameras_surface_refit_device(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                             const ssd_frame_moments *d_prev, int min_points, double k_sigma, double gate_min,
                                             ssd_frame_moments *d_out)
{
  return refit_enqueue_impl(h, "ssd_enqueue_cameras_surface_refit_device", true, d_frames, frame_stride_bytes, nframes, stream, input,
                            GateSource{ nullptr, d_prev, min_points, k_sigma, gate_min, false, 0 }, d_out);
}

/* ---- camera fold on the device (include/ssd_hip.h) -------------------------------------------------------- */

static int check_fold_args(const ssd_handle *h, const char *who, bool pointers, int nframes, int ncams)
{
  if(!pointers)
    return fail(SSD_E_ARG, std::string(who) + ": null argument");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, std::string(who) + ": nframes must lie in 1 .. max_frames_per_batch");
  if(ncams < 1 || ncams > SSD_MAX_CAMERAS)
    return fail(SSD_E_ARG, std::string(who) + ": ncams must be 1.." + std::to_string(SSD_MAX_CAMERAS));
  return SSD_OK;
}

int ssd_enqueue_camera_fold(ssd_handle *h, const ssd_frame_moments *d_moments, const int32_t *d_camera_of_frame, int nframes, int ncams,
                            int accumulate, void *stream, ssd_camera_fold *d_fold)
{
  const int rc = check_fold_args(h, "ssd_enqueue_camera_fold", h && d_moments && d_camera_of_frame && d_fold, nframes, ncams);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  launch_camera_fold(d_moments, d_camera_of_frame, nframes, ncams, accumulate != 0, d_fold, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SSD_OK;
}

int ssd_enqueue_camera_ground_gates(ssd_handle *h, const ssd_frame_moments *d_moments, const int32_t *d_camera_of_frame, int nframes,
                                    const ssd_camera_fold *d_fold, int ncams, int fold_min_points, double k_sigma, double gate_min,
                                    void *stream, ssd_frame_gates *d_gates)
{
  int rc = check_fold_args(h, "ssd_enqueue_camera_ground_gates", h && d_moments && d_camera_of_frame && d_fold && d_gates, nframes, ncams);
  if(!rc) rc = check_gate_rule("ssd_enqueue_camera_ground_gates", k_sigma, gate_min);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  launch_camera_ground_gates(d_moments, d_camera_of_frame, nframes, d_fold, ncams, fold_min_points, k_sigma, gate_min, d_gates,
                             static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return SSD_OK;
}

int ssd_enqueue_cameras_surface_refit_folded(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                             const ssd_frame_moments *d_prev, int min_points, double k_sigma, double gate_min,
                                             int fold_min_points, ssd_frame_moments *d_out)
{
  return refit_enqueue_impl(h, "ssd_enqueue_cameras_surface_refit_folded", true, d_frames, frame_stride_bytes, nframes, stream, input,
                            GateSource{ nullptr, d_prev, min_points, k_sigma, gate_min, true, fold_min_points }, d_out);
}

int ssd_fetch_surface_refit(ssd_handle *h, void *)
{
  return pass_wait(h, &ssd_handle::refitPass, "ssd_fetch_surface_refit", "no ssd_enqueue_surface_refit to wait for");
}

int ssd_get_surface_refit_time(ssd_handle *h, float *ms)
{
  return pass_time(h, &ssd_handle::refitPass, "ssd_get_surface_refit_time", "ssd_enqueue_surface_refit", ms);
}

/* both host entry points, the caller's own refusals behind them: camOf (checked by check_cameras) = a cameras batch, each slice with its
 * part of the index, its refit passes under the cameras, each frame solved against its own camera */
static int process_host_refit_impl(ssd_handle *h, const char *who, const void *frames, int nframes, const uint16_t *camOf, int input,
                                   ssd_frame_result *results, ssd_frame_moments *first, ssd_frame_moments *refit, int min_points,
                                   double k_sigma, double gate_min, int passes, ssd_frame_surfaces *out, bool deviceGates)
{
  if(passes < 1 || passes > 4)
    return fail(SSD_E_ARG, std::string(who) + ": passes must lie in 1 .. 4");
  int rc = check_gate_rule(who, k_sigma, gate_min);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForPipeline), frames, nframes };
  rc = feed.prepare();
  if(rc) return rc;
  /* the records of a slice on the device: the first pass's in the first label staging buffer, a refit pass's in the second */
  rc = labels_prepare(h, static_cast<size_t>(feed.slice) * sizeof(ssd_frame_moments));
  if(rc) return rc;
  ssd_frame_moments *dFirst = reinterpret_cast<ssd_frame_moments *>(h->labelStage[0].get()), *dRefit = reinterpret_cast<ssd_frame_moments *>(h->labelStage[1].get());
  std::vector<ssd_frame_moments> cur(static_cast<size_t>(feed.slice));
  std::vector<ssd_frame_gates> gates(static_cast<size_t>(feed.slice));
  /* the records of the pass that ran last on the slice's stream, to the host */
  auto records = [&](const ssd_frame_moments *d, int n)
  {
    hipStream_t s = h->lane[h->lastLane].lastStream;
    HIP_TRY(hipMemcpyAsync(cur.data(), d, sizeof(ssd_frame_moments) * static_cast<size_t>(n), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return static_cast<int>(SSD_OK);
  };
  for(int c = 0; c < feed.slices(); c++)
  {
    const void *buf;
    int done, n;
    /* the body blocks on every pass, so the next slice's copy goes out in front of it, beside this slice's kernels */
    rc = feed.stage(c);
    if(!rc) rc = feed.stage(c + 1);
    if(!rc) rc = feed.ready(c, buf, done, n);
    if(rc) return rc;
    rc = enqueue_impl(h, buf, feed.f.devFrameBytes, n, h->ingestCompute, SSD_STAGE_ALL, feed.f.depth, nullptr, 0, camOf ? camOf + done : nullptr, dFirst);
    if(rc) return rc;
    if(deviceGates)
    {
      /* section 7i: the passes go out behind the enqueue with no host step between - the first gated by dFirst's planes into dRefit,
       * the later ones in place.  Then the slice's results and, behind the last pass on its stream, its records */
      for(int pass = 0; pass < passes; pass++)
      {
        rc = refit_enqueue_impl(h, who, camOf != nullptr, buf, feed.f.devFrameBytes, n, h->ingestCompute, input,
                                GateSource{ nullptr, pass == 0 ? dFirst : dRefit, min_points, k_sigma, gate_min, false, 0 }, dRefit);
        if(rc) return rc;
      }
      rc = ssd_fetch_back(h, results + done, n, 0);
      if(rc) return rc;
      if(first)
      {
        rc = records(dFirst, n);
        if(rc) return rc;
        std::memcpy(first + done, cur.data(), sizeof(ssd_frame_moments) * static_cast<size_t>(n));
      }
      rc = records(dRefit, n);
      if(rc) return rc;
    }
    else
    {
      rc = ssd_fetch_back(h, results + done, n, 0);
      if(rc) return rc;
      rc = records(dFirst, n);
      if(rc) return rc;
      if(first)
        std::memcpy(first + done, cur.data(), sizeof(ssd_frame_moments) * static_cast<size_t>(n));
      for(int pass = 0; pass < passes; pass++)
      {
        for(int i = 0; i < n; i++)
        {
          rc = ssd_surface_gates_from_moments(&cur[i], min_points, k_sigma, gate_min, &gates[i]);
          if(rc) return rc;
        }
        rc = refit_enqueue_impl(h, who, camOf != nullptr, buf, feed.f.devFrameBytes, n, h->ingestCompute, input,
                                GateSource{ gates.data(), nullptr, 0, 0.0, 0.0, false, 0 }, dRefit);
        if(rc) return rc;
        rc = ssd_fetch_surface_refit(h, nullptr);
        if(rc) return rc;
        rc = records(dRefit, n);
        if(rc) return rc;
      }
    }
    /* the buffer's last reader was the last pass, on the slice's stream (which the body has waited for: the record costs nothing) */
    rc = feed.consumed(c, h->lane[h->lastLane].lastStream);
    if(rc) return rc;
    if(refit)
      std::memcpy(refit + done, cur.data(), sizeof(ssd_frame_moments) * static_cast<size_t>(n));
    for(int i = 0; i < n; i++)
    {
      const ssd_calibration own = frame_calibration(h, camOf, done + i);
      rc = ssd_surface_fit_solve(&cur[i], &own, min_points, out + done + i);
      if(rc) return rc;
    }
  }
  return SSD_OK;
}

int ssd_process_host_surfaces_refit(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                                    ssd_frame_moments *first, ssd_frame_moments *refit, int min_points, double k_sigma, double gate_min,
                                    int passes, ssd_frame_surfaces *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_surfaces_refit", h && frames && results && out, nframes, input, kHandleCal);
  return rc ? rc : process_host_refit_impl(h, "ssd_process_host_surfaces_refit", frames, nframes, nullptr, input, results, first, refit, min_points, k_sigma,
                                           gate_min, passes, out, false);
}

int ssd_process_host_surfaces_refit_device(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                                           ssd_frame_moments *first, ssd_frame_moments *refit, int min_points, double k_sigma, double gate_min,
                                           int passes, ssd_frame_surfaces *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_surfaces_refit_device", h && frames && results && out, nframes, input, kHandleCal);
  return rc ? rc : process_host_refit_impl(h, "ssd_process_host_surfaces_refit_device", frames, nframes, nullptr, input, results, first, refit, min_points,
                                           k_sigma, gate_min, passes, out, true);
}

/* ---- surface fit of cameras batches and drift per camera (include/ssd_hip.h) ---------------------------- */

int ssd_process_host_cameras_surfaces(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                      ssd_frame_result *results, ssd_frame_moments *moments, int min_points, ssd_frame_surfaces *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras_surfaces", h && frames && results && out, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_surfaces_impl(h, frames, nframes, camera_of_frame, input, results, moments, min_points, out);
}

/* ---- trimmed refit of cameras batches (include/ssd_hip.h) -------------------------------------------------- */

int ssd_process_host_cameras_surfaces_refit(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                            ssd_frame_result *results, ssd_frame_moments *first, ssd_frame_moments *refit, int min_points,
                                            double k_sigma, double gate_min, int passes, ssd_frame_surfaces *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras_surfaces_refit", h && frames && results && out, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_refit_impl(h, "ssd_process_host_cameras_surfaces_refit", frames, nframes, camera_of_frame, input, results, first, refit,
                                           min_points, k_sigma, gate_min, passes, out, false);
}

int ssd_process_host_cameras_surfaces_refit_device(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                                   ssd_frame_result *results, ssd_frame_moments *first, ssd_frame_moments *refit, int min_points,
                                                   double k_sigma, double gate_min, int passes, ssd_frame_surfaces *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras_surfaces_refit_device", h && frames && results && out, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_refit_impl(h, "ssd_process_host_cameras_surfaces_refit_device", frames, nframes, camera_of_frame, input, results, first, refit,
                                           min_points, k_sigma, gate_min, passes, out, true);
}

/* The drift watch with the fold on the device: process_host_refit_impl's device-gated slices with an accumulating
 * k_camera_fold behind each slice's last pass where that function copies the records out, and one copy of the table's fold at the end */
int ssd_process_host_cameras_drift(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                   ssd_frame_result *results, int min_points, double k_sigma, double gate_min, int passes, int fold_min_points,
                                   ssd_camera_drift *out)
{
  const char *who = "ssd_process_host_cameras_drift";
  int rc = check_host_batch(h, who, h && frames && results && out, nframes, input, kCameraTable, camera_of_frame);
  if(rc) return rc;
  if(passes < 0 || passes > 4)
    return fail(SSD_E_ARG, std::string(who) + ": passes must lie in 0 .. 4");
  rc = check_gate_rule(who, k_sigma, gate_min);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForPipeline), frames, nframes };
  rc = feed.prepare();
  if(rc) return rc;
  rc = labels_prepare(h, static_cast<size_t>(feed.slice) * sizeof(ssd_frame_moments));
  if(!rc) rc = fold_prepare(h);
  if(rc) return rc;
  if(h->refitPass.haveLast)
    HIP_TRY(hipEventSynchronize(h->refitPass.done));                /* a folded pass still on its way owns the fold buffer */
  ssd_frame_moments *dFirst = reinterpret_cast<ssd_frame_moments *>(h->labelStage[0].get()), *dRefit = reinterpret_cast<ssd_frame_moments *>(h->labelStage[1].get());
  const int ncams = static_cast<int>(h->camParams.size());
  hipStream_t s = nullptr;
  for(int c = 0; c < feed.slices(); c++)
  {
    const void *buf;
    int done, n;
    rc = feed.stage(c);
    if(!rc) rc = feed.stage(c + 1);
    if(!rc) rc = feed.ready(c, buf, done, n);
    if(rc) return rc;
    rc = enqueue_impl(h, buf, feed.f.devFrameBytes, n, h->ingestCompute, SSD_STAGE_ALL, feed.f.depth, nullptr, 0, camera_of_frame + done, dFirst);
    if(rc) return rc;
    for(int pass = 0; pass < passes; pass++)
    {
      rc = refit_enqueue_impl(h, who, true, buf, feed.f.devFrameBytes, n, h->ingestCompute, input,
                              GateSource{ nullptr, pass == 0 ? dFirst : dRefit, min_points, k_sigma, gate_min, false, 0 }, dRefit);
      if(rc) return rc;
    }
    /* the slice's last records onto the table's fold, behind them on the stream they were made on, under the index the enqueue left in
     * its workspace.  The slice is then waited for: the next one writes the same two record buffers, and folds into the same records */
    const ssd_lane &L = h->lane[h->lastLane];
    s = L.lastStream;
    launch_camera_fold(passes ? dRefit : dFirst, L.dCamIndex, n, ncams, c > 0, h->dCamFold, s);
    HIP_TRY(hipGetLastError());
    rc = ssd_fetch_back(h, results + done, n, 0);
    if(rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    rc = feed.consumed(c, s);
    if(rc) return rc;
  }
  std::vector<ssd_camera_fold> fold(static_cast<size_t>(ncams));
  HIP_TRY(hipMemcpyAsync(fold.data(), h->dCamFold, sizeof(ssd_camera_fold) * fold.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::vector<ssd_camera> cams(static_cast<size_t>(ncams));
  for(int c = 0; c < ncams; c++)
  {
    std::memset(&cams[c], 0, sizeof(ssd_camera));
    cams[c].cal = calibration_of(h->camParams[c]);
  }
  return ssd_camera_drift_from_fold(fold.data(), cams.data(), ncams, fold_min_points, out);
}

/* ---- tread clearance (include/ssd_hip.h) ------------------------------------------------------------------ */

static const BehindWhole kClearanceBehind{ "clear", "ssd_enqueue_clearance", "ssd_enqueue_cameras_clearance", true };

/* both entry points of the pass: its own refusals, then the shared entry's, before anything is launched */
static int clearance_enqueue_impl(ssd_handle *h, const char *who, bool cameras, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                                  int input, const ssd_clearance_rule *rule, ssd_frame_moments *d_out, uint8_t *d_mask, size_t mask_stride)
{
  const std::string me(who);
  if(!h || !d_frames || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  int rc = check_clearance_rule(me, rule);
  if(rc) return rc;
  if(d_mask && mask_stride < static_cast<size_t>(h->P.nPoints))
    return fail(SSD_E_ARG, me + ": mask_stride is smaller than width * height");
  FollowPass f;
  rc = follow_enter(h, me, kClearanceBehind, &ssd_handle::clearPass, cameras, d_frames, frame_stride_bytes, nframes, stream, input, f, no_first_use);
  if(!rc) rc = pass_start(h->clearPass, f.s, f.timing);
  if(rc) return rc;
  HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(ssd_frame_moments) * static_cast<size_t>(nframes), f.s));
  if(d_mask)
  {
    /* only the bytes below width * height of every stride are the pass's */
    if(mask_stride == static_cast<size_t>(h->P.nPoints))
      HIP_TRY(hipMemsetAsync(d_mask, 0, mask_stride * static_cast<size_t>(nframes), f.s));
    else
      HIP_TRY(hipMemset2DAsync(d_mask, mask_stride, 0, static_cast<size_t>(h->P.nPoints), static_cast<size_t>(nframes), f.s));
  }
  launch_clearance(*f.B, f.chunk, h->wholeResults, *rule, d_out, d_mask, mask_stride);
  HIP_TRY(hipGetLastError());
  return follow_leave(h, &ssd_handle::clearPass, f);
}

int ssd_enqueue_clearance(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                          const ssd_clearance_rule *rule, ssd_frame_moments *d_out, uint8_t *d_mask, size_t mask_stride)
{
  return clearance_enqueue_impl(h, "ssd_enqueue_clearance", false, d_frames, frame_stride_bytes, nframes, stream, input, rule, d_out, d_mask, mask_stride);
}

int ssd_enqueue_cameras_clearance(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                  const ssd_clearance_rule *rule, ssd_frame_moments *d_out, uint8_t *d_mask, size_t mask_stride)
{
  return clearance_enqueue_impl(h, "ssd_enqueue_cameras_clearance", true, d_frames, frame_stride_bytes, nframes, stream, input, rule, d_out, d_mask, mask_stride);
}

int ssd_fetch_clearance(ssd_handle *h, void *)
{
  return pass_wait(h, &ssd_handle::clearPass, "ssd_fetch_clearance", "no ssd_enqueue_clearance to wait for");
}

int ssd_get_clearance_time(ssd_handle *h, float *ms)
{
  return pass_time(h, &ssd_handle::clearPass, "ssd_get_clearance_time", "ssd_enqueue_clearance", ms);
}

extern "C++"
{
/* The host-fed loop of a pass behind each slice's whole enqueue (the clearance pass, the tread grid).  Per slice, while it is still in its
 * staging buffer: the enqueue, pass(buf, first, n) on the compute stream, the results, copy(first, n, s) - the pass's staged records to the host,
 * behind the pass on the stream it ran on - and solve(first, i) for each of its n frames.  The body blocks on the pass, so the next slice's
 * copy goes out in front of it, beside this slice's kernels, and the staging buffers are free for the next slice */
template<class Pass, class Copy, class Solve>
static int process_host_follow(ssd_handle *h, SliceFeed &feed, const uint16_t *camOf, ssd_frame_result *results, Pass pass, Copy copy, Solve solve)
{
  for(int c = 0; c < feed.slices(); c++)
  {
    const void *buf;
    int done, n;
    int rc = feed.stage(c);
    if(!rc) rc = feed.stage(c + 1);
    if(!rc) rc = feed.ready(c, buf, done, n);
    if(rc) return rc;
    rc = enqueue_impl(h, buf, feed.f.devFrameBytes, n, h->ingestCompute, SSD_STAGE_ALL, feed.f.depth, nullptr, 0, camOf ? camOf + done : nullptr);
    if(!rc) rc = pass(buf, done, n);
    if(!rc) rc = ssd_fetch_back(h, results + done, n, 0);
    if(rc) return rc;
    hipStream_t s = h->lane[h->lastLane].lastStream;
    rc = copy(done, n, s);
    if(rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    rc = feed.consumed(c, s);
    for(int i = 0; i < n && !rc; i++)
      rc = solve(done, i);
    if(rc) return rc;
  }
  return SSD_OK;
}

} // extern "C++"

/* both host entry points, the callers' own refusals behind them: the records go out through the first label staging buffer, the mask
 * through the second */
static int process_host_clearance_impl(ssd_handle *h, const char *who, const void *frames, int nframes, const uint16_t *camOf, int input,
                                       const ssd_clearance_rule *rule, int min_support, ssd_frame_result *results, ssd_frame_moments *moments,
                                       uint8_t *mask, ssd_frame_clearance *out)
{
  int rc = check_clearance_rule(who, rule);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForPipeline), frames, nframes };
  rc = feed.prepare();
  if(rc) return rc;
  const size_t nPoints = static_cast<size_t>(h->P.nPoints);
  const size_t recordBytes = static_cast<size_t>(feed.slice) * sizeof(ssd_frame_moments), maskBytes = mask ? static_cast<size_t>(feed.slice) * nPoints : 0;
  rc = labels_prepare(h, recordBytes > maskBytes ? recordBytes : maskBytes);
  if(rc) return rc;
  ssd_frame_moments *dRecords = reinterpret_cast<ssd_frame_moments *>(h->labelStage[0].get());
  uint8_t *dMask = mask ? h->labelStage[1].get() : nullptr;
  std::vector<ssd_frame_moments> own;
  moments = moments_or_own(moments, own, nframes);
  return process_host_follow(h, feed, camOf, results,
    [&](const void *buf, int, int n)
    {
      return clearance_enqueue_impl(h, who, camOf != nullptr, buf, feed.f.devFrameBytes, n, h->ingestCompute, input, rule, dRecords, dMask, nPoints);
    },
    [&](int first, int n, hipStream_t s)
    {
      HIP_TRY(hipMemcpyAsync(moments + first, dRecords, sizeof(ssd_frame_moments) * static_cast<size_t>(n), hipMemcpyDeviceToHost, s));
      if(mask)
        HIP_TRY(hipMemcpyAsync(mask + static_cast<size_t>(first) * nPoints, dMask, static_cast<size_t>(n) * nPoints, hipMemcpyDeviceToHost, s));
      return static_cast<int>(SSD_OK);
    },
    [&](int first, int i)
    {
      const ssd_calibration cal = frame_calibration(h, camOf, first + i);
      return ssd_clearance_solve(moments + first + i, results + first + i, &cal, min_support, out + first + i);
    });
}

int ssd_process_host_clearance(ssd_handle *h, const void *frames, int nframes, int input, const ssd_clearance_rule *rule, int min_support,
                               ssd_frame_result *results, ssd_frame_moments *moments, uint8_t *mask, ssd_frame_clearance *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_clearance", h && frames && results && out, nframes, input, kHandleCal);
  return rc ? rc : process_host_clearance_impl(h, "ssd_process_host_clearance", frames, nframes, nullptr, input, rule, min_support, results, moments, mask, out);
}

int ssd_process_host_cameras_clearance(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                       const ssd_clearance_rule *rule, int min_support, ssd_frame_result *results, ssd_frame_moments *moments,
                                       uint8_t *mask, ssd_frame_clearance *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras_clearance", h && frames && results && out, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_clearance_impl(h, "ssd_process_host_cameras_clearance", frames, nframes, camera_of_frame, input, rule, min_support, results,
                                               moments, mask, out);
}

/* ---- tread grid (include/ssd_hip.h) ----------------------------------------------------------------------- */

static const BehindWhole kTreadGridBehind{ "grid", "ssd_enqueue_tread_grid", "ssd_enqueue_cameras_tread_grid", true };

/* both entry points of the pass: its own refusals, then the shared entry's, before anything is launched */
static int tread_grid_enqueue_impl(ssd_handle *h, const char *who, bool cameras, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                                   int input, const ssd_tread_grid_rule *rule, ssd_frame_tread_grid *d_out)
{
  const std::string me(who);
  if(!h || !d_frames || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  int rc = check_tread_grid_rule(me, rule);
  if(rc) return rc;
  FollowPass f;
  rc = follow_enter(h, me, kTreadGridBehind, &ssd_handle::gridPass, cameras, d_frames, frame_stride_bytes, nframes, stream, input, f, no_first_use);
  if(!rc) rc = pass_start(h->gridPass, f.s, f.timing);
  if(rc) return rc;
  HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(ssd_frame_tread_grid) * static_cast<size_t>(nframes), f.s));
  launch_tread_grid(*f.B, f.chunk, h->wholeResults, *rule, d_out);
  HIP_TRY(hipGetLastError());
  return follow_leave(h, &ssd_handle::gridPass, f);
}

int ssd_enqueue_tread_grid(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                           const ssd_tread_grid_rule *rule, ssd_frame_tread_grid *d_out)
{
  return tread_grid_enqueue_impl(h, "ssd_enqueue_tread_grid", false, d_frames, frame_stride_bytes, nframes, stream, input, rule, d_out);
}

int ssd_enqueue_cameras_tread_grid(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                   const ssd_tread_grid_rule *rule, ssd_frame_tread_grid *d_out)
{
  return tread_grid_enqueue_impl(h, "ssd_enqueue_cameras_tread_grid", true, d_frames, frame_stride_bytes, nframes, stream, input, rule, d_out);
}

int ssd_fetch_tread_grid(ssd_handle *h, void *)
{
  return pass_wait(h, &ssd_handle::gridPass, "ssd_fetch_tread_grid", "no ssd_enqueue_tread_grid to wait for");
}

int ssd_get_tread_grid_time(ssd_handle *h, float *ms)
{
  return pass_time(h, &ssd_handle::gridPass, "ssd_get_tread_grid_time", "ssd_enqueue_tread_grid", ms);
}

/* where a slice's records are staged: the first label staging buffer if it holds them as it stands, else a buffer of the pass's own
 * (every user of either has been waited for: the bodies of the host entry points block on their slices) */
static int tread_grid_stage(ssd_handle *h, int slice, ssd_frame_tread_grid *&dRecords)
{
  if(h->labelStage[0] && h->labelStageCap >= static_cast<size_t>(slice) * sizeof(ssd_frame_tread_grid))
  {
    dRecords = reinterpret_cast<ssd_frame_tread_grid *>(h->labelStage[0].get());
    return SSD_OK;
  }
  if(h->gridStageFrames < slice)
  {
    DeviceBuf<ssd_frame_tread_grid> buf;
    const hipError_t e = buf.alloc(static_cast<size_t>(slice) * sizeof(ssd_frame_tread_grid));
    if(e != hipSuccess)
      return hip_fail(e, "the tread grid's staging buffer: ");
    h->gridStage = std::move(buf);
    h->gridStageFrames = slice;
  }
  dRecords = h->gridStage;
  return SSD_OK;
}

/* both host entry points, the callers' own refusals behind them */
static int process_host_tread_grid_impl(ssd_handle *h, const char *who, const void *frames, int nframes, const uint16_t *camOf, int input,
                                        const ssd_tread_grid_rule *rule, int min_seen, int min_occ, double foot_along, double foot_deep,
                                        ssd_frame_result *results, ssd_frame_tread_grid *grids, ssd_frame_footholds *out)
{
  int rc = check_tread_grid_rule(who, rule);
  if(rc) return rc;
  if(!(foot_along >= 0.0) || !(foot_deep >= 0.0))
    return fail(SSD_E_ARG, std::string(who) + ": a foot size must be 0 or more");
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForPipeline), frames, nframes };
  rc = feed.prepare();
  if(rc) return rc;
  ssd_frame_tread_grid *dRecords = nullptr;
  rc = tread_grid_stage(h, feed.slice, dRecords);
  if(rc) return rc;
  /* a caller that asks for no records: a slice's, solved before the next slice's replace them */
  std::vector<ssd_frame_tread_grid> own;
  if(!grids)
    own.resize(static_cast<size_t>(feed.slice));
  return process_host_follow(h, feed, camOf, results,
    [&](const void *buf, int, int n)
    {
      return tread_grid_enqueue_impl(h, who, camOf != nullptr, buf, feed.f.devFrameBytes, n, h->ingestCompute, input, rule, dRecords);
    },
    [&](int first, int n, hipStream_t s)
    {
      HIP_TRY(hipMemcpyAsync(grids ? grids + first : own.data(), dRecords, sizeof(ssd_frame_tread_grid) * static_cast<size_t>(n), hipMemcpyDeviceToHost, s));
      return static_cast<int>(SSD_OK);
    },
    [&](int first, int i)
    {
      return ssd_tread_grid_solve(grids ? grids + first + i : own.data() + i, results + first + i, rule, min_seen, min_occ, foot_along, foot_deep, out + first + i);
    });
}

int ssd_process_host_tread_grid(ssd_handle *h, const void *frames, int nframes, int input, const ssd_tread_grid_rule *rule, int min_seen,
                                int min_occ, double foot_along, double foot_deep, ssd_frame_result *results, ssd_frame_tread_grid *grids,
                                ssd_frame_footholds *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_tread_grid", h && frames && results && out, nframes, input, kHandleCal);
  return rc ? rc : process_host_tread_grid_impl(h, "ssd_process_host_tread_grid", frames, nframes, nullptr, input, rule, min_seen, min_occ, foot_along,
                                                foot_deep, results, grids, out);
}

int ssd_process_host_cameras_tread_grid(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                        const ssd_tread_grid_rule *rule, int min_seen, int min_occ, double foot_along, double foot_deep,
                                        ssd_frame_result *results, ssd_frame_tread_grid *grids, ssd_frame_footholds *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras_tread_grid", h && frames && results && out, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_tread_grid_impl(h, "ssd_process_host_cameras_tread_grid", frames, nframes, camera_of_frame, input, rule, min_seen, min_occ,
                                                foot_along, foot_deep, results, grids, out);
}

/* ---- stair map (include/ssd_hip.h) ------------------------------------------------------------------------ */

/* the refusals about the maps and the index that the enqueue and the host forms share: nframes is the whole call's, so that the bound
 * on a map's count holds over all of it */
static int check_stair_maps(const std::string &me, const ssd_handle *h, const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, int nframes)
{
  if(!maps)
    return fail(SSD_E_ARG, me + ": null maps");
  if(nmaps < 1 || nmaps > SSD_MAX_STAIR_MAPS)
    return fail(SSD_E_ARG, me + ": nmaps must lie in 1 .. SSD_MAX_STAIR_MAPS");
  for(int m = 0; m < nmaps; m++)
    if(maps[m].stairs.n_steps < 0 || maps[m].stairs.n_steps > SSD_MAX_STEPS)
      return fail(SSD_E_ARG, me + ": a map's n_steps must lie in 0 .. SSD_MAX_STEPS");
  unsigned long long named[SSD_MAX_STAIR_MAPS] = {};
  for(int i = 0; i < nframes; i++)
  {
    const unsigned int m = map_of_frame ? map_of_frame[i] : 0u;
    if(m == SSD_STAIR_MAP_NONE)
      continue;
    if(m >= static_cast<unsigned int>(nmaps))
      return fail(SSD_E_ARG, me + ": map_of_frame holds an index that is neither below nmaps nor SSD_STAIR_MAP_NONE");
    named[m]++;
  }
  /* no count of a record can pass 2^32 - 1 within the call: a frame adds at most its points to one word */
  for(int m = 0; m < nmaps; m++)
    if(named[m] * static_cast<unsigned long long>(h->P.nPoints) > 0xffffffffull)
      return fail(SSD_E_ARG, me + ": the frames that name one map hold more than 2^32 - 1 points");
  return SSD_OK;
}

static const BehindWhole kStairMapBehind{ "map", "ssd_enqueue_stair_map", "ssd_enqueue_cameras_stair_map", false };

/* both entry points of the pass and the slices of the host forms (checked: the caller has held the maps and the whole call's index to
 * check_stair_maps): its own refusals, then the shared entry's, before anything is launched or copied */
static int stair_map_enqueue_impl(ssd_handle *h, const char *who, bool cameras, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                                  int input, const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule,
                                  int accumulate, ssd_frame_tread_grid *d_out, bool checked)
{
  const std::string me(who);
  if(!h || !d_frames || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  int rc = check_tread_grid_rule(me, rule);
  if(rc) return rc;
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, me + ": nframes is not the last enqueue's");
  if(!checked)
  {
    rc = check_stair_maps(me, h, maps, nmaps, map_of_frame, nframes);
    if(rc) return rc;
  }
  ssd_ordered_pass &P = h->mapPass;
  FollowPass f;
  /* The device maps and index are one set, so the pass is an ordered one: on another stream than the previous pass's this call goes
   * behind that pass, which still reads them.  Its own: the buffers, and the pinned side of the previous call gone over */
  rc = follow_enter(h, me, kStairMapBehind, &ssd_handle::mapPass, cameras, d_frames, frame_stride_bytes, nframes, stream, input, f, [&](hipStream_t)
  {
    int own = table_prepare(h, h->stairMaps, static_cast<size_t>(SSD_MAX_STAIR_MAPS), true, "ssd_enqueue_stair_map");
    if(!own) own = table_prepare(h, h->mapIndex, static_cast<size_t>(h->F), true, "ssd_enqueue_stair_map");
    if(!own) own = table_wait(h->mapIndex);                   /* its event lies behind the maps' copy too */
    return own;
  });
  if(rc) return rc;
  hipStream_t s = f.s;
  std::memcpy(h->stairMaps.h, maps, sizeof(ssd_stair_map) * static_cast<size_t>(nmaps));
  for(int i = 0; i < nframes; i++)
    h->mapIndex.h[i] = map_of_frame ? static_cast<int>(map_of_frame[i]) : 0;
  rc = table_copy(h->stairMaps, static_cast<size_t>(nmaps), s);
  if(!rc) rc = table_send(h->mapIndex, static_cast<size_t>(nframes), s);
  if(!rc) rc = pass_start(P, s, f.timing);
  if(rc) return rc;
  if(!accumulate)
    HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(ssd_frame_tread_grid) * static_cast<size_t>(nmaps), s));
  launch_stair_map(*f.B, f.chunk, h->stairMaps.d, h->mapIndex.d, nmaps, *rule, d_out);
  HIP_TRY(hipGetLastError());
  return follow_leave(h, &ssd_handle::mapPass, f);
}

int ssd_enqueue_stair_map(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                          const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule, int accumulate,
                          ssd_frame_tread_grid *d_out)
{
  return stair_map_enqueue_impl(h, "ssd_enqueue_stair_map", false, d_frames, frame_stride_bytes, nframes, stream, input, maps, nmaps, map_of_frame, rule,
                                accumulate, d_out, false);
}

int ssd_enqueue_cameras_stair_map(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                                  const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule, int accumulate,
                                  ssd_frame_tread_grid *d_out)
{
  return stair_map_enqueue_impl(h, "ssd_enqueue_cameras_stair_map", true, d_frames, frame_stride_bytes, nframes, stream, input, maps, nmaps, map_of_frame,
                                rule, accumulate, d_out, false);
}

int ssd_fetch_stair_map(ssd_handle *h, void *)
{
  return pass_wait(h, &ssd_handle::mapPass, "ssd_fetch_stair_map", "no ssd_enqueue_stair_map to wait for");
}

int ssd_get_stair_map_time(ssd_handle *h, float *ms)
{
  return pass_time(h, &ssd_handle::mapPass, "ssd_get_stair_map_time", "ssd_enqueue_stair_map", ms);
}

/* Both host entry points, the callers' own refusals behind them: the rule, then the maps and the WHOLE call's index and bound, then the
 * foot sizes - all before a byte of `frames` is read or anything is allocated.  process_host_follow fits: its pass is a slice's enqueue
 * under the slice's part of the index (the loop hands it the slice's first frame), with accumulate on from the second slice; its copy
 * does nothing until the last slice and then takes the nmaps records; and nothing is solved per frame - the maps are solved behind the
 * loop, whose last iteration has waited for the copy */
static int process_host_stair_map_impl(ssd_handle *h, const char *who, const void *frames, int nframes, const uint16_t *camOf, int input,
                                       const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule, int min_seen,
                                       int min_occ, double foot_along, double foot_deep, ssd_frame_result *results, ssd_frame_tread_grid *grids,
                                       ssd_frame_footholds *out)
{
  int rc = check_tread_grid_rule(who, rule);
  if(rc) return rc;
  rc = check_stair_maps(who, h, maps, nmaps, map_of_frame, nframes);
  if(rc) return rc;
  if(!(foot_along >= 0.0) || !(foot_deep >= 0.0))
    return fail(SSD_E_ARG, std::string(who) + ": a foot size must be 0 or more");
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForPipeline), frames, nframes };
  rc = feed.prepare();
  if(rc) return rc;
  if(!h->mapStage)
  {
    DeviceBuf<ssd_frame_tread_grid> buf;
    const hipError_t e = buf.alloc(sizeof(ssd_frame_tread_grid) * static_cast<size_t>(SSD_MAX_STAIR_MAPS));
    if(e != hipSuccess)
      return hip_fail(e, "the stair map's staging buffer: ");
    h->mapStage = std::move(buf);
  }
  ssd_frame_tread_grid *dRecords = h->mapStage;
  std::vector<ssd_frame_tread_grid> own;
  if(!grids)
  {
    own.resize(static_cast<size_t>(nmaps));
    grids = own.data();
  }
  rc = process_host_follow(h, feed, camOf, results,
    [&](const void *buf, int first, int n)
    {
      return stair_map_enqueue_impl(h, who, camOf != nullptr, buf, feed.f.devFrameBytes, n, h->ingestCompute, input, maps, nmaps,
                                    map_of_frame ? map_of_frame + first : nullptr, rule, first != 0, dRecords, true);
    },
    [&](int first, int n, hipStream_t s)
    {
      if(first + n == nframes)
        HIP_TRY(hipMemcpyAsync(grids, dRecords, sizeof(ssd_frame_tread_grid) * static_cast<size_t>(nmaps), hipMemcpyDeviceToHost, s));
      return static_cast<int>(SSD_OK);
    },
    [](int, int) { return static_cast<int>(SSD_OK); });
  for(int m = 0; m < nmaps && !rc; m++)
    rc = ssd_tread_grid_solve(grids + m, &maps[m].stairs, rule, min_seen, min_occ, foot_along, foot_deep, out + m);
  return rc;
}

int ssd_process_host_stair_map(ssd_handle *h, const void *frames, int nframes, int input, const ssd_stair_map *maps, int nmaps,
                               const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule, int min_seen, int min_occ, double foot_along,
                               double foot_deep, ssd_frame_result *results, ssd_frame_tread_grid *grids, ssd_frame_footholds *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_stair_map", h && frames && results && out, nframes, input, kHandleCal);
  return rc ? rc : process_host_stair_map_impl(h, "ssd_process_host_stair_map", frames, nframes, nullptr, input, maps, nmaps, map_of_frame, rule, min_seen,
                                               min_occ, foot_along, foot_deep, results, grids, out);
}

int ssd_process_host_cameras_stair_map(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                       const ssd_stair_map *maps, int nmaps, const uint16_t *map_of_frame, const ssd_tread_grid_rule *rule,
                                       int min_seen, int min_occ, double foot_along, double foot_deep, ssd_frame_result *results,
                                       ssd_frame_tread_grid *grids, ssd_frame_footholds *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras_stair_map", h && frames && results && out, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_stair_map_impl(h, "ssd_process_host_cameras_stair_map", frames, nframes, camera_of_frame, input, maps, nmaps, map_of_frame,
                                               rule, min_seen, min_occ, foot_along, foot_deep, results, grids, out);
}

/* ---- riser fit (include/ssd_hip.h): host side ------------------------------------------------------------ */

/* both host entry points: the batch through process_host_impl with the riser moments on, then the riser records, the moments, the solve */
static int process_host_riser_fits_impl(ssd_handle *h, const char *who, const void *frames, int nframes, const uint16_t *camOf, int input,
                                        ssd_frame_result *results, ssd_frame_risers *risers, ssd_frame_moments *moments, int min_points,
                                        ssd_frame_riser_fits *out)
{
  if(!h->P.risers || !h->dRisers)
    return fail(SSD_E_ARG, std::string(who) + ": call ssd_set_risers(h, 1, ...) first");
  std::vector<ssd_frame_moments> own;
  moments = moments_or_own(moments, own, nframes);
  const bool was = h->riserMoments;
  int rc = ssd_set_riser_moments(h, 1);
  if(rc) return rc;
  rc = process_host_impl(h, frames, nframes, input, results, StagedOut{}, camOf);
  if(!rc) rc = ssd_fetch_risers(h, risers, nframes, nullptr);
  if(!rc) rc = ssd_fetch_riser_moments(h, moments, nframes, nullptr);
  h->riserMoments = was;                      /* the call has returned its batches: nothing is in flight */
  if(rc) return rc;
  for(int i = 0; i < nframes; i++)
  {
    const ssd_calibration cal = frame_calibration(h, camOf, i);
    rc = ssd_riser_fit_solve(moments + i, risers + i, &cal, min_points, out + i);
    if(rc) return rc;
  }
  return SSD_OK;
}

int ssd_process_host_riser_fits(ssd_handle *h, const void *frames, int nframes, int input, ssd_frame_result *results,
                                ssd_frame_risers *risers, ssd_frame_moments *moments, int min_points, ssd_frame_riser_fits *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_riser_fits", h && frames && results && risers && out, nframes, input, kHandleCal);
  return rc ? rc : process_host_riser_fits_impl(h, "ssd_process_host_riser_fits", frames, nframes, nullptr, input, results, risers, moments, min_points, out);
}

int ssd_process_host_cameras_riser_fits(ssd_handle *h, const void *frames, int nframes, const uint16_t *camera_of_frame, int input,
                                        ssd_frame_result *results, ssd_frame_risers *risers, ssd_frame_moments *moments, int min_points,
                                        ssd_frame_riser_fits *out)
{
  const int rc = check_host_batch(h, "ssd_process_host_cameras_riser_fits", h && frames && results && risers && out, nframes, input, kCameraTable, camera_of_frame);
  return rc ? rc : process_host_riser_fits_impl(h, "ssd_process_host_cameras_riser_fits", frames, nframes, camera_of_frame, input, results, risers, moments, min_points, out);
}

/* the records and the priors of the ground fit, on its first call.  The pinned sides of THIS pass are not counted as workspace (the other
 * three passes' are: DESIGN.md section 7u) */
static_assert(sizeof(ssd_ground_moments) == sizeof(long long) * kGroundSums, "ssd_ground_moments is k_ground_moments' record");
static int ground_prepare(ssd_handle *h)
{
  const int rc = records_prepare(h, h->ground, false, "ssd_enqueue_ground_fit");
  return rc ? rc : table_prepare(h, h->groundPriors, static_cast<size_t>(h->F), false, "ssd_enqueue_ground_fit");
}

/* the refusals of a ground-fit call, before anything is launched or copied */
static int check_ground_fit(const ssd_handle *h, const char *who, int input, const ssd_camera *priors, int npriors, int nframes, double tol)
{
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, std::string(who) + ": input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  if(!(tol > 0.0) || !(tol <= 1.0))
    return fail(SSD_E_ARG, std::string(who) + ": tol must lie in (0, 1]");
  if(npriors != 0 && npriors != 1 && npriors != nframes)
    return fail(SSD_E_ARG, std::string(who) + ": npriors must be 0, 1 or nframes");
  if(npriors > 0 && !priors)
    return fail(SSD_E_ARG, std::string(who) + ": null priors");
  if(input == SSD_INPUT_DEPTH16)
  {
    if(npriors == 0 && !h->haveIntr)
      return fail(SSD_E_ARG, std::string(who) + ": depth input with the handle's calibration: call ssd_set_intrinsics first");
    for(int i = 0; i < npriors; i++)
      if(!priors[i].has_intrinsics || !good_intrinsics(priors[i].intr))
        return fail(SSD_E_ARG, std::string(who) + ": depth input, and prior " + std::to_string(i) + " has no (valid) intrinsics");
  }
  return SSD_OK;
}

/* arguments checked by the callers */
static int enqueue_ground_fit_impl(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, hipStream_t s, int input,
                                   const ssd_camera *priors, int npriors, double tol)
{
  const bool depth = input == SSD_INPUT_DEPTH16;
  int rc = check_device_frames(h, "ssd_enqueue_ground_fit", d_frames, frame_stride_bytes, nframes, input);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  rc = ground_prepare(h);
  if(!rc) rc = table_wait(h->groundPriors);
  if(!rc) rc = pass_open(h->ground.pass, s, false, "ssd_enqueue_ground_fit");   /* another stream: behind the previous call */
  if(rc) return rc;
  const int np = npriors > 0 ? npriors : 1;
  h->groundPriorCal.resize(static_cast<size_t>(np));
  if(npriors == 0)
  {
    ssd_calibration &c = h->groundPriorCal[0];
    c = handle_calibration(h);
    ground_prior_fill(h->groundPriors.h[0], c, depth ? &h->intr : nullptr);
  }
  else
    for(int i = 0; i < np; i++)
    {
      h->groundPriorCal[i] = priors[i].cal;
      ground_prior_fill(h->groundPriors.h[i], priors[i].cal, depth ? &priors[i].intr : nullptr);
    }
  rc = table_send(h->groundPriors, static_cast<size_t>(np), s);
  if(!rc) rc = records_zero(h->ground, nframes, s);
  if(rc) return rc;
  const GroundRange R{ h->cfg.x_min, h->cfg.x_max, h->cfg.y_min, h->cfg.y_max, tol };
  launch_ground_moments(d_frames, frame_stride_bytes, h->P.W, h->P.H, nframes, depth, h->groundPriors.d, np > 1 ? 1 : 0, R,
                        reinterpret_cast<long long *>(h->ground.d.get()), s);
  return records_finish(h->ground, nframes, s, false);
}

int ssd_enqueue_ground_fit(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                           const ssd_camera *priors, int npriors, double tol)
{
  if(!h || !d_frames)
    return fail(SSD_E_ARG, "ssd_enqueue_ground_fit: null argument");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, "ssd_enqueue_ground_fit: nframes must be 1..max_frames_per_batch");
  const int rc = check_ground_fit(h, "ssd_enqueue_ground_fit", input, priors, npriors, nframes, tol);
  if(rc) return rc;
  return enqueue_ground_fit_impl(h, d_frames, frame_stride_bytes, nframes, static_cast<hipStream_t>(stream), input, priors, npriors, tol);
}

int ssd_fetch_ground_fit(ssd_handle *h, ssd_ground_fit *out, int nframes, int min_points, void *)
{
  const int wait = records_wait(h, &ssd_handle::ground, out, nframes, "ssd_fetch_ground_fit", "ssd_enqueue_ground_fit", "frame");
  if(wait) return wait;
  const bool each = h->groundPriorCal.size() > 1;
  for(int i = 0; i < nframes; i++)
  {
    const int rc = ssd_ground_fit_solve(&h->ground.h[i], &h->groundPriorCal[each ? i : 0], min_points, out + i);
    if(rc) return rc;
  }
  return SSD_OK;
}

int ssd_process_host_ground_fit(ssd_handle *h, const void *frames, int nframes, int input, const ssd_camera *priors, int npriors,
                                double tol, int min_points, ssd_ground_fit *out)
{
  int rc = check_host_batch(h, "ssd_process_host_ground_fit", h && frames && out, nframes, input, kOwnPriors);
  if(!rc) rc = check_ground_fit(h, "ssd_process_host_ground_fit", input, priors, npriors, nframes, tol);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForGroundFit), frames, nframes };
  rc = feed.prepare();
  if(rc) return rc;
  const bool each = npriors == nframes && npriors > 1;             /* a prior per frame: a slice takes its part of them */
  return process_host_frames(h, feed,
    [&](const void *buf, int at, int n)
    {
      return enqueue_ground_fit_impl(h, buf, feed.f.devFrameBytes, n, h->ingestCompute, input, each ? priors + at : priors, each ? n : npriors, tol);
    },
    [&](int at, int n) { return ssd_fetch_ground_fit(h, out + at, n, min_points, nullptr); });      /* a slice's records, solved into `out` */
}

/* ---- stair pose: a camera located against a stair map (include/ssd_hip.h) ------------------------------------ */

/* the records, the targets and the index of the pass, on its first call */
static int stair_pose_prepare(ssd_handle *h)
{
  const char *me = "ssd_enqueue_stair_pose";
  int rc = records_prepare(h, h->pose, true, me);
  if(!rc) rc = table_prepare(h, h->poseTargetsUp, static_cast<size_t>(SSD_MAX_STAIR_MAPS), true, me);
  return rc ? rc : table_prepare(h, h->poseIndexUp, static_cast<size_t>(h->F), true, me);
}

/* arguments checked by the callers */
static int enqueue_stair_pose_impl(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, hipStream_t s, int input,
                                   const ssd_stair_pose_target *targets, int ntargets, const uint16_t *target_of_frame, const ssd_stair_pose_rule &rule)
{
  const bool depth = input == SSD_INPUT_DEPTH16;
  int rc = check_device_frames(h, "ssd_enqueue_stair_pose", d_frames, frame_stride_bytes, nframes, input);
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  rc = stair_pose_prepare(h);
  if(!rc) rc = table_wait(h->poseIndexUp);                      /* its event lies behind the targets' copy too */
  if(rc) return rc;
  const bool timing = h->timing;
  rc = pass_open(h->pose.pass, s, timing, "ssd_enqueue_stair_pose");   /* another stream: behind the previous call */
  if(rc) return rc;
  h->poseTargets.assign(targets, targets + ntargets);
  h->poseIndex.resize(static_cast<size_t>(nframes));
  for(int t = 0; t < ntargets; t++)
    pose_target_fill(h->poseTargetsUp.h[t], targets[t], depth, rule);
  for(int i = 0; i < nframes; i++)
    h->poseIndexUp.h[i] = h->poseIndex[i] = target_of_frame ? static_cast<int>(target_of_frame[i]) : 0;
  rc = table_copy(h->poseTargetsUp, static_cast<size_t>(ntargets), s);
  if(!rc) rc = table_send(h->poseIndexUp, static_cast<size_t>(nframes), s);
  if(!rc) rc = pass_start(h->pose.pass, s, timing);         /* the timed span excludes the uploads */
  if(!rc) rc = records_zero(h->pose, nframes, s);
  if(rc) return rc;
  const PoseRange R{ h->cfg.x_min, h->cfg.x_max, h->cfg.y_min, h->cfg.y_max };
  launch_stair_pose(d_frames, frame_stride_bytes, h->P.W, h->P.H, nframes, depth, h->poseTargetsUp.d, ntargets, h->poseIndexUp.d, R, h->pose.d, s);
  return records_finish(h->pose, nframes, s, timing);
}

int ssd_enqueue_stair_pose(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int input,
                           const ssd_stair_pose_target *targets, int ntargets, const uint16_t *target_of_frame, const ssd_stair_pose_rule *rule)
{
  const std::string me("ssd_enqueue_stair_pose");
  if(!h || !d_frames)
    return fail(SSD_E_ARG, me + ": null argument");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, me + ": nframes must be 1..max_frames_per_batch");
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, me + ": input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  int rc = check_pose_rule(me, rule);
  if(!rc) rc = check_pose_targets(me, targets, ntargets, target_of_frame, nframes, input);
  if(rc) return rc;
  return enqueue_stair_pose_impl(h, d_frames, frame_stride_bytes, nframes, static_cast<hipStream_t>(stream), input, targets, ntargets, target_of_frame, *rule);
}

int ssd_fetch_stair_pose_moments(ssd_handle *h, ssd_stair_pose_moments *out, int nframes, void *)
{
  return records_fetch(h, &ssd_handle::pose, out, nframes, "ssd_fetch_stair_pose_moments", "ssd_enqueue_stair_pose", "frame");
}

int ssd_fetch_stair_pose(ssd_handle *h, ssd_stair_pose *out, int min_points, double observable, void *)
{
  if(!h || !out)
    return fail(SSD_E_ARG, "ssd_fetch_stair_pose: null argument");
  const int wait = pass_wait(h, &h->pose.pass, "ssd_fetch_stair_pose", "no ssd_enqueue_stair_pose to wait for");
  if(wait) return wait;
  std::vector<ssd_stair_pose_moments> folds(h->poseTargets.size());
  std::memset(folds.data(), 0, sizeof(ssd_stair_pose_moments) * folds.size());
  int rc = pose_fold_frames("ssd_fetch_stair_pose", h->pose.h, h->poseIndex.data(), h->pose.count, folds);
  for(size_t t = 0; t < folds.size() && !rc; t++)
    rc = ssd_stair_pose_solve(&folds[t], &h->poseTargets[t], min_points, observable, out + t);
  return rc;
}

int ssd_get_stair_pose_time(ssd_handle *h, float *ms)
{
  return pass_time(h, h ? &h->pose.pass : nullptr, "ssd_get_stair_pose_time", "ssd_enqueue_stair_pose", ms);
}

int ssd_process_host_stair_pose(ssd_handle *h, const void *frames, int nframes, int input, const ssd_stair_pose_target *targets, int ntargets,
                                const uint16_t *target_of_frame, const ssd_stair_pose_rule *rule, int min_points, double observable,
                                ssd_stair_pose_moments *moments, ssd_stair_pose *out)
{
  const std::string me("ssd_process_host_stair_pose");
  int rc = check_host_batch(h, "ssd_process_host_stair_pose", h && frames && out, nframes, input, kOwnPriors);
  if(!rc) rc = check_pose_rule(me, rule);
  if(!rc) rc = check_pose_targets(me, targets, ntargets, target_of_frame, nframes, input);
  if(!rc && (!(observable >= 0.0) || !(observable <= 1.0)))
    rc = fail(SSD_E_ARG, me + ": observable must lie in [0, 1]");
  if(rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, input, kForGroundFit), frames, nframes };
  rc = feed.prepare();
  if(rc) return rc;
  std::vector<ssd_stair_pose_moments> folds(static_cast<size_t>(ntargets)), own;
  std::memset(folds.data(), 0, sizeof(ssd_stair_pose_moments) * folds.size());
  if(!moments)
    own.resize(static_cast<size_t>(feed.slice));
  rc = process_host_frames(h, feed,
    [&](const void *buf, int at, int n)
    {
      return enqueue_stair_pose_impl(h, buf, feed.f.devFrameBytes, n, h->ingestCompute, input, targets, ntargets, target_of_frame ? target_of_frame + at : nullptr, *rule);
    },
    /* a slice's records, behind its kernel: to the caller's array or the call's own, and onto the folds - frame order, slice by slice */
    [&](int at, int n)
    {
      ssd_stair_pose_moments *dst = moments ? moments + at : own.data();
      const int got = ssd_fetch_stair_pose_moments(h, dst, n, nullptr);
      return got ? got : pose_fold_frames("ssd_process_host_stair_pose", dst, h->poseIndex.data(), n, folds);
    });
  for(int t = 0; t < ntargets && !rc; t++)
    rc = ssd_stair_pose_solve(&folds[static_cast<size_t>(t)], targets + t, min_points, observable, out + t);
  return rc;
}

/* ---- depth fusion: one trimmed-median frame from n frames of a still camera (include/ssd_hip.h) ---------------- */

static bool ranges_overlap(const void *a, size_t aBytes, const void *b, size_t bBytes)
{
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + bBytes && b0 < a0 + aBytes;
}

/* What a depth pre-pass reads and writes: nframes 16-bit frames in, `count` 16-bit frames out and, optionally, a byte map per output frame
 * (noun / mapName: what the pass calls it, for the refusals).  Neither may overlap the input: a kernel that reads several frames, or its
 * neighbours' pixels, races with any write into what it reads */
static int check_depth_planes(const ssd_handle *h, const std::string &me, const void *d_frames, size_t frame_stride_bytes, int nframes, const void *d_out,
                              size_t out_stride_bytes, const uint8_t *d_map, size_t map_stride_bytes, int count, const char *noun, const char *mapName)
{
  int rc = check_device_frames(h, me.c_str(), d_frames, frame_stride_bytes, nframes, SSD_INPUT_DEPTH16);
  if(!rc) rc = check_device_frames(h, me.c_str(), d_out, out_stride_bytes, count, SSD_INPUT_DEPTH16);
  if(rc) return rc;
  const size_t nPoints = static_cast<size_t>(h->P.nPoints), frameBytes = nPoints * 2;
  if(d_map && count > 1 && map_stride_bytes < nPoints)
    return fail(SSD_E_ARG, me + ": the " + noun + " stride must hold a frame's bytes");
  const size_t inBytes = static_cast<size_t>(nframes - 1) * frame_stride_bytes + frameBytes;
  if(ranges_overlap(d_frames, inBytes, d_out, static_cast<size_t>(count - 1) * out_stride_bytes + frameBytes) ||
     (d_map && ranges_overlap(d_frames, inBytes, d_map, static_cast<size_t>(count - 1) * map_stride_bytes + nPoints)))
    return fail(SSD_E_ARG, me + ": the output and the " + mapName + " must not overlap the frames");
  return SSD_OK;
}

/* the refusals of a fusion call, before anything is launched or copied; *use: the rule to go by, *ngroups: its groups */
static int check_depth_fuse(const ssd_handle *h, const std::string &me, const void *d_frames, size_t frame_stride_bytes, int nframes, int n, int hop,
                            const ssd_depth_fuse_rule *rule, const void *d_out, size_t out_stride_bytes, const uint8_t *d_support,
                            size_t support_stride_bytes, ssd_depth_fuse_rule *use, int *ngroups)
{
  if(!h || !d_frames || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  const int rc = check_fuse_rule(me, n, rule, use);
  if(rc) return rc;
  if(hop < 1 || hop > n)
    return fail(SSD_E_ARG, me + ": hop must lie in 1 .. n");
  if(nframes < n || nframes > h->F)
    return fail(SSD_E_ARG, me + ": nframes must lie in n .. max_frames_per_batch");
  *ngroups = (nframes - n) / hop + 1;
  if(*ngroups > h->F)
    return fail(SSD_E_ARG, me + ": more groups than max_frames_per_batch");
  return check_depth_planes(h, me, d_frames, frame_stride_bytes, nframes, d_out, out_stride_bytes, d_support, support_stride_bytes, *ngroups, "support", "support");
}

/* arguments checked by the callers */
static int enqueue_depth_fuse_impl(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, hipStream_t s, int n, int hop, int ngroups,
                                   const ssd_depth_fuse_rule &rule, void *d_out, size_t out_stride_bytes, uint8_t *d_support, size_t support_stride_bytes)
{
  HIP_TRY(hipSetDevice(h->device));
  int rc = records_prepare(h, h->fuse, true, "ssd_enqueue_depth_fuse");
  if(rc) return rc;
  const bool timing = h->timing;
  rc = pass_open(h->fuse.pass, s, timing, "ssd_enqueue_depth_fuse");   /* another stream: behind the previous call */
  if(!rc) rc = pass_start(h->fuse.pass, s, timing);
  if(!rc) rc = records_zero(h->fuse, ngroups, s);
  if(rc) return rc;
  launch_depth_fuse(d_frames, frame_stride_bytes, h->P.nPoints, n, hop, ngroups, rule, d_out, out_stride_bytes, d_support, support_stride_bytes,
                    h->fuse.d, h->tune.fuseGroupFastest != 0, s);
  return records_finish(h->fuse, ngroups, s, timing);
}

int ssd_enqueue_depth_fuse(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, int n, int hop,
                           const ssd_depth_fuse_rule *rule, void *d_out, size_t out_stride_bytes, uint8_t *d_support, size_t support_stride_bytes)
{
  ssd_depth_fuse_rule R;
  int ngroups = 0;
  const int rc = check_depth_fuse(h, "ssd_enqueue_depth_fuse", d_frames, frame_stride_bytes, nframes, n, hop, rule, d_out, out_stride_bytes, d_support,
                                  support_stride_bytes, &R, &ngroups);
  if(rc) return rc;
  return enqueue_depth_fuse_impl(h, d_frames, frame_stride_bytes, static_cast<hipStream_t>(stream), n, hop, ngroups, R, d_out, out_stride_bytes,
                                 d_support, support_stride_bytes);
}

int ssd_fetch_depth_fuse(ssd_handle *h, ssd_depth_fuse_stats *out, int ngroups, void *)
{
  return records_fetch(h, &ssd_handle::fuse, out, ngroups, "ssd_fetch_depth_fuse", "ssd_enqueue_depth_fuse", "group");
}

int ssd_get_depth_fuse_time(ssd_handle *h, float *ms)
{
  return pass_time(h, h ? &h->fuse.pass : nullptr, "ssd_get_depth_fuse_time", "ssd_enqueue_depth_fuse", ms);
}

extern "C++"
{
/* The host-fed form of a depth pre-pass: every n frames of the host's become one on the device (n = 1: each frame becomes another), and
 * that one is detected.  pre(buf, stride, at, cnt, stage, stageStride) enqueues the pre-pass of a slice's cnt frames, the batch's
 * frames at .. at + cnt - 1, into the staging buffer on ingestCompute, stats(g0, groups) fetches its records where the caller wants them; `frames`, if any, takes the staged frames; kind:
 * what they are, for the allocation's message.  The stream arrangement is that of the other stand-alone frame passes
 * (process_host_frames): slice c's copy goes out, slice c - 1 is collected - its results, which lie behind its detection and so behind its
 * pre-pass, then its records and its staged frames -, and only then slice c is pre-passed and detected.  So ONE staging buffer and the
 * pass's one set of records do: what overlaps is a slice's copy with the slice before it, not two slices' kernels.  And one buffer does for
 * every pre-pass of the handle: a call that succeeds has collected its last slice when it returns (process_host_frames ends with that
 * slice's collect, whose ssd_fetch_back waits behind the detection that read the buffer), and the grow path below waits for every
 * workspace's last enqueue before it gives the buffer back. */
template<class Pre, class Stats>
static int process_depth_host_pre(ssd_handle *h, const std::string &me, const char *kind, const uint16_t *depth, int nframes, int n,
                                  ssd_frame_result *results, uint16_t *frames, Pre pre, Stats stats)
{
  if(h->P.W % 4 != 0)
    return fail(SSD_E_ARG, me + ": width must be a multiple of 4 (ssd_enqueue_depth)");
  HIP_TRY(hipSetDevice(h->device));
  SliceFeed feed{ h, host_frames(h, SSD_INPUT_DEPTH16, kForGroundFit), depth, nframes };
  const int rc = feed.prepare();
  if(rc) return rc;
  feed.slice = feed.slice / n * n;                                 /* a whole number of groups (n <= 16 <= a slice's frames, or n <= F) */
  if(feed.slice < n)
    return fail(SSD_E_ARG, me + ": n exceeds a slice's frames");
  const size_t frameBytes = static_cast<size_t>(h->P.nPoints) * 2, stride = feed.f.devFrameBytes;
  const size_t stageBytes = static_cast<size_t>(feed.slice / n) * stride;
  if(h->depthStageCap < stageBytes)
  {
    for(int k = 0; k < h->depth; k++)                                /* its readers are this handle's detections */
      if(h->lane[k].haveLast)
        HIP_TRY(hipEventSynchronize(h->lane[k].done));
    h->depthStage.reset();
    h->depthStageCap = 0;
    const hipError_t e = h->depthStage.alloc(stageBytes);
    if(e != hipSuccess)
      return hip_fail(e, me + ": the " + kind + " frames' buffer: ");
    h->depthStageCap = stageBytes;
  }
  return process_host_frames(h, feed,
    [&](const void *buf, int at, int cnt)
    {
      int r = pre(buf, feed.f.devFrameBytes, at, cnt, h->depthStage.get(), stride);
      if(!r) r = enqueue_impl(h, h->depthStage, stride, cnt / n, h->ingestCompute, SSD_STAGE_ALL, true);
      return r;
    },
    [&](int at, int cnt)
    {
      const int g0 = at / n, groups = cnt / n;
      int r = ssd_fetch_back(h, results + g0, groups, 0);
      if(!r) r = stats(g0, groups);
      if(!r && frames)
      {
        HIP_TRY(hipMemcpy2DAsync(reinterpret_cast<unsigned char *>(frames) + static_cast<size_t>(g0) * frameBytes, frameBytes, h->depthStage, stride,
                                 frameBytes, static_cast<size_t>(groups), hipMemcpyDeviceToHost, h->ingestCompute));
        HIP_TRY(hipStreamSynchronize(h->ingestCompute));
      }
      return r;
    });
}
} // extern "C++"

/* Host-fed, disjoint groups of n */
int ssd_process_depth_host_fused(ssd_handle *h, const uint16_t *depth, int nframes, int n, const ssd_depth_fuse_rule *rule,
                                 ssd_frame_result *results, uint16_t *fused, ssd_depth_fuse_stats *stats)
{
  const std::string me("ssd_process_depth_host_fused");
  int rc = check_host_batch(h, me.c_str(), h && depth && results, nframes, SSD_INPUT_DEPTH16, kHandleCal);
  ssd_depth_fuse_rule R;
  if(!rc) rc = check_fuse_rule(me, n, rule, &R);
  if(rc) return rc;
  if(n > h->F || nframes % n != 0)
    return fail(SSD_E_ARG, me + ": n must not exceed max_frames_per_batch and nframes must be a multiple of n");
  return process_depth_host_pre(h, me, "fused", depth, nframes, n, results, fused,
    [&](const void *buf, size_t stride, int, int cnt, unsigned char *stage, size_t stageStride)
    {
      return enqueue_depth_fuse_impl(h, buf, stride, h->ingestCompute, n, n, cnt / n, R, stage, stageStride, nullptr, 0);
    },
    [&](int g0, int groups) { return stats ? ssd_fetch_depth_fuse(h, stats + g0, groups, nullptr) : static_cast<int>(SSD_OK); });
}

/* ---- depth edge filter: mixed and lone pixels out of one frame (include/ssd_hip.h) -------------------------------- */

/* the refusals of a filter call, before anything is launched or copied; *use: the rule to go by */
static int check_depth_edges(const ssd_handle *h, const std::string &me, const void *d_frames, size_t frame_stride_bytes, int nframes,
                             const ssd_depth_edge_rule *rule, const void *d_out, size_t out_stride_bytes, const uint8_t *d_cls, size_t cls_stride_bytes,
                             ssd_depth_edge_rule *use)
{
  if(!h || !d_frames || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  const int rc = check_edge_rule(me, rule, use);
  if(rc) return rc;
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, me + ": nframes must lie in 1 .. max_frames_per_batch");
  return check_depth_planes(h, me, d_frames, frame_stride_bytes, nframes, d_out, out_stride_bytes, d_cls, cls_stride_bytes, nframes, "class", "class map");
}

/* arguments checked by the callers */
static int enqueue_depth_edges_impl(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, hipStream_t s,
                                    const ssd_depth_edge_rule &rule, void *d_out, size_t out_stride_bytes, uint8_t *d_cls, size_t cls_stride_bytes)
{
  HIP_TRY(hipSetDevice(h->device));
  int rc = records_prepare(h, h->edge, true, "ssd_enqueue_depth_edges");
  if(rc) return rc;
  const bool timing = h->timing;
  rc = pass_open(h->edge.pass, s, timing, "ssd_enqueue_depth_edges");   /* another stream: behind the previous call */
  if(!rc) rc = pass_start(h->edge.pass, s, timing);
  if(!rc) rc = records_zero(h->edge, nframes, s);
  if(rc) return rc;
  launch_depth_edges(d_frames, frame_stride_bytes, h->P.W, h->P.H, nframes, rule, d_out, out_stride_bytes, d_cls, cls_stride_bytes, h->edge.d, s);
  return records_finish(h->edge, nframes, s, timing);
}

int ssd_enqueue_depth_edges(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, const ssd_depth_edge_rule *rule,
                            void *d_out, size_t out_stride_bytes, uint8_t *d_cls, size_t cls_stride_bytes)
{
  ssd_depth_edge_rule R;
  const int rc = check_depth_edges(h, "ssd_enqueue_depth_edges", d_frames, frame_stride_bytes, nframes, rule, d_out, out_stride_bytes, d_cls,
                                   cls_stride_bytes, &R);
  if(rc) return rc;
  return enqueue_depth_edges_impl(h, d_frames, frame_stride_bytes, nframes, static_cast<hipStream_t>(stream), R, d_out, out_stride_bytes, d_cls,
                                  cls_stride_bytes);
}

int ssd_fetch_depth_edges(ssd_handle *h, ssd_depth_edge_stats *out, int nframes, void *)
{
  return records_fetch(h, &ssd_handle::edge, out, nframes, "ssd_fetch_depth_edges", "ssd_enqueue_depth_edges", "frame");
}

int ssd_get_depth_edges_time(ssd_handle *h, float *ms)
{
  return pass_time(h, h ? &h->edge.pass : nullptr, "ssd_get_depth_edges_time", "ssd_enqueue_depth_edges", ms);
}

/* Host-fed: process_depth_host_pre with groups of one.  Slices are whole frames and the filter never looks across frames, so nothing is
 * cut down */
int ssd_process_depth_host_edges(ssd_handle *h, const uint16_t *depth, int nframes, const ssd_depth_edge_rule *rule, ssd_frame_result *results,
                                 uint16_t *filtered, ssd_depth_edge_stats *stats)
{
  const std::string me("ssd_process_depth_host_edges");
  int rc = check_host_batch(h, me.c_str(), h && depth && results, nframes, SSD_INPUT_DEPTH16, kHandleCal);
  ssd_depth_edge_rule R;
  if(!rc) rc = check_edge_rule(me, rule, &R);
  if(rc) return rc;
  return process_depth_host_pre(h, me, "filtered", depth, nframes, 1, results, filtered,
    [&](const void *buf, size_t stride, int, int cnt, unsigned char *stage, size_t stageStride)
    {
      return enqueue_depth_edges_impl(h, buf, stride, cnt, h->ingestCompute, R, stage, stageStride, nullptr, 0);
    },
    [&](int at, int cnt) { return stats ? ssd_fetch_depth_edges(h, stats + at, cnt, nullptr) : static_cast<int>(SSD_OK); });
}

/* ---- depth warp: the frame another pose would have seen (include/ssd_hip.h) ----------------------------------- */

/* Word safety: k_depth_warp swaps the aligned 32-bit word that holds a pixel, so every such word must be the frame's own - an even
 * number of pixels, the output and its stride multiples of 4.  Every caller of enqueue_depth_warp_impl goes through this */
static int check_warp_words(const ssd_handle *h, const std::string &me, const void *d_out, size_t out_stride_bytes)
{
  if(h->P.nPoints % 2 != 0)
    return fail(SSD_E_ARG, me + ": width * height must be even (the output is written in 32-bit words)");
  if(reinterpret_cast<size_t>(d_out) % 4 != 0 || out_stride_bytes % 4 != 0)
    return fail(SSD_E_ARG, me + ": the output and its stride must be multiples of 4 bytes (the output is written in 32-bit words)");
  return SSD_OK;
}

/* the refusals of a warp call, before anything is launched or copied */
static int check_depth_warp(const ssd_handle *h, const std::string &me, const void *d_frames, size_t frame_stride_bytes, int nframes,
                            const ssd_depth_warp_view *views, const ssd_intrinsics *dst, const void *d_out, size_t out_stride_bytes)
{
  if(!h || !d_frames || !views || !dst || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, me + ": nframes must lie in 1 .. max_frames_per_batch");
  int rc = check_warp_views(me, views, nframes, dst);
  if(!rc) rc = check_device_frames(h, me.c_str(), d_frames, frame_stride_bytes, nframes, SSD_INPUT_DEPTH16);
  if(!rc) rc = check_device_frames(h, me.c_str(), d_out, out_stride_bytes, nframes, SSD_INPUT_DEPTH16);
  if(rc) return rc;
  rc = check_warp_words(h, me, d_out, out_stride_bytes);
  if(rc) return rc;
  const size_t frameBytes = static_cast<size_t>(h->P.nPoints) * 2;
  if(ranges_overlap(d_frames, static_cast<size_t>(nframes - 1) * frame_stride_bytes + frameBytes, d_out,
                    static_cast<size_t>(nframes - 1) * out_stride_bytes + frameBytes))
    return fail(SSD_E_ARG, me + ": the output must not overlap the frames");
  return SSD_OK;
}

/* arguments checked by the callers */
static int enqueue_depth_warp_impl(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, hipStream_t s,
                                   const ssd_depth_warp_view *views, const ssd_intrinsics &dst, void *d_out, size_t out_stride_bytes)
{
  const char *me = "ssd_enqueue_depth_warp";
  HIP_TRY(hipSetDevice(h->device));
  int rc = records_prepare(h, h->warp, true, me);
  if(!rc) rc = table_prepare(h, h->warpViews, static_cast<size_t>(h->F), true, me);
  if(!rc) rc = table_wait(h->warpViews);
  if(rc) return rc;
  const bool timing = h->timing;
  rc = pass_open(h->warp.pass, s, timing, me);                  /* another stream: behind the previous call */
  if(rc) return rc;
  std::memcpy(h->warpViews.h, views, sizeof(ssd_depth_warp_view) * static_cast<size_t>(nframes));
  rc = table_send(h->warpViews, static_cast<size_t>(nframes), s);
  if(!rc) rc = pass_start(h->warp.pass, s, timing);             /* the timed span excludes the upload */
  if(!rc) rc = records_zero(h->warp, nframes, s);
  if(rc) return rc;
  /* the frames' own bytes to 0, "nothing landed": the bytes between and behind the frames are not the pass's */
  const size_t frameBytes = static_cast<size_t>(h->P.nPoints) * 2;
  HIP_TRY(hipMemset2DAsync(d_out, nframes > 1 ? out_stride_bytes : frameBytes, 0, frameBytes, static_cast<size_t>(nframes), s));
  launch_depth_warp(d_frames, frame_stride_bytes, h->P.W, h->P.H, nframes, h->warpViews.d, dst, d_out, out_stride_bytes, h->warp.d, s);
  return records_finish(h->warp, nframes, s, timing);
}

int ssd_enqueue_depth_warp(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream,
                           const ssd_depth_warp_view *views, const ssd_intrinsics *dst, void *d_out, size_t out_stride_bytes)
{
  const int rc = check_depth_warp(h, "ssd_enqueue_depth_warp", d_frames, frame_stride_bytes, nframes, views, dst, d_out, out_stride_bytes);
  if(rc) return rc;
  return enqueue_depth_warp_impl(h, d_frames, frame_stride_bytes, nframes, static_cast<hipStream_t>(stream), views, *dst, d_out, out_stride_bytes);
}

int ssd_fetch_depth_warp(ssd_handle *h, ssd_depth_warp_stats *out, int nframes, void *)
{
  return records_fetch(h, &ssd_handle::warp, out, nframes, "ssd_fetch_depth_warp", "ssd_enqueue_depth_warp", "frame");
}

int ssd_get_depth_warp_time(ssd_handle *h, float *ms)
{
  return pass_time(h, h ? &h->warp.pass : nullptr, "ssd_get_depth_warp_time", "ssd_enqueue_depth_warp", ms);
}

/* Host-fed, disjoint groups of n: process_depth_host_pre, whose pre-pass is two - the slice warped into warpStage, that fused into the
 * staging buffer the detection reads.  Both run on ingestCompute, so the fusion lies behind the warp and the next slice's warp behind
 * this slice's fusion; warpStage grows only behind what that stream holds */
int ssd_process_depth_host_warp_fused(ssd_handle *h, const uint16_t *depth, int nframes, int n, const ssd_depth_warp_view *views,
                                      const ssd_intrinsics *dst, const ssd_depth_fuse_rule *fuse_rule, ssd_frame_result *results,
                                      uint16_t *fused, ssd_depth_warp_stats *warp_stats, ssd_depth_fuse_stats *fuse_stats)
{
  const std::string me("ssd_process_depth_host_warp_fused");
  int rc = check_host_batch(h, me.c_str(), h && depth && results, nframes, SSD_INPUT_DEPTH16, kHandleCal);
  ssd_depth_fuse_rule R;
  if(!rc) rc = check_fuse_rule(me, n, fuse_rule, &R);
  if(!rc) rc = check_warp_views(me, views, nframes, dst);
  if(rc) return rc;
  if(n > h->F || nframes % n != 0)
    return fail(SSD_E_ARG, me + ": n must not exceed max_frames_per_batch and nframes must be a multiple of n");
  if(h->P.nPoints % 2 != 0)
    return fail(SSD_E_ARG, me + ": width * height must be even (the output is written in 32-bit words)");
  if(std::memcmp(dst, &h->intr, sizeof(*dst)) != 0)
    return fail(SSD_E_ARG, me + ": dst must be the intrinsics the handle detects under (ssd_set_intrinsics)");
  return process_depth_host_pre(h, me, "fused", depth, nframes, n, results, fused,
    [&](const void *buf, size_t stride, int at, int cnt, unsigned char *stage, size_t stageStride)
    {
      const size_t need = static_cast<size_t>(cnt) * stride;
      if(h->warpStageCap < need)
      {
        HIP_TRY(hipStreamSynchronize(h->ingestCompute));            /* its readers are this handle's fusions on that stream */
        h->warpStage.reset();
        h->warpStageCap = 0;
        const hipError_t e = h->warpStage.alloc(need);
        if(e != hipSuccess)
          return hip_fail(e, me + ": the warped frames' buffer: ");
        h->warpStageCap = need;
      }
      /* the stage's words are its own: the allocation is aligned and the slices' stride a multiple of 16 - checked all the same */
      int r = check_warp_words(h, me, h->warpStage.get(), stride);
      if(!r) r = enqueue_depth_warp_impl(h, buf, stride, cnt, h->ingestCompute, views + at, *dst, h->warpStage.get(), stride);
      if(!r) r = enqueue_depth_fuse_impl(h, h->warpStage.get(), stride, h->ingestCompute, n, n, cnt / n, R, stage, stageStride, nullptr, 0);
      return r;
    },
    [&](int g0, int groups)
    {
      int r = warp_stats ? ssd_fetch_depth_warp(h, warp_stats + static_cast<size_t>(g0) * n, groups * n, nullptr) : static_cast<int>(SSD_OK);
      if(!r && fuse_stats) r = ssd_fetch_depth_fuse(h, fuse_stats + g0, groups, nullptr);
      return r;
    });
}

/* ---- depth fill: holes and one-pixel see-through closed between agreeing samples (include/ssd_hip.h) ----------------- */

/* the refusals of a fill call, before anything is launched or copied; *use: the rule to go by */
static int check_depth_fill(const ssd_handle *h, const std::string &me, const void *d_frames, size_t frame_stride_bytes, int nframes,
                            const ssd_depth_fill_rule *rule, const void *d_out, size_t out_stride_bytes, const uint8_t *d_cls, size_t cls_stride_bytes,
                            ssd_depth_fill_rule *use)
{
  if(!h || !d_frames || !d_out)
    return fail(SSD_E_ARG, me + ": null argument");
  const int rc = check_fill_rule(me, rule, use);
  if(rc) return rc;
  if(nframes < 1 || nframes > h->F)
    return fail(SSD_E_ARG, me + ": nframes must lie in 1 .. max_frames_per_batch");
  return check_depth_planes(h, me, d_frames, frame_stride_bytes, nframes, d_out, out_stride_bytes, d_cls, cls_stride_bytes, nframes, "class", "class map");
}

/* arguments checked by the callers */
static int enqueue_depth_fill_impl(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, hipStream_t s,
                                   const ssd_depth_fill_rule &rule, void *d_out, size_t out_stride_bytes, uint8_t *d_cls, size_t cls_stride_bytes)
{
  HIP_TRY(hipSetDevice(h->device));
  int rc = records_prepare(h, h->fill, true, "ssd_enqueue_depth_fill");
  if(rc) return rc;
  const bool timing = h->timing;
  rc = pass_open(h->fill.pass, s, timing, "ssd_enqueue_depth_fill");    /* another stream: behind the previous call */
  if(!rc) rc = pass_start(h->fill.pass, s, timing);
  if(!rc) rc = records_zero(h->fill, nframes, s);
  if(rc) return rc;
  launch_depth_fill(d_frames, frame_stride_bytes, h->P.W, h->P.H, nframes, rule, d_out, out_stride_bytes, d_cls, cls_stride_bytes, h->fill.d, s);
  return records_finish(h->fill, nframes, s, timing);
}

int ssd_enqueue_depth_fill(ssd_handle *h, const void *d_frames, size_t frame_stride_bytes, int nframes, void *stream, const ssd_depth_fill_rule *rule,
                           void *d_out, size_t out_stride_bytes, uint8_t *d_cls, size_t cls_stride_bytes)
{
  ssd_depth_fill_rule R;
  const int rc = check_depth_fill(h, "ssd_enqueue_depth_fill", d_frames, frame_stride_bytes, nframes, rule, d_out, out_stride_bytes, d_cls,
                                  cls_stride_bytes, &R);
  if(rc) return rc;
  return enqueue_depth_fill_impl(h, d_frames, frame_stride_bytes, nframes, static_cast<hipStream_t>(stream), R, d_out, out_stride_bytes, d_cls,
                                 cls_stride_bytes);
}

int ssd_fetch_depth_fill(ssd_handle *h, ssd_depth_fill_stats *out, int nframes, void *)
{
  return records_fetch(h, &ssd_handle::fill, out, nframes, "ssd_fetch_depth_fill", "ssd_enqueue_depth_fill", "frame");
}

int ssd_get_depth_fill_time(ssd_handle *h, float *ms)
{
  return pass_time(h, h ? &h->fill.pass : nullptr, "ssd_get_depth_fill_time", "ssd_enqueue_depth_fill", ms);
}

/* Host-fed: process_depth_host_pre with groups of one, as the edge filter's form */
int ssd_process_depth_host_fill(ssd_handle *h, const uint16_t *depth, int nframes, const ssd_depth_fill_rule *rule, ssd_frame_result *results,
                                uint16_t *filled, ssd_depth_fill_stats *stats)
{
  const std::string me("ssd_process_depth_host_fill");
  int rc = check_host_batch(h, me.c_str(), h && depth && results, nframes, SSD_INPUT_DEPTH16, kHandleCal);
  ssd_depth_fill_rule R;
  if(!rc) rc = check_fill_rule(me, rule, &R);
  if(rc) return rc;
  return process_depth_host_pre(h, me, "filled", depth, nframes, 1, results, filled,
    [&](const void *buf, size_t stride, int, int cnt, unsigned char *stage, size_t stageStride)
    {
      return enqueue_depth_fill_impl(h, buf, stride, cnt, h->ingestCompute, R, stage, stageStride, nullptr, 0);
    },
    [&](int at, int cnt) { return stats ? ssd_fetch_depth_fill(h, stats + at, cnt, nullptr) : static_cast<int>(SSD_OK); });
}

/* a slice's scratch plane between two pre-passes on ingestCompute (warpStage, fillStage): at least `need` bytes; it grows only behind
 * what that stream holds, which is all that reads it */
static int slice_stage_grow(ssd_handle *h, ssd::DeviceBuf<unsigned char> &buf, size_t &cap, size_t need, const std::string &me, const char *kind)
{
  if(cap >= need)
    return SSD_OK;
  HIP_TRY(hipStreamSynchronize(h->ingestCompute));
  buf.reset();
  cap = 0;
  const hipError_t e = buf.alloc(need);
  if(e != hipSuccess)
    return hip_fail(e, me + ": the " + kind + " frames' buffer: ");
  cap = need;
  return SSD_OK;
}

/* Host-fed, disjoint groups of n: ssd_process_depth_host_warp_fused with the fill between its two pre-passes.  The slice is warped into
 * warpStage, that filled into fillStage (the fill reads its neighbours, so it cannot run in place), that fused into the staging buffer
 * the detection reads.  All three run on ingestCompute, each behind the one before and the next slice's warp behind this slice's fusion */
int ssd_process_depth_host_warp_fill_fused(ssd_handle *h, const uint16_t *depth, int nframes, int n, const ssd_depth_warp_view *views,
                                           const ssd_intrinsics *dst, const ssd_depth_fill_rule *fill_rule, const ssd_depth_fuse_rule *fuse_rule,
                                           ssd_frame_result *results, uint16_t *fused, ssd_depth_warp_stats *warp_stats,
                                           ssd_depth_fill_stats *fill_stats, ssd_depth_fuse_stats *fuse_stats)
{
  const std::string me("ssd_process_depth_host_warp_fill_fused");
  int rc = check_host_batch(h, me.c_str(), h && depth && results, nframes, SSD_INPUT_DEPTH16, kHandleCal);
  ssd_depth_fuse_rule R;
  ssd_depth_fill_rule Q;
  if(!rc) rc = check_fuse_rule(me, n, fuse_rule, &R);
  if(!rc) rc = check_fill_rule(me, fill_rule, &Q);
  if(!rc) rc = check_warp_views(me, views, nframes, dst);
  if(rc) return rc;
  if(n > h->F || nframes % n != 0)
    return fail(SSD_E_ARG, me + ": n must not exceed max_frames_per_batch and nframes must be a multiple of n");
  if(h->P.nPoints % 2 != 0)
    return fail(SSD_E_ARG, me + ": width * height must be even (the output is written in 32-bit words)");
  if(std::memcmp(dst, &h->intr, sizeof(*dst)) != 0)
    return fail(SSD_E_ARG, me + ": dst must be the intrinsics the handle detects under (ssd_set_intrinsics)");
  return process_depth_host_pre(h, me, "fused", depth, nframes, n, results, fused,
    [&](const void *buf, size_t stride, int at, int cnt, unsigned char *stage, size_t stageStride)
    {
      const size_t need = static_cast<size_t>(cnt) * stride;
      int r = slice_stage_grow(h, h->warpStage, h->warpStageCap, need, me, "warped");
      if(!r) r = slice_stage_grow(h, h->fillStage, h->fillStageCap, need, me, "filled");
      if(!r) r = check_warp_words(h, me, h->warpStage.get(), stride);
      if(!r) r = enqueue_depth_warp_impl(h, buf, stride, cnt, h->ingestCompute, views + at, *dst, h->warpStage.get(), stride);
      if(!r) r = enqueue_depth_fill_impl(h, h->warpStage.get(), stride, cnt, h->ingestCompute, Q, h->fillStage.get(), stride, nullptr, 0);
      if(!r) r = enqueue_depth_fuse_impl(h, h->fillStage.get(), stride, h->ingestCompute, n, n, cnt / n, R, stage, stageStride, nullptr, 0);
      return r;
    },
    [&](int g0, int groups)
    {
      int r = warp_stats ? ssd_fetch_depth_warp(h, warp_stats + static_cast<size_t>(g0) * n, groups * n, nullptr) : static_cast<int>(SSD_OK);
      if(!r && fill_stats) r = ssd_fetch_depth_fill(h, fill_stats + static_cast<size_t>(g0) * n, groups * n, nullptr);
      if(!r && fuse_stats) r = ssd_fetch_depth_fuse(h, fuse_stats + g0, groups, nullptr);
      return r;
    });
}

int ssd_get_debug(ssd_handle *h, int frame, ssd_debug_frame *out)
{
  if(!h || !out)
    return fail(SSD_E_ARG, "ssd_get_debug: null");
  if(!h->dDebug || frame < 0 || frame >= h->lastFrames)
    return fail(SSD_E_ARG, "ssd_get_debug: debug capture off or frame out of range");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, &h->dDebug[frame].d, sizeof(ssd_debug_frame), hipMemcpyDeviceToHost));
  return SSD_OK;
}

int ssd_get_debug_image(ssd_handle *h, int frame, int step_slot, int closed, uint8_t *out)
{
  if(!h || !out)
    return fail(SSD_E_ARG, "ssd_get_debug_image: null");
  if(!h->dDebugImg || h->debug != 1 || frame < 0 || frame >= h->lastFrames || step_slot < -1 || step_slot >= h->P.maxStepImages)
    return fail(SSD_E_ARG, "ssd_get_debug_image: image capture off (ssd_set_debug(h, 1)) or index out of range");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const int slot = step_slot < 0 ? h->P.maxStepImages : step_slot;
  const unsigned long long *src = h->dDebugImg +
    ((static_cast<size_t>(frame) * (h->P.maxStepImages + 1) + slot) * 2 + (closed ? 1 : 0)) * h->imgWords;
  std::vector<unsigned long long> words(h->imgWords);
  HIP_TRY(hipMemcpy(words.data(), src, h->imgWords * 8, hipMemcpyDeviceToHost));
  const int W = h->P.W, H = h->P.H, W64 = h->P.W64;
  for(int y = 0; y < H; y++)
    for(int x = 0; x < W; x++)
      out[static_cast<size_t>(y) * W + x] = ((words[static_cast<size_t>(y) * W64 + (x >> 6)] >> (x & 63)) & 1ull) ? 0xff : 0;
  return SSD_OK;
}

} // extern "C"
