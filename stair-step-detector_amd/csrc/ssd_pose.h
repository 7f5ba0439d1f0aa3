/*
 * ssd_pose.h — the stair pose's rule (include/ssd_hip.h), stated once for the device (k_stair_pose,
 * ssd_kernels_pose.hip) and the host (ssd_stair_pose_host, ssd_host.cpp), the fold's step, and the kernel's launcher.  Built on
 * ssd_ground.h (the prior as the kernel reads it, the depth maps), ssd_clearance.h (the external world of a point, a tread's shrunk
 * quadrilateral) and ssd_moments.h (the fixed-point sums), which stay as they are.  Both sides are compiled without FMA contraction and
 * every operation is +, -, * or a comparison of doubles in one order; the rule decides only WHICH class a point is summed into, and
 * everything summed is an integer: they agree bit for bit.
 */
#ifndef SSD_POSE_H_
#define SSD_POSE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ssd_hip.h"
#include "ssd_clearance.h"
#include "ssd_ground.h"
#include "ssd_moments.h"

namespace ssd
{

constexpr int kPoseTreads = SSD_MAX_STEPS;             /* tread classes: 0 .. 16 */
constexpr int kPoseRisers = SSD_MAX_STEPS - 1;         /* riser classes: 17 .. 32 */
constexpr int kPoseClasses = kPoseTreads + kPoseRisers;
constexpr int kPoseSums = kGroundSums + 1;             /* the ten sums and n_far: an ssd_surface_moments */
constexpr int kPoseWords = kPoseClasses * kPoseSums;   /* 363 int64 of a record that are ever added to */

static_assert(sizeof(ssd_surface_moments) == sizeof(int64_t) * kPoseSums, "a class is the ten sums and n_far");
static_assert(sizeof(ssd_frame_moments) == 8 + sizeof(ssd_surface_moments) * SSD_MAX_STEPS && sizeof(ssd_stair_pose_moments) == 2 * sizeof(ssd_frame_moments),
              "a record is two ssd_frame_moments");

/* the ranges a rule must lie in: margin in [0, 1], band, clear and reach in (0, 1]; a NaN fails */
inline bool pose_rule_ok(const ssd_stair_pose_rule &r)
{
  return r.margin >= 0.0 && r.margin <= 1.0 && r.band > 0.0 && r.band <= 1.0 && r.clear > 0.0 && r.clear <= 1.0 && r.reach > 0.0 && r.reach <= 1.0;
}

/* A riser as the rule reads it: the interval of heights, strictly, and the front edge of the step above - its start, its direction, its
 * squared length and reach^2 times that, which the squared cross product is held against.  live: L2 > 0 (a NaN: not live) */
struct PoseRiser
{
  double lo, hi, x, y, dx, dy, l2, r2;
  int live, pad;
};

/* A target as the kernel reads it: the prior (CameraToWorld and the intrinsics: GroundPrior; ToExternalWorld: ClearanceWorld), the
 * record's headers, the rule's band, and the map's treads and risers.  nSteps == 0: the record stays all zero (a thrown or empty map). */
struct PoseTarget
{
  GroundPrior cam;
  ClearanceWorld world;
  double band;
  int nSteps, ground;
  ClearanceSurface tread[kPoseTreads];
  PoseRiser riser[kPoseRisers];
};
static_assert(sizeof(PoseTarget) % 8 == 0 && alignof(PoseTarget) == 8, "a target is copied into LDS in 8-byte words");

/* the x / y measuring range of the handle */
struct PoseRange
{
  double xMin, xMax, yMin, yMax;
};

/* a caller's target and rule as a PoseTarget (the map's n_steps lies in 0 .. SSD_MAX_STEPS: the callers have refused anything else) */
inline void pose_target_fill(PoseTarget &T, const ssd_stair_pose_target &t, bool depth, const ssd_stair_pose_rule &rule)
{
  T = PoseTarget{};
  const ssd_calibration &cal = t.prior.cal;
  for(int i = 0; i < 9; i++) T.cam.a[i] = cal.a[i];
  for(int i = 0; i < 3; i++) T.cam.b[i] = cal.b[i];
  if(depth)
  {
    const ssd_intrinsics &in = t.prior.intr;
    T.cam.ppx = in.ppx; T.cam.ppy = in.ppy; T.cam.fx = in.fx; T.cam.fy = in.fy; T.cam.depthUnits = in.depth_units;
  }
  for(int i = 0; i < 4; i++) T.world.r2[i] = cal.r2[i];
  T.world.t2[0] = cal.t2[0]; T.world.t2[1] = cal.t2[1];
  T.world.worldZ = cal.world_z;
  T.band = rule.band;
  const ssd_frame_result &st = t.map.stairs;
  if((st.status & SSD_ST_THROW) || st.n_steps <= 0)
    return;
  T.nSteps = st.n_steps;
  T.ground = t.map.ground != 0 ? 1 : 0;
  for(int k = 0; k < st.n_steps; k++)
    clearance_surface(st.steps[k], rule.margin, T.tread[k]);
  for(int i = 0; i + 1 < st.n_steps; i++)
  {
    const ssd_step &up = st.steps[i + 1];
    PoseRiser &r = T.riser[i];
    r.lo = st.steps[i].height + rule.clear;
    r.hi = up.height - rule.clear;
    r.x = up.quad[0];
    r.y = up.quad[1];
    r.dx = up.quad[2] - up.quad[0];
    r.dy = up.quad[3] - up.quad[1];
    r.l2 = r.dx * r.dx + r.dy * r.dy;
    r.r2 = (rule.reach * rule.reach) * r.l2;
    r.live = r.l2 > 0.0 ? 1 : 0;
  }
}

/* is (ex, ey) within reach of the vertical plane under the riser's edge, between the edge's ends */
__host__ __device__ inline bool pose_at_riser(const PoseRiser &r, double ex, double ey)
{
  const double a = ex - r.x, b = ey - r.y;
  const double c = b * r.dx - a * r.dy, t = a * r.dx + b * r.dy;
  return r.live != 0 && c * c <= r.r2 && t >= 0.0 && t <= r.l2;
}

/* The class of one point: -1 none, k < kPoseTreads tread k, kPoseTreads + i riser i; rx, ry, rz: its rounded camera coordinates
 * (moment_round), for the sums.  From ez alone first: which bands and which riser intervals can hold the point - the edge tests run
 * over those alone, lowest first. */
__host__ __device__ inline int pose_class(const GroundPrior &C, const ClearanceWorld &X, const PoseTarget &T, const PoseRange &R, float fx, float fy, float fz)
{
  if(!(fz > 0.0f))
    return -1;
  const double x = fx, y = fy, z = fz;
  /* CameraToWorld as K1's doubles (ssd_prefilter.h, world_rows): row sums left to right, then the translation */
  double wx = (C.a[0] * x + C.a[1] * y) + C.a[2] * z;
  double wy = (C.a[3] * x + C.a[4] * y) + C.a[5] * z;
  double wz = (C.a[6] * x + C.a[7] * y) + C.a[8] * z;
  wx = wx + C.b[0];
  wy = wy + C.b[1];
  wz = wz + C.b[2];
  if(!((wx > R.xMin) & (wx < R.xMax) & (wy > R.yMin) & (wy < R.yMax)))
    return -1;
  const double ez = wz + X.worldZ;
  const int n = T.nSteps;
  unsigned int treads = 0u, risers = 0u;
  for(int k = 0; k < n; k++)
    if(!(__builtin_fabs(ez - T.tread[k].height) > T.band))
      treads |= 1u << k;
  for(int i = 0; i + 1 < n; i++)
    if(ez > T.riser[i].lo && ez < T.riser[i].hi)
      risers |= 1u << i;
  if((treads | risers) == 0u)
    return -1;
  double ex, ey;
  clearance_external(X, wx, wy, ex, ey);
  while(treads != 0u)
  {
    const int k = __builtin_ctz(treads);
    treads &= treads - 1u;
    if(clearance_inside(T.tread[k], ex, ey))
      return k;
  }
  while(risers != 0u)
  {
    const int i = __builtin_ctz(risers);
    risers &= risers - 1u;
    if(pose_at_riser(T.riser[i], ex, ey))
      return kPoseTreads + i;
  }
  return -1;
}

/* a classified point into the eleven sums of its class: the ten by the fixed-point rule, or n_far */
template<typename Acc>
__host__ __device__ inline void pose_add(float fx, float fy, float fz, Acc &acc)
{
  const double rx = moment_round(static_cast<double>(fx)), ry = moment_round(static_cast<double>(fy)), rz = moment_round(static_cast<double>(fz));
  const bool near = moment_near(rx) && moment_near(ry) && moment_near(rz);
  /* the point's own ten sums first, then eleven unconditional additions: no element of acc is chosen by address, so a lane's sums
   * stay in registers */
  long long d[kGroundSums] = {};
  if(near)
    moment_add(rx, ry, rz, d);
#pragma unroll
  for(int i = 0; i < kGroundSums; i++)
    acc[i] += d[i];
  acc[kGroundSums] += near ? 0 : 1;
}

/* where class c's sums lie in a record, in int64 words from its start (word 0 and word 188 hold the two headers) */
__host__ __device__ inline int pose_word(int c)
{
  constexpr int half = static_cast<int>(sizeof(ssd_frame_moments) / sizeof(int64_t));
  return c < kPoseTreads ? 1 + c * kPoseSums : half + 1 + (c - kPoseTreads) * kPoseSums;
}

/* the headers of a target's record */
__host__ __device__ inline void pose_headers(int nSteps, int ground, int32_t head[4])
{
  head[0] = nSteps;
  head[1] = nSteps > 0 ? ground : 0;
  head[2] = nSteps > 1 ? nSteps - 1 : 0;
  head[3] = 0;
}

/* The fold's step over two records (ssd_stair_pose_add): false, and acc as it was, if a sum would leave int64 */
inline bool pose_fold(const ssd_stair_pose_moments &in, ssd_stair_pose_moments &acc)
{
  const ssd_frame_moments *a[2] = { &in.treads, &in.risers };
  ssd_frame_moments *b[2] = { &acc.treads, &acc.risers };
  for(int h = 0; h < 2; h++)
  {
    const int64_t *x = reinterpret_cast<const int64_t *>(a[h]->s), *y = reinterpret_cast<const int64_t *>(b[h]->s);
    int64_t t;
    for(int i = 0; i < SSD_MAX_STEPS * kPoseSums; i++)
      if(__builtin_add_overflow(x[i], y[i], &t))
        return false;
  }
  for(int h = 0; h < 2; h++)
  {
    const int64_t *x = reinterpret_cast<const int64_t *>(a[h]->s);
    int64_t *y = reinterpret_cast<int64_t *>(b[h]->s);
    b[h]->n_surfaces = a[h]->n_surfaces;
    b[h]->ground = a[h]->ground;
    for(int i = 0; i < SSD_MAX_STEPS * kPoseSums; i++)
      y[i] += x[i];
  }
  return true;
}

/* k_stair_pose over nframes frames (frame i at frames + i * strideBytes; W * H points each; depthInput: uint16 depth, else xyz floats),
 * frame i against targets[targetOf[i]] (device; an index not below ntargets: the frame adds nothing); adds into records[i], which the
 * caller zeroed on the stream, and writes its headers */
void launch_stair_pose(const void *frames, size_t strideBytes, int W, int H, int nframes, bool depthInput, const PoseTarget *targets, int ntargets,
                       const int *targetOf, const PoseRange &R, ssd_stair_pose_moments *records, hipStream_t s);

} // namespace ssd

#endif /* SSD_POSE_H_ */
