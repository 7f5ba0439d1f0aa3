/*
 * ssd_clearance.h — the tread clearance rule (include/ssd_hip.h), stated once for the device (k_clearance and
 * k_clearance_cams, ssd_kernels_clearance.hip) and the host (ssd_clearance_host, ssd_host.cpp), and the kernels' launcher.
 * The rule speaks of public data only: a frame's ssd_frame_result, the calibration, the point.  Both sides are compiled without FMA
 * contraction and every operation is +, -, * or a comparison of doubles in one order; the rule decides only WHICH points are summed, and
 * everything summed is an integer by the fixed-point rule of ssd_moments.h: they agree bit for bit.
 */
#ifndef SSD_CLEARANCE_H_
#define SSD_CLEARANCE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/ssd_hip.h"

namespace ssd
{

/* ToExternalWorld as the rule reads it (ssd_calibration's r2, t2, world_z) */
struct ClearanceWorld
{
  double r2[4], t2[2], worldZ;
};

/* One side of a surface's ring: its start, its direction, and margin^2 |direction|^2, which the squared cross product is held against */
struct ClearanceSide
{
  double x, y, dx, dy, m2;
};

/* A surface as the rule reads it: its height, the ring's orientation (+1 / -1; 0: the surface takes nothing) and the four sides */
struct ClearanceSurface
{
  double height, o;
  ClearanceSide side[4];
};

/* the ranges a rule must lie in: margin in [0, 1], lo in (0, 1], hi in (lo, 8]; a NaN fails */
inline bool clearance_rule_ok(const ssd_clearance_rule &r)
{
  return r.margin >= 0.0 && r.margin <= 1.0 && r.lo > 0.0 && r.lo <= 1.0 && r.hi > r.lo && r.hi <= 8.0;
}

/* A reported step as a ClearanceSurface.  Ring: FL, FR, BR, BL = quad[0..1], [2..3], [6..7], [4..5]; twice the signed area
 * A2 = ((t0 + t1) + t2) + t3 with t_i = x_i y_(i+1) - x_(i+1) y_i; A2 == 0 or unordered (a NaN corner): nothing is taken - quirk Q6's
 * all-zero ground among them. */
__host__ __device__ inline void clearance_surface(const ssd_step &s, double margin, ClearanceSurface &out)
{
  const double x[4] = { s.quad[0], s.quad[2], s.quad[6], s.quad[4] };
  const double y[4] = { s.quad[1], s.quad[3], s.quad[7], s.quad[5] };
  double t[4];
#pragma unroll
  for(int i = 0; i < 4; i++)
  {
    const int n = (i + 1) & 3;
    t[i] = x[i] * y[n] - x[n] * y[i];
    ClearanceSide &e = out.side[i];
    e.x = x[i];
    e.y = y[i];
    e.dx = x[n] - x[i];
    e.dy = y[n] - y[i];
    e.m2 = (margin * margin) * (e.dx * e.dx + e.dy * e.dy);
  }
  const double a2 = ((t[0] + t[1]) + t[2]) + t[3];
  out.height = s.height;
  out.o = a2 > 0.0 ? 1.0 : a2 < 0.0 ? -1.0 : 0.0;
}

/* Is (ex, ey) inside the surface's quadrilateral shrunk by the margin?  Per side c = o (dx (ey - y_i) - dy (ex - x_i)), kept iff
 * c >= 0 and c c >= margin^2 (dx^2 + dy^2) on all four: no square root, no division; a NaN anywhere keeps nothing. */
__host__ __device__ inline bool clearance_inside(const ClearanceSurface &S, double ex, double ey)
{
  if(S.o == 0.0)
    return false;
  bool in = true;
#pragma unroll
  for(int i = 0; i < 4; i++)
  {
    const ClearanceSide &e = S.side[i];
    const double c = S.o * (e.dx * (ey - e.y) - e.dy * (ex - e.x));
    in = in && c >= 0.0 && c * c >= e.m2;
  }
  return in;
}

/* the slab exclusion: a point within lo of ANY reported height belongs to the surfaces, whatever their quadrilaterals say */
__host__ __device__ inline bool clearance_in_slab(const ClearanceSurface *S, int n, double ez, double lo)
{
  bool slab = false;
  for(int j = 0; j < n; j++)
    slab = slab || !(__builtin_fabs(ez - S[j].height) > lo);
  return slab;
}

/* is the point's height in surface k's band, strictly */
__host__ __device__ inline bool clearance_in_band(const ClearanceSurface &S, double ez, double lo, double hi)
{
  return ez > S.height + lo && ez < S.height + hi;
}

/* external-world position of a camera-dependent world point (transformation.cpp:209-211), row sums left to right */
__host__ __device__ inline void clearance_external(const ClearanceWorld &X, double wx, double wy, double &ex, double &ey)
{
  ex = (X.r2[0] * wx + X.r2[1] * wy) + X.t2[0];
  ey = (X.r2[2] * wx + X.r2[3] * wy) + X.t2[1];
}

/* The surface a point outside every slab occupies: the lowest k among `candidates` (bit k; a superset of the surfaces whose band holds ez
 * gives the same answer as all of them) whose band holds ez and whose shrunk quadrilateral holds (ex, ey); -1: none */
__host__ __device__ inline int clearance_lowest(const ClearanceSurface *S, unsigned int candidates, double ex, double ey, double ez, double lo, double hi)
{
  while(candidates != 0u)
  {
    const int k = __builtin_ctz(candidates);
    candidates &= candidates - 1u;
    if(clearance_in_band(S[k], ez, lo, hi) && clearance_inside(S[k], ex, ey))
      return k;
  }
  return -1;
}

/* k_clearance behind a whole run of the chain on the same workspace (k_clearance_cams behind a whole cameras batch, under the table and
 * that workspace's index): launch_surface_refit's arguments with the rule in place of the gates.  results: the batch's records as k_final
 * wrote them (device-addressable), frame i's at results + i; out: frame i's record at out + i; mask (may be null): frame i's W H bytes at
 * mask + i * maskStride - both zeroed by the caller on the stream in front of the launch, which only adds and stores occupants' bytes */
struct Batch;                                 /* ssd_launch.h */
void launch_clearance(const Batch &B, int chunkPoints, const ssd_frame_result *results, const ssd_clearance_rule &rule, ssd_frame_moments *out,
                      unsigned char *mask, size_t maskStride);

} // namespace ssd

#endif /* SSD_CLEARANCE_H_ */
