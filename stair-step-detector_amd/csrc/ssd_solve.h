/*
 * ssd_solve.h — the solve the fits share (DESIGN.md sections 7c, 7d, 7g and 7i): integer moments -> the centred scatter, exact in
 * 128-bit integers -> its eigenvalues and eigenvectors (cyclic Jacobi) -> the plane of lambda_min, and the trimmed refit's gate rule
 * on top of it; and camera_to_world_from_plane, the pose a floor's plane gives (section 7j).  Stated once for the host
 * (ssd_ground_fit_solve, ssd_surface_fit_solve, ssd_riser_fit_solve, ssd_surface_gates_from_moments, the calibrations from a plane
 * and from points: ssd_host.cpp) and the device (k_surface_gates: ssd_kernels_solve.hip, k_camera_ground_gates: ssd_kernels_fold.hip).
 * Both sides are compiled without FMA contraction; every operation is +, -, *, /, sqrt or a comparison of doubles, each correctly
 * rounded on both sides, in one order: they agree bit for bit (tests/golden/solve_goldens.json holds the host to the text this was
 * moved from, tests/test_gpu_surface_gates.py the device to the host).  Nothing transcendental is here: atan2 and asin stay in the
 * host-only solves.
 */
#ifndef SSD_SOLVE_H_
#define SSD_SOLVE_H_

#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>

#include "../../include/ssd_hip.h"
#include "ssd_moments.h"

namespace ssd
{

/* x[i] of three values by selection: no array is indexed by a run-time number, so on the device everything stays in registers */
__host__ __device__ inline double solve_pick(double x0, double x1, double x2, int i) { return i == 0 ? x0 : i == 1 ? x1 : x2; }

/* eigenvalues (ascending) and eigenvectors (columns of v) of a symmetric 3 x 3 matrix: cyclic Jacobi.  The order is a stable
 * insertion sort of the three diagonal entries by <, first to last: what std::sort runs at this length. */
__host__ __device__ inline void jacobi3(double a[3][3], double lambda[3], double v[3][3])
{
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
      v[i][j] = i == j ? 1.0 : 0.0;
  for(int sweep = 0; sweep < 64; sweep++)
  {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    if(off == 0.0)
      break;
#pragma unroll
    for(int p = 0; p < 2; p++)
#pragma unroll
      for(int q = p + 1; q < 3; q++)
      {
        if(a[p][q] == 0.0)
          continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        const double app = a[p][p], aqq = a[q][q], apq = a[p][q];
        a[p][p] = app - t * apq;
        a[q][q] = aqq + t * apq;
        a[p][q] = a[q][p] = 0.0;
        const int r = 3 - p - q;
        const double arp = a[r][p], arq = a[r][q];
        a[r][p] = a[p][r] = c * arp - s * arq;
        a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
        for(int k = 0; k < 3; k++)
        {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
  const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
  int o0 = 0, o1 = 1, o2 = 2;
  if(d1 < d0)                                   /* the second entry in front of the first */
  {
    o0 = 1; o1 = 0;
  }
  const double e0 = o0 == 0 ? d0 : d1, e1 = o1 == 0 ? d0 : d1;
  if(d2 < e0)                                   /* the third entry: to the front, ... */
  {
    o2 = o1; o1 = o0; o0 = 2;
  }
  else if(d2 < e1)                              /* ... or between the two */
  {
    o2 = o1; o1 = 2;
  }
  const int order[3] = { o0, o1, o2 };
  double vv[3][3];
#pragma unroll
  for(int k = 0; k < 3; k++)
  {
    lambda[k] = solve_pick(d0, d1, d2, order[k]);
#pragma unroll
    for(int i = 0; i < 3; i++)
      vv[i][k] = solve_pick(v[i][0], v[i][1], v[i][2], order[k]);
  }
#pragma unroll
  for(int i = 0; i < 3; i++)
#pragma unroll
    for(int k = 0; k < 3; k++)
      v[i][k] = vv[i][k];
}

/* The core of the solve, shared by the ground fit, the surface fit, the riser fit and the gates: moments -> the centred scatter
 * N SS - S (x) S, exact in 128-bit integers, converted once to double (to nearest, ties to even) and scaled to m^2; its eigenvalues
 * ascending (cyclic Jacobi); n0 = the unit eigenvector of lambda_min signed away from the camera (dist = n0 . centroid >= 0).
 * Returns FEW, DEGENERATE (the points determine no plane) or OK. */
struct PlaneOfMoments
{
  double lambda[3], n0[3], centroid[3], dist;
};

__host__ __device__ inline int plane_of_moments(const ssd_ground_moments *m, int min_points, PlaneOfMoments &pl)
{
  const int64_t n = m->n;
  if(n < (min_points > 1 ? min_points : 1))
    return SSD_GF_FEW;
  /* the centred scatter N SS - S (x) S, exact: N < 2^23 and SS < 2^63, |S| < 2^43, so both products lie below 2^86 */
  typedef __int128 i128;
  const double scale = 1.0 / (static_cast<double>(n) * static_cast<double>(n) * kGroundScale * kGroundScale);
  const int64_t s[3] = { m->s[0], m->s[1], m->s[2] };
  const int64_t ss[3][3] = { { m->ss[0], m->ss[1], m->ss[2] }, { m->ss[1], m->ss[3], m->ss[4] }, { m->ss[2], m->ss[4], m->ss[5] } };
  double c[3][3], v[3][3];
  double (&lambda)[3] = pl.lambda;
#pragma unroll
  for(int i = 0; i < 3; i++)
#pragma unroll
    for(int j = 0; j < 3; j++)
      c[i][j] = static_cast<double>(static_cast<i128>(n) * ss[i][j] - static_cast<i128>(s[i]) * s[j]) * scale;   /* m^2 */
  jacobi3(c, lambda, v);
  /* an eigenvalue at the rounding level of the largest one is zero (collinear points leave +-1e-17 lambda_max, of either sign) */
  const double zero = 64.0 * 2.220446049250313e-16 * lambda[2];
  const double lmin = lambda[0] > zero ? lambda[0] : 0.0, lmid = lambda[1] > zero ? lambda[1] : 0.0;
  if(!(lmid > 0.0) || lmid < SSD_GF_PLANARITY * lmin)
    return SSD_GF_DEGENERATE;
  double (&n0)[3] = pl.n0;
  n0[0] = v[0][0]; n0[1] = v[1][0]; n0[2] = v[2][0];
  const double rn = 1.0 / sqrt(n0[0] * n0[0] + n0[1] * n0[1] + n0[2] * n0[2]);
  double (&centroid)[3] = pl.centroid;
#pragma unroll
  for(int i = 0; i < 3; i++)
  {
    n0[i] *= rn;
    centroid[i] = static_cast<double>(s[i]) / (static_cast<double>(n) * kGroundScale);
  }
  double dist = n0[0] * centroid[0] + n0[1] * centroid[1] + n0[2] * centroid[2];
  if(dist < 0.0)
  {
    dist = -dist;
#pragma unroll
    for(int i = 0; i < 3; i++)
      n0[i] = -n0[i];
  }
  pl.dist = dist;
  return SSD_GF_OK;
}

/* CameraToWorld from the floor's plane in camera coordinates (unit normal n0 pointing away from the camera, dist = n0 . a point of
 * the plane): the rest of Transformation_<3>(triangleInPlane), transformation.cpp:108-157, behind its normal.  Shared by
 * ssd_calibration_from_points, ssd_calibration_from_plane and ssd_ground_fit_solve on the host and by k_camera_ground_gates on the
 * device (which needs only whether it succeeds: section 7j); false in the degenerate cases (reference assert, transformation.cpp:153). */
__host__ __device__ inline bool camera_to_world_from_plane(double n0x, double n0y, double n0z, double dist, double a[9], double b[3])
{
  struct V3 { double x, y, z; };
  auto cross = [](V3 p, V3 q) { return V3{ p.y * q.z - p.z * q.y, p.z * q.x - p.x * q.z, p.x * q.y - p.y * q.x }; };
  auto norm = [](V3 p)
  {
    const double m2 = p.x * p.x + p.y * p.y + p.z * p.z;
    const double rm = 1.0 / sqrt(m2);
    return V3{ p.x * rm, p.y * rm, p.z * rm };
  };
  const V3 zB{ -n0x, -n0y, -n0z };
  const V3 yB = norm(V3{ 0.0, -zB.z / zB.y, 1.0 });
  const V3 xB = cross(yB, zB);
  if(!(dist > 0.0) || !std::isfinite(yB.y) || !std::isfinite(xB.x))
    return false;
  a[0] = xB.x; a[1] = xB.y; a[2] = xB.z;
  a[3] = yB.x; a[4] = yB.y; a[5] = yB.z;
  a[6] = zB.x; a[7] = zB.y; a[8] = zB.z;
  b[0] = 0.0; b[1] = 0.0; b[2] = dist;
  return true;
}

/* The gate rule of the trimmed refit (ssd_surface_gates_from_moments, k_surface_gates): the fitted plane in camera coordinates and
 * gate = max(k_sigma * rms, gate_min), rms = sqrt(max(lambda_min, 0)); an all-zero gate unless the status is SSD_GF_OK. */
__host__ __device__ inline ssd_plane_gate gate_of_moments(const ssd_ground_moments *m, int min_points, double k_sigma, double gate_min)
{
  ssd_plane_gate g;
  g.n[0] = 0.0; g.n[1] = 0.0; g.n[2] = 0.0;
  g.dist = 0.0;
  g.gate = 0.0;
  PlaneOfMoments pl;
  if(plane_of_moments(m, min_points, pl) != SSD_GF_OK)
    return g;                                   /* an all-zero gate: the surface gathers nothing */
  g.n[0] = pl.n0[0]; g.n[1] = pl.n0[1]; g.n[2] = pl.n0[2];
  g.dist = pl.dist;
  const double rms = sqrt(pl.lambda[0] > 0.0 ? pl.lambda[0] : 0.0), wide = k_sigma * rms;
  g.gate = wide > gate_min ? wide : gate_min;
  return g;
}

} // namespace ssd

#endif /* SSD_SOLVE_H_ */
