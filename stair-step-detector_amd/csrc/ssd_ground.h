/*
 * ssd_ground.h — the ground fit's floor-point rule (include/ssd_hip.h), stated once for the device
 * (k_ground_moments, ssd_kernels_ground.hip) and the host (ssd_ground_moments_host, ssd_host.cpp), and the kernel's launcher.
 * Both sides are compiled without FMA contraction, and everything summed is an integer: they agree bit for bit.
 */
#ifndef SSD_GROUND_H_
#define SSD_GROUND_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ssd_moments.h"

namespace ssd
{

/* one frame's prior as the kernel reads it: CameraToWorld and, for 16-bit depth input, the intrinsics */
struct GroundPrior
{
  double a[9], b[3];
  float ppx, ppy, fx, fy, depthUnits;
  int pad[3];
};

/* what every frame of a call shares: the handle's x / y measuring range and the call's tolerance */
struct GroundRange
{
  double xMin, xMax, yMin, yMax, tol;
};

/* One point into a lane's / the host's sums, by the fixed-point rule of ssd_moments.h (kGroundSums, moment_round, moment_near,
 * moment_add: the overflow argument stands there) */
__host__ __device__ inline void ground_point(const GroundPrior &C, const GroundRange &R, float fx, float fy, float fz, long long (&acc)[kGroundSums])
{
  if(!(fz > 0.0f))
    return;
  const double x = fx, y = fy, z = fz;
  /* CameraToWorld as K1's doubles (ssd_prefilter.h, world_rows): row sums left to right, then the translation */
  double wx = (C.a[0] * x + C.a[1] * y) + C.a[2] * z;
  double wy = (C.a[3] * x + C.a[4] * y) + C.a[5] * z;
  double wz = (C.a[6] * x + C.a[7] * y) + C.a[8] * z;
  wx = wx + C.b[0];
  wy = wy + C.b[1];
  wz = wz + C.b[2];
  const double rx = moment_round(x), ry = moment_round(y), rz = moment_round(z);
  const bool nx = moment_near(rx), ny = moment_near(ry), nz = moment_near(rz);
  const bool floor = (wx > R.xMin) & (wx < R.xMax) & (wy > R.yMin) & (wy < R.yMax) & (wz >= -R.tol) & (wz <= R.tol) &
                     nx & ny & nz;
  if(!floor)
    return;
  moment_add(rx, ry, rz, acc);
}

/* rs2::pointcloud's maps as ssd_deproject_host computes them (float arithmetic, one correctly rounded division each) */
__host__ __device__ inline float ground_map_x(const GroundPrior &C, int u) { return (static_cast<float>(u) - C.ppx) / C.fx; }
__host__ __device__ inline float ground_map_y(const GroundPrior &C, int v) { return (static_cast<float>(v) - C.ppy) / C.fy; }

/* k_ground_moments<SRC> over nframes frames (frame i at frames + i * strideBytes; W * H points each; depthInput: uint16 depth, else
 * xyz floats), frame i with priors[i * priorStep]; adds into records[i * kGroundSums ..], which the caller zeroed on the stream */
void launch_ground_moments(const void *frames, size_t strideBytes, int W, int H, int nframes, bool depthInput, const GroundPrior *priors,
                           int priorStep, const GroundRange &R, long long *records, hipStream_t s);

} // namespace ssd

#endif /* SSD_GROUND_H_ */
