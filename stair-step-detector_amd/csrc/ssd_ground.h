/*
 * ssd_ground.h — the ground fit's floor-point rule (include/ssd_hip.h), stated once for the device
 * (k_ground_moments, ssd_kernels_ground.hip) and the host (ssd_ground_moments_host, ssd_capi.hip), and the kernel's launcher.
 * Both sides are compiled without FMA contraction, and everything summed is an integer: they agree bit for bit.
 */
#ifndef SSD_GROUND_H_
#define SSD_GROUND_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

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

constexpr int kGroundSums = 10;               /* ssd_ground_moments as 10 int64: n, s[3], ss[6] */
constexpr double kGroundScale = 65536.0;      /* 2^-16 m fixed point */
constexpr double kGroundLimit = 1048576.0;    /* |q| < 2^20, |v| < 16 m */

/* One point into a lane's / the host's sums.  Overflow: |q| < 2^20, so a product is below 2^40; a frame has at most
 * 3175 * 2560 < 2^23 points (ssd_hip.h, configuration limits), so every sum stays below 2^63: int64 is exact, whatever the order. */
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
  /* q = llrint(v * 2^16) on the rounded double (the product is exact: a power of two), so that no conversion is out of range */
  const double rx = __builtin_rint(x * kGroundScale), ry = __builtin_rint(y * kGroundScale), rz = __builtin_rint(z * kGroundScale);
  const bool floor = (wx > R.xMin) & (wx < R.xMax) & (wy > R.yMin) & (wy < R.yMax) & (wz >= -R.tol) & (wz <= R.tol) &
                     (__builtin_fabs(rx) < kGroundLimit) & (__builtin_fabs(ry) < kGroundLimit) & (__builtin_fabs(rz) < kGroundLimit);
  if(!floor)
    return;
  const long long qx = static_cast<int>(rx), qy = static_cast<int>(ry), qz = static_cast<int>(rz);
  acc[0] += 1;
  acc[1] += qx; acc[2] += qy; acc[3] += qz;
  acc[4] += qx * qx; acc[5] += qx * qy; acc[6] += qx * qz;
  acc[7] += qy * qy; acc[8] += qy * qz;
  acc[9] += qz * qz;
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
