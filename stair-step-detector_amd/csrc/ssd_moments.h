/*
 * ssd_moments.h — the fixed-point rule of the integer moments (include/ssd_hip.h: ssd_ground_moments), stated once for the ground fit
 * (ssd_ground.h: k_ground_moments, ssd_ground_moments_host) and the surface fit (k_surface_moments in ssd_kernels.hip,
 * ssd_surface_moments_host): q = llrint(double(v) * 65536.0) per camera coordinate, a point with some |q| >= 2^20 is not summed,
 * and the ten sums n, s[3], ss[6] of the others.  Everything summed is an integer: device and host agree bit for bit.
 */
#ifndef SSD_MOMENTS_H_
#define SSD_MOMENTS_H_

#include <hip/hip_runtime.h>

namespace ssd
{

constexpr int kGroundSums = 10;               /* ssd_ground_moments as 10 int64: n, s[3], ss[6] */
constexpr double kGroundScale = 65536.0;      /* 2^-16 m fixed point */
constexpr double kGroundLimit = 1048576.0;    /* |q| < 2^20, |v| < 16 m */

/* q = llrint(v * 2^16) as the rounded double (the product is exact: a power of two), so that no conversion is out of range */
__host__ __device__ inline double moment_round(double v) { return __builtin_rint(v * kGroundScale); }
/* ... and whether it may be summed */
__host__ __device__ inline bool moment_near(double r) { return __builtin_fabs(r) < kGroundLimit; }

/* One point (its three rounded coordinates, each moment_near) into a lane's / the host's sums.  Overflow: |q| < 2^20, so a product is
 * below 2^40; a frame has at most 3175 * 2560 < 2^23 points (ssd_hip.h, configuration limits), so every sum stays below 2^63: int64 is
 * exact, whatever the order. */
template<typename Acc>
__host__ __device__ inline void moment_add(double rx, double ry, double rz, Acc &acc)
{
  const long long qx = static_cast<int>(rx), qy = static_cast<int>(ry), qz = static_cast<int>(rz);
  acc[0] += 1;
  acc[1] += qx; acc[2] += qy; acc[3] += qz;
  acc[4] += qx * qx; acc[5] += qx * qy; acc[6] += qx * qz;
  acc[7] += qy * qy; acc[8] += qy * qz;
  acc[9] += qz * qz;
}

} // namespace ssd

#endif /* SSD_MOMENTS_H_ */
