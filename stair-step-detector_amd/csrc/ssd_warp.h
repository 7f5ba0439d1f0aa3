/*
 * ssd_warp.h — the depth warp's per-sample rule (include/ssd_hip.h), stated once for the device (k_depth_warp,
 * ssd_k_warp.h) and the host (ssd_depth_warp_host, ssd_host.cpp), and the kernel's launcher.  The point in float as ssd_deproject_host
 * makes it, everything behind it in doubles, no FMA (-ffp-contract=off on both sides), every division and floor IEEE: both sides agree
 * byte for byte.  What a sample's class, its target pixel and its value ARE stands here; the minimum per target pixel is the caller's.
 */
#ifndef SSD_WARP_H_
#define SSD_WARP_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ssd_hip.h"

namespace ssd
{

constexpr int kWarpWords = 8;               /* ssd_depth_warp_stats as int64 words, in its order; the last two stay 0 */
constexpr int kWarpSums = 6;
/* a sample's class is the index of its count in the record; kWarpNFilled counts output pixels, not samples */
enum { kWarpNEmpty = 0, kWarpNBehind, kWarpNRange, kWarpNOutside, kWarpNLanded, kWarpNFilled };

/* the target's intrinsics as the rule uses them: promoted once */
struct WarpTarget
{
  double fx, fy, ppx, ppy, units;
};

__host__ __device__ inline WarpTarget warp_target(const ssd_intrinsics &dst)
{
  return WarpTarget{ static_cast<double>(dst.fx), static_cast<double>(dst.fy), static_cast<double>(dst.ppx), static_cast<double>(dst.ppy),
                     static_cast<double>(dst.depth_units) };
}

/* rs2::pointcloud's maps under the source's intrinsics, as ssd_deproject_host computes them (float, one correctly rounded division) */
__host__ __device__ inline float warp_map_x(const ssd_intrinsics &src, int u) { return (static_cast<float>(u) - src.ppx) / src.fx; }
__host__ __device__ inline float warp_map_y(const ssd_intrinsics &src, int v) { return (static_cast<float>(v) - src.ppy) / src.fy; }

/* Steps 1 to 7 for the sample d at a source pixel whose maps' values are xm and ym: its class, and where it LANDED the target pixel
 * (a, b) and the value q (1 .. 65535) */
__host__ __device__ inline int warp_sample(const ssd_depth_warp_view &V, const WarpTarget &T, int W, int H, uint32_t d, float xm, float ym,
                                           int &a, int &b, uint32_t &q)
{
  a = 0; b = 0; q = 0u;
  if(d == 0u)
    return kWarpNEmpty;
  /* step 2: deproject4's expressions (ssd_k_point.h), ssd_deproject_host's order */
  const float dm = static_cast<float>(d) * V.src.depth_units;
  const float xf = dm * xm, yf = dm * ym;
  const double x = xf, y = yf, z = dm;
  /* step 3: as K1 writes its rows - row sums left to right, then the translation */
  const double X = ((V.r[0] * x + V.r[1] * y) + V.r[2] * z) + V.t[0];
  const double Y = ((V.r[3] * x + V.r[4] * y) + V.r[5] * z) + V.t[1];
  const double Z = ((V.r[6] * x + V.r[7] * y) + V.r[8] * z) + V.t[2];
  if(!(Z > 0.0))
    return kWarpNBehind;
  const double qf = floor(Z / T.units + 0.5);
  if(!(qf >= 1.0 && qf <= 65535.0))
    return kWarpNRange;
  const double uf = (X / Z) * T.fx + T.ppx, vf = (Y / Z) * T.fy + T.ppy;
  const double af = floor(uf + 0.5), bf = floor(vf + 0.5);
  if(!(af >= 0.0 && af < static_cast<double>(W) && bf >= 0.0 && bf < static_cast<double>(H)))   /* in doubles: a NaN fails it */
    return kWarpNOutside;
  a = static_cast<int>(af);
  b = static_cast<int>(bf);
  q = static_cast<uint32_t>(qf);
  return kWarpNLanded;
}

/* what a target pixel holding `old` (0: nothing landed yet) holds once q has landed on it */
__host__ __device__ inline uint32_t warp_min(uint32_t old, uint32_t q) { return old == 0u ? q : (old < q ? old : q); }

/* k_depth_warp over nframes frames of W x H uint16 (frame i at frames + i * strideBytes, rows packed) under views[i] (device memory):
 * warped frame i at out + i * outStride, which the caller zeroed on the stream (0: nothing landed) - the frames' own bytes only; adds
 * into stats[i], zeroed likewise.  out and outStride are multiples of 4 and W * H is even (the kernel swaps whole 32-bit words) */
void launch_depth_warp(const void *frames, size_t strideBytes, int W, int H, int nframes, const ssd_depth_warp_view *views,
                       const ssd_intrinsics &dst, void *out, size_t outStride, ssd_depth_warp_stats *stats, hipStream_t s);

} // namespace ssd

#endif /* SSD_WARP_H_ */
