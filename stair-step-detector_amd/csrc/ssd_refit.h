/*
 * ssd_refit.h — the trimmed surface refit's gate rule (include/ssd_hip.h), stated once for the device
 * (k_surface_refit and k_surface_refit_cams, ssd_kernels_refit.hip) and the host (ssd_surface_refit_moments_host, ssd_host.cpp), and the
 * kernels' launchers.
 * Both sides are compiled without FMA contraction; the gate decides only WHICH points are summed, and everything summed is an
 * integer by the fixed-point rule of ssd_moments.h: they agree bit for bit.
 */
#ifndef SSD_REFIT_H_
#define SSD_REFIT_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ssd_device.h"
#include "ssd_moments.h"

namespace ssd
{

/* a half-width that gathers anything: a finite number above 0 (NaN fails both comparisons) */
__host__ __device__ inline bool refit_gate_open(double gate) { return gate > 0.0 && gate < __builtin_inf(); }

/* Is a point that carries label k + 1 kept by its frame's gates?  The residual in doubles, the floats widened first, row sum left to
 * right, then the distance: ((n0 x + n1 y) + n2 z) - dist, no FMA.  A point exactly on the gate's edge is kept. */
__host__ __device__ inline bool refit_keeps(const ssd_frame_gates &G, int k, float fx, float fy, float fz)
{
  if(k >= G.n_surfaces)
    return false;
  const ssd_plane_gate &g = G.g[k];
  const double x = fx, y = fy, z = fz;
  const double r = ((g.n[0] * x + g.n[1] * y) + g.n[2] * z) - g.dist;
  return refit_gate_open(g.gate) && __builtin_fabs(r) <= g.gate;
}

/* k_surface_refit after a whole run of the chain on the same workspace (k_surface_refit_cams after a whole cameras batch, under the table
 * and that workspace's index: DESIGN.md section 7h): launch_surface_moments' arguments, and gates[i] = frame i's (device memory); frame i's
 * record at out + i, zeroed by the caller on the stream in front of the launch */
struct Batch;                                 /* ssd_launch.h */
void launch_surface_refit(const Batch &B, int chunkPoints, const ssd_frame_gates *gates, ssd_frame_moments *out);

} // namespace ssd

#endif /* SSD_REFIT_H_ */
