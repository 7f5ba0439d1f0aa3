/*
 * ssd_kernels_solve.hip - k_surface_gates: the trimmed refit's gates made on the device (ssd_enqueue_surface_gates and the
 * *_refit_device entry points), and its launcher.
 *
 * The kernel is the host function's loop over ssd_solve.h, one lane per surface: frame i's ssd_frame_gates is byte for byte
 * ssd_surface_gates_from_moments(&rec[i], min_points, k_sigma, gate_min, ..).  A translation unit of its own, so that no code object of
 * the chain moves; compiled like them without FMA contraction - the agreement with the host rests on it.
 */
#include "ssd_launch.h"
#include "ssd_solve.h"

namespace ssd
{

static_assert(sizeof(ssd_plane_gate) == 40 && sizeof(ssd_frame_gates) == 8 + SSD_MAX_STEPS * sizeof(ssd_plane_gate), "ssd_frame_gates: a header of two int32, then five doubles per surface");
static_assert(sizeof(ssd_frame_moments) == 8 + SSD_MAX_STEPS * sizeof(ssd_surface_moments), "ssd_frame_moments: a header of two int32, then eleven int64 per surface");

constexpr int kGateLanes = 32;                   /* lanes per frame: two frames per wave */
constexpr int kGateThreads = 256;
constexpr int kGateFrames = kGateThreads / kGateLanes;      /* frames per block */
static_assert(SSD_MAX_STEPS < kGateLanes, "a lane per surface and one for the header");

/* Lane k < SSD_MAX_STEPS of a frame's 32 solves surface k and writes its gate - the solved one, or zeros at k >= n_surfaces (whose
 * moments are never read) and for FEW / DEGENERATE -, lane SSD_MAX_STEPS writes the header: all 688 bytes of the record, whatever was
 * there.  A record whose n_surfaces lies outside 0 .. SSD_MAX_STEPS (the host function refuses it) gives the all-zero record.  Lanes
 * leave the Jacobi loop at different sweeps; nothing wave-wide happens inside it. */
__global__ __launch_bounds__(kGateThreads) void k_surface_gates(const ssd_frame_moments *__restrict__ rec, int nframes, int min_points, double k_sigma,
                                                               double gate_min, ssd_frame_gates *__restrict__ out)
{
  const int k = threadIdx.x & (kGateLanes - 1);
  const int frame = blockIdx.x * kGateFrames + (threadIdx.x / kGateLanes);
  if(frame >= nframes || k > SSD_MAX_STEPS)
    return;
  const ssd_frame_moments &m = rec[frame];
  int n = m.n_surfaces;
  if(n < 0 || n > SSD_MAX_STEPS)
    n = 0;
  ssd_frame_gates &G = out[frame];
  if(k == SSD_MAX_STEPS)
  {
    G.n_surfaces = n;
    G.reserved = 0;
    return;
  }
  ssd_plane_gate g;
  g.n[0] = 0.0; g.n[1] = 0.0; g.n[2] = 0.0;
  g.dist = 0.0;
  g.gate = 0.0;
  if(k < n)
    g = gate_of_moments(&m.s[k].m, min_points, k_sigma, gate_min);
  G.g[k] = g;
}

void launch_surface_gates(const ssd_frame_moments *rec, int nframes, int min_points, double k_sigma, double gate_min, ssd_frame_gates *out, hipStream_t s)
{
  hipLaunchKernelGGL(k_surface_gates, dim3((nframes + kGateFrames - 1) / kGateFrames), dim3(kGateThreads), 0, s, rec, nframes, min_points, k_sigma,
                     gate_min, out);
}

} // namespace ssd
