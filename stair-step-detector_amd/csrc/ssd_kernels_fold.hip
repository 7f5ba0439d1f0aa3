/*
 * ssd_kernels_fold.hip - the camera fold on the device: k_camera_fold (ssd_enqueue_camera_fold), the camera's
 * gate on top of it, k_camera_ground_gates (ssd_enqueue_camera_ground_gates), and their launchers.
 *
 * k_camera_fold is ssd_camera_drift_fold's loop (ssd_fold.h), k_camera_ground_gates is ssd_ground_fit_solve's status and plane
 * (ssd_solve.h) with ssd_camera_ground_gates' overlay.  A translation unit of its own, so that no code object of the chain moves;
 * compiled like them without FMA contraction - the overlay's agreement with the host rests on it, the fold is integers alone.
 */
#include "ssd_launch.h"
#include "ssd_fold.h"
#include "ssd_solve.h"

#include <cstddef>

namespace ssd
{

static_assert(sizeof(ssd_camera_fold) == 104, "ssd_camera_fold: four int32, the ten sums, n_far");
static_assert(offsetof(ssd_camera_fold, camera) == offsetof(ssd_camera_drift, camera) && offsetof(ssd_camera_fold, frames) == offsetof(ssd_camera_drift, frames) &&
              offsetof(ssd_camera_fold, frames_ground) == offsetof(ssd_camera_drift, frames_ground) &&
              offsetof(ssd_camera_fold, frames_left) == offsetof(ssd_camera_drift, frames_left) && offsetof(ssd_camera_fold, m) == offsetof(ssd_camera_drift, m) &&
              offsetof(ssd_camera_fold, n_far) == offsetof(ssd_camera_drift, n_far) && offsetof(ssd_camera_drift, fit) == sizeof(ssd_camera_fold),
              "ssd_camera_fold is the head of ssd_camera_drift, field for field");
static_assert(offsetof(ssd_camera_fold, m) == 16 && offsetof(ssd_frame_moments, s) == 8, "the sums are int64 at 8-byte offsets");

constexpr int kFoldWave = 64;                    /* one wave per camera: a block is a wave */

/* |x| as an unsigned number (|-2^63| = 2^63) and a sum that stops at 2^64 - 1 */
__device__ inline unsigned long long fold_mag(long long x) { return x < 0 ? 0ull - static_cast<unsigned long long>(x) : static_cast<unsigned long long>(x); }
__device__ inline unsigned long long fold_sat(unsigned long long a, unsigned long long b) { return a + b < a ? ~0ull : a + b; }

/* Wave c folds the frames that name camera c, a chunk of 64 frames at a time, lane l with frame base + l.  The record stays in every
 * lane's registers, the same in all of them.
 *   The fast path: the lanes with a frame to fold (it names c and has a ground) load its eleven integers, the others hold zeros; each
 * column is added across the wave, wrapping, and beside it the column's magnitudes, saturating.  Where |have| + sum |add| stays inside
 * int64 for every column, no prefix of the chunk can leave it in any order: every frame fits, and the wrapped sums are the exact ones -
 * what the host's loop arrives at.
 *   Otherwise every lane walks the chunk in index order by the host's own step (the same addresses in all lanes: one request each).
 * No atomics, no LDS. */
__global__ __launch_bounds__(kFoldWave) void k_camera_fold(const ssd_frame_moments *__restrict__ rec, const int *__restrict__ camOf, int nframes, int ncams,
                                                          int accumulate, ssd_camera_fold *out)
{
  const int c = blockIdx.x, lane = threadIdx.x;
  if(c >= ncams)
    return;
  ssd_camera_fold d;
  d.camera = c;
  d.frames = 0; d.frames_ground = 0; d.frames_left = 0;
  int64_t have[kFoldSums];
#pragma unroll
  for(int k = 0; k < kFoldSums; k++)
    have[k] = 0;
  if(accumulate)
  {
    const ssd_camera_fold &was = out[c];
    d.frames = was.frames; d.frames_ground = was.frames_ground; d.frames_left = was.frames_left;
    fold_get(was, have);
  }
  fold_put(d, have);
  for(int base = 0; base < nframes; base += kFoldWave)
  {
    const int i = base + lane;
    const bool mine = i < nframes && camOf[i] == c;
    bool fold = false;
    if(mine)
      fold = rec[i].ground == 1 && rec[i].n_surfaces >= 1;
    const unsigned long long named = __ballot(mine), folded = __ballot(fold);
    if(named == 0)
      continue;
    if(folded == 0)
    {
      d.frames += __popcll(named);
      continue;
    }
    long long add[kFoldSums];
    const long long *src = reinterpret_cast<const long long *>(&rec[fold ? i : 0].s[0]);
#pragma unroll
    for(int k = 0; k < kFoldSums; k++)
      add[k] = fold ? src[k] : 0ll;
    fold_get(d, have);
    bool fast = true;
    long long sum[kFoldSums];
#pragma unroll
    for(int k = 0; k < kFoldSums; k++)
    {
      unsigned long long s = static_cast<unsigned long long>(add[k]), m = fold_mag(add[k]);
#pragma unroll
      for(int w = 1; w < kFoldWave; w <<= 1)
      {
        s += __shfl_xor(s, w, kFoldWave);
        m = fold_sat(m, __shfl_xor(m, w, kFoldWave));
      }
      if(fold_sat(fold_mag(have[k]), m) > 0x7fffffffffffffffull)
        fast = false;
      sum[k] = static_cast<long long>(static_cast<unsigned long long>(have[k]) + s);
    }
    if(fast)
    {
      int64_t take[kFoldSums];
#pragma unroll
      for(int k = 0; k < kFoldSums; k++)
        take[k] = sum[k];
      fold_put(d, take);
      d.frames += __popcll(named);
      d.frames_ground += __popcll(folded);
      continue;
    }
    const int end = nframes - base < kFoldWave ? nframes - base : kFoldWave;
    for(int j = 0; j < end; j++)
      if((named >> j) & 1ull)
        fold_step(d, rec[base + j]);
  }
  if(lane == 0)
    out[c] = d;
}

/* Lane i overlays frame i's ground gate with its camera's plane: ssd_camera_ground_gates, with drift[c].fit's status, normal, dist and
 * rms solved here from fold[c].m as ssd_ground_fit_solve orders them - plane_of_moments, then DEGENERATE when
 * camera_to_world_from_plane fails (its matrix is not kept).  Every lane solves its own camera's sum: the lanes of a camera repeat each
 * other, and a batch needs no second kernel and no buffer between the two.  A frame without a ground, of a camera that is not OK, or
 * whose index lies outside the table is left as given, byte for byte. */
__global__ __launch_bounds__(kFoldWave) void k_camera_ground_gates(const ssd_frame_moments *__restrict__ rec, const int *__restrict__ camOf, int nframes,
                                                                  const ssd_camera_fold *__restrict__ fold, int ncams, int min_points, double k_sigma,
                                                                  double gate_min, ssd_frame_gates *gates)
{
  const int i = blockIdx.x * kFoldWave + threadIdx.x;
  if(i >= nframes)
    return;
  const int c = camOf[i];
  if(c < 0 || c >= ncams)
    return;
  if(rec[i].ground != 1 || rec[i].n_surfaces < 1)
    return;
  const ssd_ground_moments m = fold[c].m;
  PlaneOfMoments pl;
  if(plane_of_moments(&m, min_points, pl) != SSD_GF_OK)
    return;
  double a[9], b[3];
  if(!camera_to_world_from_plane(pl.n0[0], pl.n0[1], pl.n0[2], pl.dist, a, b))
    return;
  const double rms = sqrt(pl.lambda[0] > 0.0 ? pl.lambda[0] : 0.0);
  ssd_frame_gates &G = gates[i];
  ssd_plane_gate g;
  g.n[0] = pl.n0[0]; g.n[1] = pl.n0[1]; g.n[2] = pl.n0[2];
  g.dist = pl.dist;
  const double wide = k_sigma * rms;
  g.gate = wide > gate_min ? wide : gate_min;
  G.g[0] = g;
  if(G.n_surfaces < 1)
    G.n_surfaces = 1;
}

void launch_camera_fold(const ssd_frame_moments *rec, const int *camOf, int nframes, int ncams, bool accumulate, ssd_camera_fold *out, hipStream_t s)
{
  hipLaunchKernelGGL(k_camera_fold, dim3(ncams), dim3(kFoldWave), 0, s, rec, camOf, nframes, ncams, accumulate ? 1 : 0, out);
}

void launch_camera_ground_gates(const ssd_frame_moments *rec, const int *camOf, int nframes, const ssd_camera_fold *fold, int ncams, int min_points,
                                double k_sigma, double gate_min, ssd_frame_gates *gates, hipStream_t s)
{
  hipLaunchKernelGGL(k_camera_ground_gates, dim3((nframes + kFoldWave - 1) / kFoldWave), dim3(kFoldWave), 0, s, rec, camOf, nframes, fold, ncams,
                     min_points, k_sigma, gate_min, gates);
}

} // namespace ssd
