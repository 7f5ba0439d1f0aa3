/*
 * ssd_fold.h — the step of the camera fold (DESIGN.md sections 7e and 7j): one frame's record onto its camera's record.  Stated once
 * for the host (ssd_camera_drift_fold: ssd_host.cpp) and the device (k_camera_fold: ssd_kernels_fold.hip).  Integers only, so the two
 * sides agree by construction; what has to be kept is the order - frames in index order - and the rule "whole or not at all".
 */
#ifndef SSD_FOLD_H_
#define SSD_FOLD_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ssd_hip.h"

namespace ssd
{

constexpr int kFoldSums = static_cast<int>(sizeof(ssd_surface_moments) / sizeof(int64_t));     /* the ten sums of m, then n_far */
static_assert(sizeof(ssd_surface_moments) == sizeof(int64_t) * kFoldSums && sizeof(ssd_ground_moments) == sizeof(int64_t) * (kFoldSums - 1) &&
              offsetof(ssd_surface_moments, n_far) == sizeof(ssd_ground_moments),
              "ssd_surface_moments is the ten sums and n_far, contiguous");

/* the record's sums as kFoldSums integers, and back (Rec: ssd_camera_drift or ssd_camera_fold - the same head) */
template<typename Rec>
__host__ __device__ inline void fold_get(const Rec &d, int64_t have[kFoldSums])
{
  have[0] = d.m.n;
#pragma unroll
  for(int k = 0; k < 3; k++)
    have[1 + k] = d.m.s[k];
#pragma unroll
  for(int k = 0; k < 6; k++)
    have[4 + k] = d.m.ss[k];
  have[kFoldSums - 1] = d.n_far;
}

template<typename Rec>
__host__ __device__ inline void fold_put(Rec &d, const int64_t sum[kFoldSums])
{
  d.m.n = sum[0];
#pragma unroll
  for(int k = 0; k < 3; k++)
    d.m.s[k] = sum[1 + k];
#pragma unroll
  for(int k = 0; k < 6; k++)
    d.m.ss[k] = sum[4 + k];
  d.n_far = sum[kFoldSums - 1];
}

/* Frame `fm`, which names d's camera, onto d.  The frame counts in `frames`; it is folded only with a ground (ground == 1 and
 * n_surfaces >= 1: its s[0] is then the ground's, and nothing else of fm.s is read); every sum is tried before any is taken, so a frame
 * goes in whole (frames_ground) or not at all (frames_left: a later, smaller frame may still fit). */
template<typename Rec>
__host__ __device__ inline void fold_step(Rec &d, const ssd_frame_moments &fm)
{
  d.frames++;
  if(fm.ground != 1 || fm.n_surfaces < 1)
    return;
  int64_t have[kFoldSums], sum[kFoldSums];
  fold_get(d, have);
  const int64_t *add = reinterpret_cast<const int64_t *>(&fm.s[0]);
  bool fits = true;
#pragma unroll
  for(int k = 0; k < kFoldSums; k++)
    if(__builtin_add_overflow(have[k], add[k], &sum[k]))
      fits = false;
  if(!fits)
  {
    d.frames_left++;
    return;
  }
  fold_put(d, sum);
  d.frames_ground++;
}

} // namespace ssd

#endif /* SSD_FOLD_H_ */
