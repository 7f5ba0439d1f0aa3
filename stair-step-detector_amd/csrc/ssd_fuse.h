/*
 * ssd_fuse.h — the depth fusion's per-pixel rule (include/ssd_hip.h), stated once for the device (k_depth_fuse,
 * ssd_k_fuse.h) and the host (ssd_depth_fuse_host, ssd_host.cpp), and the kernel's launcher.  Integers only, no floating point
 * anywhere: both sides agree byte for byte.  The kernel finds the median with a sorting network over packed registers and the host with
 * a small sort; what a sample's agreement, a pixel's class, its output and its share of the group's record ARE stands here.
 */
#ifndef SSD_FUSE_H_
#define SSD_FUSE_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ssd_hip.h"

namespace ssd
{

constexpr int kFuseWords = 8;               /* ssd_depth_fuse_stats as int64 words, in its order; the last one stays 0 */
enum { kFuseNFused = 0, kFuseNEmpty, kFuseNFew, kFuseNSplit, kFuseSumValid, kFuseSumAgree, kFuseSumAbsDev };

__host__ __device__ inline bool fuse_rule_ok(int n, const ssd_depth_fuse_rule &r)
{
  return n >= 1 && n <= SSD_FUSE_MAX_FRAMES && r.min_valid >= 1 && r.min_valid <= n && r.min_agree >= 1 && r.min_agree <= n &&
         r.tol >= 0 && r.tol <= 65535;
}

/* step 2: which of the m valid samples, counted from 0 in ascending order, is the lower median (m >= 1) */
__host__ __device__ inline int fuse_median_index(int m) { return (m - 1) / 2; }

/* step 3: |a - b| of two samples as 32-bit values, which cannot wrap */
__host__ __device__ inline uint32_t fuse_dev(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

/* ... and whether sample d agrees with the median: from the sample's own validity, never from what the sort made of it */
__host__ __device__ inline bool fuse_agrees(uint32_t d, uint32_t med, uint32_t tol) { return d != 0u && fuse_dev(d, med) <= tol; }

/* steps 1, 4 and 5 behind the counts: m valid samples, c of them agreeing with sum s (c >= 1 where m >= 1).  The output, and the class
 * as the index of its count in the record */
__host__ __device__ inline uint32_t fuse_output(uint32_t m, uint32_t c, uint32_t s, const ssd_depth_fuse_rule &r, int &cls)
{
  if(m == 0u)
  {
    cls = kFuseNEmpty;
    return 0u;
  }
  if(m < static_cast<uint32_t>(r.min_valid))
  {
    cls = kFuseNFew;
    return 0u;
  }
  if(c < static_cast<uint32_t>(r.min_agree))
  {
    cls = kFuseNSplit;
    return 0u;
  }
  cls = kFuseNFused;
  return (2u * s + c) / (2u * c);           /* s <= 16 * 65535: 32 bits hold it */
}

/* k_depth_fuse over ngroups groups of n frames (group g: frames g * hop .. g * hop + n - 1 at strideBytes apart, nPoints uint16 each):
 * fused frame g at out + g * outStride, its support bytes (support may be null) at support + g * supStride; adds into stats[g], which
 * the caller zeroed on the stream.  groupFastest: neighbouring blocks take the same chunk of neighbouring groups, else neighbouring
 * chunks of one group */
void launch_depth_fuse(const void *frames, size_t strideBytes, int nPoints, int n, int hop, int ngroups, const ssd_depth_fuse_rule &rule,
                       void *out, size_t outStride, uint8_t *support, size_t supStride, ssd_depth_fuse_stats *stats, bool groupFastest,
                       hipStream_t s);

} // namespace ssd

#endif /* SSD_FUSE_H_ */
