/*
 * ssd_edges.h — the depth edge filter's per-pixel rule (include/ssd_hip.h), stated once for the device
 * (k_depth_edges, ssd_k_edges.h) and the host (ssd_depth_edges_host, ssd_host.cpp), and the kernel's launcher.  Integers only: both
 * sides agree byte for byte.  A pixel that does not exist (outside the frame) is handed to these functions as the sample 0, which is
 * never near and never one end of a bridge - exactly what the rule says of it.  The kernel counts the near neighbours and finds the
 * bridges of two pixels at a time in packed 16-bit registers; what t, a pixel's class, its output and its share of the frame's record
 * ARE stands here, and the host statement takes the counts from here as well.
 */
#ifndef SSD_EDGES_H_
#define SSD_EDGES_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ssd_hip.h"

namespace ssd
{

constexpr int kEdgeWords = 8;               /* ssd_depth_edge_stats as int64 words, in its order; the last three stay 0 */
constexpr int kEdgeSumSupport = 4;          /* words 0 .. 3 are the classes' counts, indexed by SSD_EDGE_KEPT .. SSD_EDGE_BRIDGE */

__host__ __device__ inline bool edge_rule_ok(const ssd_depth_edge_rule &r)
{
  return r.min_support >= 0 && r.min_support <= 8 && r.tol >= 0 && r.tol <= 65535 && r.slope >= 0 && r.slope <= 4096;
}

/* t(d): d * slope <= 65535 * 4096 < 2^28; the sum saturates at 65535, so t fits a 16-bit half */
__host__ __device__ inline uint32_t edge_t(uint32_t d, const ssd_depth_edge_rule &r)
{
  const uint32_t t = static_cast<uint32_t>(r.tol) + ((d * static_cast<uint32_t>(r.slope)) >> 12);
  return t < 65535u ? t : 65535u;
}

/* whether the neighbour q (0: invalid or outside the frame) is near the sample d */
__host__ __device__ inline bool edge_near(uint32_t q, uint32_t d, uint32_t t) { return q != 0u && (q > d ? q - d : d - q) <= t; }

/* whether d lies between the opposite neighbours a and b, more than t from either (0: invalid or outside the frame: no bridge) */
__host__ __device__ inline bool edge_bridged(uint32_t a, uint32_t b, uint32_t d, uint32_t t)
{
  return a != 0u && b != 0u && ((a + t < d && d + t < b) || (b + t < d && d + t < a));
}

/* the class of the sample d with c near neighbours, in the order the rule tests them */
__host__ __device__ inline int edge_class(uint32_t d, uint32_t c, bool bridged, const ssd_depth_edge_rule &r)
{
  if(d == 0u)
    return SSD_EDGE_EMPTY;
  if(c < static_cast<uint32_t>(r.min_support))
    return SSD_EDGE_LONE;
  if(r.bridge != 0 && bridged)
    return SSD_EDGE_BRIDGE;
  return SSD_EDGE_KEPT;
}

/* one pixel from its eight neighbours in reading order (NW N NE W E SW S SE; 0 where there is none): the class, and c in *support */
__host__ __device__ inline int edge_pixel(uint32_t d, const uint32_t (&q)[8], const ssd_depth_edge_rule &r, uint32_t *support)
{
  const uint32_t t = edge_t(d, r);
  uint32_t c = 0u;
  for(int i = 0; i < 8; i++)
    c += edge_near(q[i], d, t) ? 1u : 0u;
  const bool bridged = edge_bridged(q[3], q[4], d, t) || edge_bridged(q[1], q[6], d, t) || edge_bridged(q[0], q[7], d, t) ||
                       edge_bridged(q[2], q[5], d, t);
  *support = c;
  return edge_class(d, c, bridged, r);
}

/* k_depth_edges over nframes frames of W x H uint16 (frame i at frames + i * strideBytes, rows packed): filtered frame i at out + i *
 * outStride, its class bytes (cls may be null) at cls + i * clsStride; adds into stats[i], which the caller zeroed on the stream */
void launch_depth_edges(const void *frames, size_t strideBytes, int W, int H, int nframes, const ssd_depth_edge_rule &rule, void *out,
                        size_t outStride, uint8_t *cls, size_t clsStride, ssd_depth_edge_stats *stats, hipStream_t s);

} // namespace ssd

#endif /* SSD_EDGES_H_ */
