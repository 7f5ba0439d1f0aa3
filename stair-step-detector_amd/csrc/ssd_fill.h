/*
 * ssd_fill.h — the depth fill's per-pixel rule (include/ssd_hip.h), stated once for the device (k_depth_fill,
 * ssd_k_fill.h) and the host (ssd_depth_fill_host, ssd_host.cpp), and the kernel's launcher.  Integers only: both sides agree byte for
 * byte.  A pixel that does not exist (outside the frame) is handed to these functions as the sample 0, which is never one end of an
 * agreeing pair - exactly what the rule says of it.  The kernel finds the agreeing and the covering pairs of two pixels at a time in
 * packed 16-bit registers; what t, a pixel's class, its output and its share of the frame's record ARE stands here, and the host
 * statement takes the pairs from here as well.  t is the edge filter's (edge_t, ssd_edges.h), taken at the pair's lower sample.
 */
#ifndef SSD_FILL_H_
#define SSD_FILL_H_

#include "ssd_edges.h"

namespace ssd
{

constexpr int kFillWords = 8;               /* ssd_depth_fill_stats as int64 words, in its order; the last two stay 0 */
constexpr int kFillSumPairs = 4;            /* words 0 .. 3 are the classes' counts, indexed by SSD_FILL_KEPT .. SSD_FILL_COVERED */
constexpr int kFillSumSpread = 5;
constexpr uint32_t kFillNoPair = 65535u;    /* the spread of "no pair yet": a pair that agrees has lo >= 1, so its spread is at most 65534 */

__host__ __device__ inline bool fill_rule_ok(const ssd_depth_fill_rule &r)
{
  return r.min_pairs >= 1 && r.min_pairs <= 4 && r.cover >= 0 && r.cover <= 4 && r.tol >= 0 && r.tol <= 65535 && r.slope >= 0 && r.slope <= 4096;
}

/* the edge filter's rule that carries this rule's tol and slope: what edge_t reads */
__host__ __device__ inline ssd_depth_edge_rule fill_edge_rule(const ssd_depth_fill_rule &r)
{
  ssd_depth_edge_rule e;
  e.min_support = 0;
  e.bridge = 0;
  e.tol = r.tol;
  e.slope = r.slope;
  return e;
}

/* the pairs of one kind (agreeing, or covering) seen so far, and the best of them: the smallest spread, the first one on a tie */
struct FillBest
{
  uint32_t n, spread, m;
};

__host__ __device__ inline FillBest fill_none()
{
  const FillBest b = { 0u, kFillNoPair, 0u };
  return b;
}

/* one opposite pair (a, b) of the pixel with sample d (0: invalid or outside the frame), in the rule's order: onto the agreeing pairs,
 * and onto the covering ones.  hi + t < d in 32 bits: at most 2 * 65535 */
__host__ __device__ inline void fill_pair(uint32_t a, uint32_t b, uint32_t d, const ssd_depth_edge_rule &e, FillBest &agree, FillBest &cover)
{
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a, spread = hi - lo;
  const uint32_t t = edge_t(lo, e);
  if(lo == 0u || spread > t)
    return;
  const uint32_t m = lo + ((spread + 1u) >> 1);                  /* = (a + b + 1) >> 1; lies in lo .. hi */
  agree.n++;
  if(spread < agree.spread)
  {
    agree.spread = spread;
    agree.m = m;
  }
  if(hi + t < d)
  {
    cover.n++;
    if(spread < cover.spread)
    {
      cover.spread = spread;
      cover.m = m;
    }
  }
}

/* the class of the sample d with na agreeing and nc covering pairs, in the order the rule tests them */
__host__ __device__ inline int fill_class(uint32_t d, uint32_t na, uint32_t nc, const ssd_depth_fill_rule &r)
{
  if(d == 0u)
    return na < static_cast<uint32_t>(r.min_pairs) ? SSD_FILL_EMPTY : SSD_FILL_FILLED;
  if(r.cover != 0 && nc >= static_cast<uint32_t>(r.cover))
    return SSD_FILL_COVERED;
  return SSD_FILL_KEPT;
}

/* what a pixel of class k puts out: mAgree / mCover - the m of its best agreeing / covering pair */
__host__ __device__ inline uint32_t fill_output(int k, uint32_t d, uint32_t mAgree, uint32_t mCover)
{
  return k == SSD_FILL_FILLED ? mAgree : k == SSD_FILL_COVERED ? mCover : k == SSD_FILL_EMPTY ? 0u : d;
}

/* a pixel's share of sum_pairs and of sum_spread: the pairs that made it FILLED or COVERED, and the spread of the one whose m it took */
__host__ __device__ inline uint32_t fill_pairs_share(int k, uint32_t na, uint32_t nc)
{
  return k == SSD_FILL_FILLED ? na : k == SSD_FILL_COVERED ? nc : 0u;
}

__host__ __device__ inline uint32_t fill_spread_share(int k, uint32_t spreadAgree, uint32_t spreadCover)
{
  return k == SSD_FILL_FILLED ? spreadAgree : k == SSD_FILL_COVERED ? spreadCover : 0u;
}

/* one pixel from its eight neighbours in reading order (NW N NE W E SW S SE; 0 where there is none): the class; its output, its pairs
 * and the spread it used in *out, *pairs, *spread */
__host__ __device__ inline int fill_pixel(uint32_t d, const uint32_t (&q)[8], const ssd_depth_fill_rule &r, uint32_t *out, uint32_t *pairs,
                                          uint32_t *spread)
{
  const ssd_depth_edge_rule e = fill_edge_rule(r);
  FillBest agree = fill_none(), cover = fill_none();
  fill_pair(q[3], q[4], d, e, agree, cover);                      /* W / E */
  fill_pair(q[1], q[6], d, e, agree, cover);                      /* N / S */
  fill_pair(q[0], q[7], d, e, agree, cover);                      /* NW / SE */
  fill_pair(q[2], q[5], d, e, agree, cover);                      /* NE / SW */
  const int k = fill_class(d, agree.n, cover.n, r);
  *out = fill_output(k, d, agree.m, cover.m);
  *pairs = fill_pairs_share(k, agree.n, cover.n);
  *spread = fill_spread_share(k, agree.spread, cover.spread);
  return k;
}

/* k_depth_fill over nframes frames of W x H uint16 (frame i at frames + i * strideBytes, rows packed): filled frame i at out + i *
 * outStride, its class bytes (cls may be null) at cls + i * clsStride; adds into stats[i], which the caller zeroed on the stream */
void launch_depth_fill(const void *frames, size_t strideBytes, int W, int H, int nframes, const ssd_depth_fill_rule &rule, void *out,
                       size_t outStride, uint8_t *cls, size_t clsStride, ssd_depth_fill_stats *stats, hipStream_t s);

} // namespace ssd

#endif /* SSD_FILL_H_ */
