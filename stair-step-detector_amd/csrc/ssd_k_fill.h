/*
 * ssd_k_fill.h - k_depth_fill, the depth fill's one kernel (ssd_enqueue_depth_fill).
 * ssd_kernels_ground.hip, the unit of the stand-alone frame passes, includes it behind ssd_k_edges.h and holds its launcher.
 *
 * The edge filter's sibling: the same 3 x 3 stencil over registers, on the row machinery of ssd_k_edges.h, which is called and not
 * restated - a lane's strip of kEdgeStrip pixels, a wave's span, the tile of kEdgeTile rows with three rows in registers, edge_issue /
 * edge_finish / edge_no_row with the loads of row r + 2 issued early, the shuffles for the pixels beside a strip, the WIDE condition and
 * the shape of the record's reduction.  k_depth_edges itself is left as it is, so its code object keeps its bytes; what is written
 * again here is the walk down the tile around this kernel's own pixel function.
 *
 * Two pixels at a time in packed 16-bit halves.  For an opposite pair (a, b): lo and hi by packed min and max; the spread hi - lo cannot
 * wrap; both ends are valid iff lo != 0; the pair agrees iff that and spread -sat t == 0; m = lo + ((spread + 1) >> 1), which can wrap
 * only where lo == 0, a pair that does not agree; the pair covers d iff it agrees and (d -sat hi) -sat t != 0, which is hi + t < d.  The
 * best pair is a running minimum of the spread under a strict less-than in the rule's order, "no pair" standing as the spread 65535,
 * which no agreeing pair has (lo >= 1).  At slope 0 t is one value for the launch and that path is taken wave-uniformly; otherwise t
 * comes per half from edge_t at lo.  The class, the output and the record's shares come from ssd_fill.h per pixel.  A lane keeps six
 * sums; they are reduced across the wave (shuffles), across the block's waves (dynamic LDS, 256 bytes) and go out as one 64-bit add per
 * block and non-zero word.
 */
#ifndef SSD_K_FILL_H_
#define SSD_K_FILL_H_

#include "ssd_fill.h"
#include "ssd_k_edges.h"

namespace ssd
{

constexpr int kFillLds = kEdgeWaves * kFillWords * 8;                /* 256 bytes: a multiple of 16 */

struct FillArgs
{
  const unsigned char *frames;
  size_t strideBytes;
  unsigned char *out;
  size_t outStride;
  unsigned char *cls;                        /* null: none */
  size_t clsStride;
  unsigned long long *stats;                 /* kFillWords per frame */
  int W, H, nframes, spans, tasks, blocksPerFrame;
  ssd_depth_fill_rule rule;
};

/* a lane's share of its frame's record */
struct FillSums
{
  unsigned int cls[4];
  unsigned int pairs, spread;
};

/* the running best of one kind of pair for two pixels: their count, the smallest spread so far and its m */
struct FillBest2
{
  edge_u16x2 n, spread, m;
};

/* one opposite pair (a, b), each two packed pixels, of the pixel pair d onto the agreeing pairs and the covering ones.  FLAT: t is
 * tFlat for every pixel (slope 0) */
template<bool FLAT>
__device__ __forceinline__ void fill_pair2(unsigned int a, unsigned int b, edge_u16x2 d, edge_u16x2 tFlat, const ssd_depth_edge_rule &e,
                                           FillBest2 &agree, FillBest2 &cover)
{
  const edge_u16x2 one = { 1, 1 }, zero = { 0, 0 };
  const edge_u16x2 aa = edge_pack(a), bb = edge_pack(b);
  const edge_u16x2 lo = __builtin_elementwise_min(aa, bb), hi = __builtin_elementwise_max(aa, bb);
  const edge_u16x2 spread = hi - lo;
  edge_u16x2 t = tFlat;
  if(!FLAT)
  {
    const unsigned int l = edge_bits(lo);
    t = edge_pack(edge_t(l & 0xffffu, e) | (edge_t(l >> 16, e) << 16));
  }
  const edge_u16x2 agrees = __builtin_elementwise_min(lo, one) & (one ^ __builtin_elementwise_min(__builtin_elementwise_sub_sat(spread, t), one));
  const edge_u16x2 covers = agrees & __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_elementwise_sub_sat(d, hi), t), one);
  const edge_u16x2 m = lo + ((spread + one) >> one);
  /* the spread where the pair counts, 65535 where it does not; better: all ones where it is below the best so far */
  const edge_u16x2 keyA = spread | (agrees - one), keyC = spread | (covers - one);
  const edge_u16x2 betterA = zero - __builtin_elementwise_min(__builtin_elementwise_sub_sat(agree.spread, keyA), one);
  const edge_u16x2 betterC = zero - __builtin_elementwise_min(__builtin_elementwise_sub_sat(cover.spread, keyC), one);
  agree.n += agrees;
  agree.m = (m & betterA) | (agree.m & ~betterA);
  agree.spread = __builtin_elementwise_min(agree.spread, keyA);
  cover.n += covers;
  cover.m = (m & betterC) | (cover.m & ~betterC);
  cover.spread = __builtin_elementwise_min(cover.spread, keyC);
}

/* the pixel pair k (1 .. 4) of the current row C between the rows P above and N below -> the two outputs packed as the samples are,
 * their classes in the low two bytes of *cls2.  live: bit 0 / 1 - the lower / upper pixel exists */
template<bool FLAT>
__device__ __forceinline__ unsigned int fill_pair_of_pixels(const EdgeRow &P, const EdgeRow &C, const EdgeRow &N, int k, unsigned int live,
                                                            const ssd_depth_fill_rule &rule, const ssd_depth_edge_rule &e, edge_u16x2 tFlat,
                                                            unsigned int *cls2, FillSums &S)
{
  const unsigned int dd = C.e[k];
  const edge_u16x2 d = edge_pack(dd);
  const edge_u16x2 none = { static_cast<unsigned short>(kFillNoPair), static_cast<unsigned short>(kFillNoPair) }, zero = { 0, 0 };
  FillBest2 agree = { zero, none, zero }, cover = { zero, none, zero };
  fill_pair2<FLAT>(edge_shift(C.e[k], C.e[k - 1]), edge_shift(C.e[k + 1], C.e[k]), d, tFlat, e, agree, cover);        /* W / E */
  fill_pair2<FLAT>(P.e[k], N.e[k], d, tFlat, e, agree, cover);                                                        /* N / S */
  fill_pair2<FLAT>(edge_shift(P.e[k], P.e[k - 1]), edge_shift(N.e[k + 1], N.e[k]), d, tFlat, e, agree, cover);        /* NW / SE */
  fill_pair2<FLAT>(edge_shift(P.e[k + 1], P.e[k]), edge_shift(N.e[k], N.e[k - 1]), d, tFlat, e, agree, cover);        /* NE / SW */
  const unsigned int na = edge_bits(agree.n), nc = edge_bits(cover.n), ma = edge_bits(agree.m), mc = edge_bits(cover.m);
  const unsigned int sa = edge_bits(agree.spread), sc = edge_bits(cover.spread);
  unsigned int o[2];
  int kk[2];
#pragma unroll
  for(int j = 0; j < 2; j++)
  {
    const int sh = 16 * j;
    const unsigned int dj = (dd >> sh) & 0xffffu, naj = (na >> sh) & 0xffffu, ncj = (nc >> sh) & 0xffffu;
    kk[j] = fill_class(dj, naj, ncj, rule);
    o[j] = fill_output(kk[j], dj, (ma >> sh) & 0xffffu, (mc >> sh) & 0xffffu);
    const bool lives = (live & (1u << j)) != 0u;                    /* a pixel that does not exist is EMPTY: it has no pair */
#pragma unroll
    for(int i = 0; i < 4; i++)
      S.cls[i] += lives && kk[j] == i ? 1u : 0u;
    S.pairs += fill_pairs_share(kk[j], naj, ncj);
    S.spread += fill_spread_share(kk[j], (sa >> sh) & 0xffffu, (sc >> sh) & 0xffffu);
  }
  *cls2 = static_cast<unsigned int>(kk[0]) | (static_cast<unsigned int>(kk[1]) << 8);
  return o[0] | (o[1] << 16);
}

/* WIDE: as k_depth_edges - the width is a multiple of 8 and the frames, the output and the class maps lie on 16 (8) byte boundaries */
template<bool WIDE>
__global__ __launch_bounds__(kEdgeThreads) void k_depth_fill(const FillArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char fillLds[];
  const int t = static_cast<int>(threadIdx.x), lane = t & 63;
  const int frame = static_cast<int>(blockIdx.x) / A.blocksPerFrame;
  const int task = (static_cast<int>(blockIdx.x) % A.blocksPerFrame) * kEdgeWaves + (t >> 6);      /* wave-uniform */
  const int W = A.W, H = A.H;
  FillSums S = {};
  if(task < A.tasks)
  {
    const int x0 = (task % A.spans) * kEdgeSpan + lane * kEdgeStrip;
    const int r0 = (task / A.spans) * kEdgeTile, r1 = r0 + kEdgeTile < H ? r0 + kEdgeTile : H;
    const unsigned short *in = reinterpret_cast<const unsigned short *>(A.frames + static_cast<size_t>(frame) * A.strideBytes);
    unsigned short *out = reinterpret_cast<unsigned short *>(A.out + static_cast<size_t>(frame) * A.outStride);
    unsigned char *cls = A.cls ? A.cls + static_cast<size_t>(frame) * A.clsStride : nullptr;
    const ssd_depth_edge_rule e = fill_edge_rule(A.rule);
    const bool flat = A.rule.slope == 0;                                                           /* launch-uniform */
    const unsigned int t0 = edge_t(0u, e);
    const edge_u16x2 tFlat = edge_pack(t0 | (t0 << 16));
    unsigned int live = 0u;
#pragma unroll
    for(int i = 0; i < kEdgeStrip; i++)
      live |= x0 + i < W ? 1u << i : 0u;
    EdgeRow P = r0 > 0 ? edge_finish(edge_issue<WIDE>(in + static_cast<size_t>(r0 - 1) * W, W, x0, lane), lane) : edge_no_row();
    EdgeRow C = edge_finish(edge_issue<WIDE>(in + static_cast<size_t>(r0) * W, W, x0, lane), lane);
    EdgeRow N = r0 + 1 < H ? edge_finish(edge_issue<WIDE>(in + static_cast<size_t>(r0 + 1) * W, W, x0, lane), lane) : edge_no_row();
    for(int r = r0; r < r1; r++)
    {
      /* the row below the next one, wanted unless this is the tile's last row: issued now, shuffled when it is needed */
      const bool more = r + 1 < r1 && r + 2 < H;
      EdgeRaw raw = { make_uint4(0u, 0u, 0u, 0u), 0u };
      if(more)
        raw = edge_issue<WIDE>(in + static_cast<size_t>(r + 2) * W, W, x0, lane);
      unsigned int o[4], kc[4];
      if(flat)
      {
#pragma unroll
        for(int k = 0; k < 4; k++)
          o[k] = fill_pair_of_pixels<true>(P, C, N, k + 1, (live >> (2 * k)) & 3u, A.rule, e, tFlat, &kc[k], S);
      }
      else
      {
#pragma unroll
        for(int k = 0; k < 4; k++)
          o[k] = fill_pair_of_pixels<false>(P, C, N, k + 1, (live >> (2 * k)) & 3u, A.rule, e, tFlat, &kc[k], S);
      }
      const size_t at = static_cast<size_t>(r) * W + x0;
      if(WIDE)
      {
        if(x0 < W)
        {
          *reinterpret_cast<uint4 *>(out + at) = make_uint4(o[0], o[1], o[2], o[3]);
          if(cls)
            *reinterpret_cast<uint2 *>(cls + at) = make_uint2(kc[0] | (kc[1] << 16), kc[2] | (kc[3] << 16));
        }
      }
      else
      {
#pragma unroll
        for(int i = 0; i < kEdgeStrip; i++)
          if(x0 + i < W)
          {
            out[at + i] = static_cast<unsigned short>(o[i >> 1] >> (16 * (i & 1)));
            if(cls)
              cls[at + i] = static_cast<unsigned char>(kc[i >> 1] >> (8 * (i & 1)));
          }
      }
      P = C;
      C = N;
      N = more ? edge_finish(raw, lane) : edge_no_row();
    }
  }
  /* the block's sums into the frame's record */
  unsigned long long acc[kFillSumSpread + 1] = { S.cls[0], S.cls[1], S.cls[2], S.cls[3], S.pairs, S.spread };
#pragma unroll
  for(int i = 0; i <= kFillSumSpread; i++)
  {
#pragma unroll
    for(int o = 32; o >= 1; o >>= 1)
      acc[i] += __shfl_xor(acc[i], o);
  }
  unsigned long long *part = reinterpret_cast<unsigned long long *>(fillLds);
  if(lane == 0)
  {
#pragma unroll
    for(int i = 0; i <= kFillSumSpread; i++)
      part[(t >> 6) * kFillWords + i] = acc[i];
  }
  __syncthreads();
  if(t <= kFillSumSpread)
  {
    unsigned long long sum = 0ull;
#pragma unroll
    for(int w = 0; w < kEdgeWaves; w++)
      sum += part[w * kFillWords + t];
    if(sum != 0ull)
      atomicAdd(A.stats + static_cast<size_t>(frame) * kFillWords + t, sum);
  }
}

} // namespace ssd

#endif /* SSD_K_FILL_H_ */
