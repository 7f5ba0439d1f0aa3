/*
 * ssd_k_edges.h - k_depth_edges, the depth edge filter's one kernel (ssd_enqueue_depth_edges).
 * ssd_kernels_ground.hip, the unit of the stand-alone frame passes, includes it and holds its launcher.
 *
 * A 3 x 3 stencil over registers.  A lane owns a strip of kEdgeStrip = 8 neighbouring pixels of a row (four registers of two packed
 * samples), a wave a span of 64 strips = 512 pixels, and a wave walks down a tile of kEdgeTile rows with the previous, the current and
 * the next row in registers: a row comes from memory once per tile, plus the two halo rows above and below it.  A block's four waves
 * take four neighbouring tasks (the spans of a row tile first), so they sit side by side in one row tile where the frame is 2048 pixels
 * wide or wider.  The pixel left of a strip and the pixel right of it come from the neighbouring lanes by a wave shuffle; lanes 0 and 63
 * load theirs from memory, the index clamped into the row and the value killed where the pixel does not exist.  A row that does not
 * exist is a row of zeros and is never loaded: 0 is an invalid sample, which is never near and never the end of a bridge, so nothing
 * outside the frame takes part, as the rule says.  The loads of row r + 2 are issued before row r is worked on; their shuffles wait
 * until the row is needed.
 *
 * Two pixels at a time in packed 16-bit halves: with s1 = d -sat q and s2 = q -sat d (saturating at 0, so neither wraps), q is more
 * than t below d iff s1 -sat t != 0 and more than t above iff s2 -sat t != 0; near is neither of them with q != 0, a bridge is a valid
 * pixel below on one side and a pixel above on the opposite one.  t (ssd_edges.h) saturates at 65535 and fits its half.  The class,
 * the output and the record come from ssd_edges.h per pixel.  A lane keeps five sums; they are reduced across the wave (shuffles),
 * across the block's waves (dynamic LDS, 256 bytes) and go out as one 64-bit add per block and non-zero word.
 */
#ifndef SSD_K_EDGES_H_
#define SSD_K_EDGES_H_

#include "ssd_edges.h"

namespace ssd
{

constexpr int kEdgeThreads = 256;
constexpr int kEdgeWaves = kEdgeThreads / 64;
constexpr int kEdgeStrip = 8;                                        /* pixels of a lane per row */
constexpr int kEdgeSpan = 64 * kEdgeStrip;                           /* pixels of a wave per row */
constexpr int kEdgeTile = 32;                                        /* rows a wave walks down */
constexpr int kEdgeLds = kEdgeWaves * kEdgeWords * 8;                /* 256 bytes: a multiple of 16 */

typedef unsigned short edge_u16x2 __attribute__((ext_vector_type(2)));

struct EdgeArgs
{
  const unsigned char *frames;
  size_t strideBytes;
  unsigned char *out;
  size_t outStride;
  unsigned char *cls;                        /* null: none */
  size_t clsStride;
  unsigned long long *stats;                 /* kEdgeWords per frame */
  int W, H, nframes, spans, tasks, blocksPerFrame;
  ssd_depth_edge_rule rule;
};

/* a row's loads in flight: the strip, and for lanes 0 and 63 the pixel beside the wave's span */
struct EdgeRaw
{
  uint4 v;
  unsigned int beside;
};

/* a row ready for the stencil: e[1 .. 4] the strip, e[0]'s high half the pixel left of it, e[5]'s low half the pixel right of it */
struct EdgeRow
{
  unsigned int e[6];
};

__device__ __forceinline__ edge_u16x2 edge_pack(unsigned int v) { return __builtin_bit_cast(edge_u16x2, v); }
__device__ __forceinline__ unsigned int edge_bits(edge_u16x2 v) { return __builtin_bit_cast(unsigned int, v); }
/* the pair of pixels one to the left of hi's pair: lo's upper pixel and hi's lower one */
__device__ __forceinline__ unsigned int edge_shift(unsigned int hi, unsigned int lo) { return (lo >> 16) | (hi << 16); }

/* row y of a frame (row: its first sample, y inside the frame - wave-uniform).  x0: the lane's first column */
template<bool WIDE>
__device__ __forceinline__ EdgeRaw edge_issue(const unsigned short *row, int W, int x0, int lane)
{
  EdgeRaw R;
  if(WIDE)
  {
    const int xs = x0 < W ? x0 : W - kEdgeStrip;                       /* W is a multiple of 8 here: the load stays inside the row */
    R.v = *reinterpret_cast<const uint4 *>(row + xs);
    if(x0 >= W)
      R.v = make_uint4(0u, 0u, 0u, 0u);
  }
  else
  {
    unsigned int p[kEdgeStrip];
#pragma unroll
    for(int e = 0; e < kEdgeStrip; e++)
    {
      const int x = x0 + e;
      p[e] = row[x < W ? x : W - 1];                                   /* the load stays inside the row */
      if(x >= W)
        p[e] = 0u;
    }
    R.v = make_uint4(p[0] | (p[1] << 16), p[2] | (p[3] << 16), p[4] | (p[5] << 16), p[6] | (p[7] << 16));
  }
  R.beside = 0u;
  if(lane == 0 || lane == 63)
  {
    const int x = lane == 0 ? x0 - 1 : x0 + kEdgeStrip;
    const int xc = x < 0 ? 0 : x < W ? x : W - 1;
    R.beside = row[xc];
    if(x < 0 || x >= W)
      R.beside = 0u;
  }
  return R;
}

/* the shuffles: every lane of the wave comes here */
__device__ __forceinline__ EdgeRow edge_finish(const EdgeRaw &R, int lane)
{
  EdgeRow r;
  unsigned int left = __shfl_up(R.v.w >> 16, 1), right = __shfl_down(R.v.x & 0xffffu, 1);
  if(lane == 0) left = R.beside;
  if(lane == 63) right = R.beside;
  r.e[0] = left << 16;
  r.e[1] = R.v.x; r.e[2] = R.v.y; r.e[3] = R.v.z; r.e[4] = R.v.w;
  r.e[5] = right;
  return r;
}

__device__ __forceinline__ EdgeRow edge_no_row()
{
  EdgeRow r;
#pragma unroll
  for(int i = 0; i < 6; i++)
    r.e[i] = 0u;
  return r;
}

/* one neighbour pair q of the pixel pair d: adds the near ones to c; low / high: 1 where q is a valid pixel more than t below d /
 * a pixel more than t above d (which is valid: it is above d >= 0 by more than t >= 0) */
__device__ __forceinline__ void edge_neighbour(unsigned int q, edge_u16x2 d, edge_u16x2 t, edge_u16x2 &c, edge_u16x2 &low, edge_u16x2 &high)
{
  const edge_u16x2 one = { 1, 1 };
  const edge_u16x2 qq = edge_pack(q);
  const edge_u16x2 nz = __builtin_elementwise_min(qq, one);
  const edge_u16x2 below = __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_elementwise_sub_sat(d, qq), t), one);
  high = __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_elementwise_sub_sat(qq, d), t), one);
  low = below & nz;
  c += nz & (one ^ (below | high));
}

/* a lane's share of its frame's record */
struct EdgeSums
{
  unsigned int cls[4];
  unsigned int support;
};

/* the pixel pair k (1 .. 4) of the current row C between the rows P above and N below -> the two outputs packed as the samples are,
 * their classes in the low two bytes of *cls2.  live: bit 0 / 1 - the lower / upper pixel exists */
__device__ __forceinline__ unsigned int edge_pair(const EdgeRow &P, const EdgeRow &C, const EdgeRow &N, int k, unsigned int live,
                                                  const ssd_depth_edge_rule &rule, unsigned int *cls2, EdgeSums &S)
{
  const unsigned int dd = C.e[k];
  const unsigned int d0 = dd & 0xffffu, d1 = dd >> 16;
  const edge_u16x2 d = edge_pack(dd);
  const edge_u16x2 t = edge_pack(edge_t(d0, rule) | (edge_t(d1, rule) << 16));
  edge_u16x2 c = { 0, 0 };
  edge_u16x2 loW, hiW, loE, hiE, loN, hiN, loS, hiS, loNW, hiNW, loSE, hiSE, loNE, hiNE, loSW, hiSW;
  edge_neighbour(edge_shift(C.e[k], C.e[k - 1]), d, t, c, loW, hiW);
  edge_neighbour(edge_shift(C.e[k + 1], C.e[k]), d, t, c, loE, hiE);
  edge_neighbour(P.e[k], d, t, c, loN, hiN);
  edge_neighbour(N.e[k], d, t, c, loS, hiS);
  edge_neighbour(edge_shift(P.e[k], P.e[k - 1]), d, t, c, loNW, hiNW);
  edge_neighbour(edge_shift(N.e[k + 1], N.e[k]), d, t, c, loSE, hiSE);
  edge_neighbour(edge_shift(P.e[k + 1], P.e[k]), d, t, c, loNE, hiNE);
  edge_neighbour(edge_shift(N.e[k], N.e[k - 1]), d, t, c, loSW, hiSW);
  const unsigned int bridged = edge_bits((loW & hiE) | (loE & hiW) | (loN & hiS) | (loS & hiN) | (loNW & hiSE) | (loSE & hiNW) |
                                         (loNE & hiSW) | (loSW & hiNE));
  const unsigned int cc = edge_bits(c);
  const unsigned int c0 = cc & 0xffffu, c1 = cc >> 16;
  const int k0 = edge_class(d0, c0, (bridged & 0xffffu) != 0u, rule), k1 = edge_class(d1, c1, (bridged >> 16) != 0u, rule);
#pragma unroll
  for(int i = 0; i < 4; i++)
    S.cls[i] += ((live & 1u) != 0u && k0 == i ? 1u : 0u) + ((live & 2u) != 0u && k1 == i ? 1u : 0u);
  S.support += (k0 == SSD_EDGE_KEPT ? c0 : 0u) + (k1 == SSD_EDGE_KEPT ? c1 : 0u);   /* a pixel that does not exist is EMPTY */
  *cls2 = static_cast<unsigned int>(k0) | (static_cast<unsigned int>(k1) << 8);
  return (k0 == SSD_EDGE_KEPT ? d0 : 0u) | ((k1 == SSD_EDGE_KEPT ? d1 : 0u) << 16);
}

/* WIDE: the width is a multiple of 8 and the frames, the output and the class maps lie on 16 (8) byte boundaries - a strip is one
 * 128-bit load and store, its classes one 64-bit store; otherwise every access is one element, and a width that is no multiple of 8
 * ends every row in a partial strip */
template<bool WIDE>
__global__ __launch_bounds__(kEdgeThreads) void k_depth_edges(const EdgeArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char edgeLds[];
  const int t = static_cast<int>(threadIdx.x), lane = t & 63;
  const int frame = static_cast<int>(blockIdx.x) / A.blocksPerFrame;
  const int task = (static_cast<int>(blockIdx.x) % A.blocksPerFrame) * kEdgeWaves + (t >> 6);      /* wave-uniform */
  const int W = A.W, H = A.H;
  EdgeSums S = {};
  if(task < A.tasks)
  {
    const int x0 = (task % A.spans) * kEdgeSpan + lane * kEdgeStrip;
    const int r0 = (task / A.spans) * kEdgeTile, r1 = r0 + kEdgeTile < H ? r0 + kEdgeTile : H;
    const unsigned short *in = reinterpret_cast<const unsigned short *>(A.frames + static_cast<size_t>(frame) * A.strideBytes);
    unsigned short *out = reinterpret_cast<unsigned short *>(A.out + static_cast<size_t>(frame) * A.outStride);
    unsigned char *cls = A.cls ? A.cls + static_cast<size_t>(frame) * A.clsStride : nullptr;
    unsigned int live = 0u;
#pragma unroll
    for(int e = 0; e < kEdgeStrip; e++)
      live |= x0 + e < W ? 1u << e : 0u;
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
#pragma unroll
      for(int k = 0; k < 4; k++)
        o[k] = edge_pair(P, C, N, k + 1, (live >> (2 * k)) & 3u, A.rule, &kc[k], S);
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
        for(int e = 0; e < kEdgeStrip; e++)
          if(x0 + e < W)
          {
            out[at + e] = static_cast<unsigned short>(o[e >> 1] >> (16 * (e & 1)));
            if(cls)
              cls[at + e] = static_cast<unsigned char>(kc[e >> 1] >> (8 * (e & 1)));
          }
      }
      P = C;
      C = N;
      N = more ? edge_finish(raw, lane) : edge_no_row();
    }
  }
  /* the block's sums into the frame's record */
  unsigned long long acc[kEdgeSumSupport + 1] = { S.cls[0], S.cls[1], S.cls[2], S.cls[3], S.support };
#pragma unroll
  for(int i = 0; i <= kEdgeSumSupport; i++)
  {
#pragma unroll
    for(int o = 32; o >= 1; o >>= 1)
      acc[i] += __shfl_xor(acc[i], o);
  }
  unsigned long long *part = reinterpret_cast<unsigned long long *>(edgeLds);
  if(lane == 0)
  {
#pragma unroll
    for(int i = 0; i <= kEdgeSumSupport; i++)
      part[(t >> 6) * kEdgeWords + i] = acc[i];
  }
  __syncthreads();
  if(t <= kEdgeSumSupport)
  {
    unsigned long long sum = 0ull;
#pragma unroll
    for(int w = 0; w < kEdgeWaves; w++)
      sum += part[w * kEdgeWords + t];
    if(sum != 0ull)
      atomicAdd(A.stats + static_cast<size_t>(frame) * kEdgeWords + t, sum);
  }
}

} // namespace ssd

#endif /* SSD_K_EDGES_H_ */
