/*
 * ssd_k_fuse.h - k_depth_fuse, the depth fusion's one kernel (ssd_enqueue_depth_fuse).  ssd_kernels_ground.hip,
 * the unit of the stand-alone frame passes, includes it and holds its launcher.
 *
 * A stream: every sample of a group is read once (2 bytes) and 2 (+ 1) bytes per pixel come out.  A lane takes eight pixels of every
 * frame of its group - one 128-bit load per frame in the wide body, eight 2-byte loads in the narrow one - so a pair of pixels is one
 * register per frame.  The median comes from Batcher's odd-even merge sort over NP = 1, 2, 4, 8 or 16 such registers, packed 16-bit
 * min / max two pixels at a time; the sort's key is the sample minus one (mod 2^16), which keeps the order of the valid samples and
 * puts every invalid one (0 -> 0xFFFF) above the largest valid key (65534): the first m keys are the valid samples.  The median's
 * index differs per pixel: it is picked by a chain of masked maxima over the sorted registers (ascending: the k-th is the largest of
 * the first k + 1), never by indexing.  m, the agreement, the sum and the deviations come from the ORIGINAL samples (ssd_fuse.h).
 * Frames n .. NP - 1 of a padded size are invalid samples.  A lane keeps the group's seven sums; they are reduced across the wave
 * (shuffles), across the block's waves (dynamic LDS, 256 bytes) and go out as one 64-bit add per block and non-zero word.
 */
#ifndef SSD_K_FUSE_H_
#define SSD_K_FUSE_H_

#include "ssd_fuse.h"

namespace ssd
{

constexpr int kFuseThreads = 256;
constexpr int kFuseWaves = kFuseThreads / 64;
constexpr int kFusePerLane = 8;                                      /* pixels of a lane per step: a unit */
constexpr int kFuseLds = kFuseWaves * kFuseWords * 8;                /* 256 bytes: a multiple of 16 */

typedef unsigned short fuse_u16x2 __attribute__((ext_vector_type(2)));
typedef short fuse_s16x2 __attribute__((ext_vector_type(2)));

struct FuseArgs
{
  const unsigned char *frames;
  size_t strideBytes;
  unsigned char *out;
  size_t outStride;
  unsigned char *support;                    /* null: none */
  size_t supStride;
  unsigned long long *stats;                 /* kFuseWords per group */
  int nPoints, n, hop, ngroups, blocksPerGroup, groupFastest;
  ssd_depth_fuse_rule rule;
};

/* a lane's share of its group's record */
struct FuseSums
{
  unsigned int cls[4];                       /* n_fused, n_empty, n_few, n_split */
  unsigned int valid, agree;
  unsigned long long dev;
};

__device__ __forceinline__ fuse_u16x2 fuse_pack(unsigned int v) { return __builtin_bit_cast(fuse_u16x2, v); }

__device__ __forceinline__ void fuse_cx(fuse_u16x2 &a, fuse_u16x2 &b)
{
  const fuse_u16x2 lo = __builtin_elementwise_min(a, b), hi = __builtin_elementwise_max(a, b);
  a = lo;
  b = hi;
}

/* Batcher's odd-even merge sort, ascending, NP a power of two: every index is a constant once the loops are unrolled */
template<int NP>
__device__ __forceinline__ void fuse_sort(fuse_u16x2 (&k)[NP])
{
#pragma unroll
  for(int p = 1; p < NP; p <<= 1)
  {
#pragma unroll
    for(int q = p; q >= 1; q >>= 1)
    {
#pragma unroll
      for(int j = q % p; j + q < NP; j += 2 * q)
      {
#pragma unroll
        for(int i = 0; i < q; i++)
          if(i + j + q < NP && (i + j) / (2 * p) == (i + j + q) / (2 * p))
            fuse_cx(k[i + j], k[i + j + q]);
      }
    }
  }
}

/* one pixel behind its median: the agreement, the output and the sums (ssd_fuse.h); HALF = which half of the packed samples */
template<int NP, int HALF>
__device__ __forceinline__ void fuse_pixel(const unsigned int (&d)[NP], unsigned int med, bool live, const ssd_depth_fuse_rule &rule,
                                           unsigned int &out, unsigned int &sup, FuseSums &S)
{
  unsigned int m = 0u, c = 0u, s = 0u;
  bool ok[NP];
#pragma unroll
  for(int j = 0; j < NP; j++)
  {
    const unsigned int v = HALF ? d[j] >> 16 : d[j] & 0xffffu;
    ok[j] = fuse_agrees(v, med, static_cast<unsigned int>(rule.tol));
    m += v != 0u ? 1u : 0u;
    c += ok[j] ? 1u : 0u;
    s += ok[j] ? v : 0u;
  }
  int cls;
  out = fuse_output(m, c, s, rule, cls);
  const bool fused = cls == kFuseNFused;
  sup = fused ? c : 0u;
  unsigned int dev = 0u;
#pragma unroll
  for(int j = 0; j < NP; j++)
  {
    const unsigned int v = HALF ? d[j] >> 16 : d[j] & 0xffffu;
    dev += ok[j] ? fuse_dev(v, out) : 0u;
  }
  if(live)
  {
    S.cls[0] += cls == kFuseNFused ? 1u : 0u;
    S.cls[1] += cls == kFuseNEmpty ? 1u : 0u;
    S.cls[2] += cls == kFuseNFew ? 1u : 0u;
    S.cls[3] += cls == kFuseNSplit ? 1u : 0u;
    S.valid += m;
    S.agree += fused ? c : 0u;
    S.dev += fused ? dev : 0u;
  }
}

/* two pixels: d[j] holds their samples of frame j (0: invalid, as every frame behind the group's n).  out: the two outputs packed as
 * the samples are; sup: their support in the low two bytes */
template<int NP>
__device__ __forceinline__ void fuse_pair(const unsigned int (&d)[NP], unsigned int live, const ssd_depth_fuse_rule &rule,
                                          unsigned int &out, unsigned int &sup, FuseSums &S)
{
  fuse_u16x2 k[NP];
  unsigned int mlo = 0u, mhi = 0u;
  const fuse_u16x2 one = { 1, 1 };
#pragma unroll
  for(int j = 0; j < NP; j++)
  {
    k[j] = fuse_pack(d[j]) - one;
    mlo += (d[j] & 0xffffu) != 0u ? 1u : 0u;
    mhi += (d[j] >> 16) != 0u ? 1u : 0u;
  }
  fuse_sort<NP>(k);
  /* the median's index per pixel (-1 where nothing is valid: nothing behind k[0] is taken) */
  const fuse_s16x2 at = { static_cast<short>((static_cast<int>(mlo) - 1) >> 1), static_cast<short>((static_cast<int>(mhi) - 1) >> 1) };
  fuse_u16x2 medKey = k[0];
#pragma unroll
  for(int j = 1; j < NP; j++)
  {
    const fuse_s16x2 jm1 = { static_cast<short>(j - 1), static_cast<short>(j - 1) };
    const fuse_s16x2 take = (jm1 - at) >> 15;                      /* all ones where at >= j */
    medKey = __builtin_elementwise_max(medKey, k[j] & __builtin_bit_cast(fuse_u16x2, take));
  }
  const fuse_u16x2 med = medKey + one;
  unsigned int o0, o1, s0, s1;
  fuse_pixel<NP, 0>(d, med.x, (live & 1u) != 0u, rule, o0, s0, S);
  fuse_pixel<NP, 1>(d, med.y, (live & 2u) != 0u, rule, o1, s1, S);
  out = o0 | (o1 << 16);
  sup = s0 | (s1 << 8);
}

/* NP: the network's size, n in (NP / 2, NP].  WIDE: the frames, the output and the support lie on 16 (8) byte boundaries - a lane's
 * unit is eight neighbouring pixels, one 128-bit load per frame and one store; the pixels behind the last whole unit, and everything
 * when !WIDE, go element by element, where !WIDE a block's units interleaved so that a wave's loads are neighbours. */
template<int NP, bool WIDE>
__global__ __launch_bounds__(kFuseThreads) void k_depth_fuse(const FuseArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char fuseLds[];
  const int bid = static_cast<int>(blockIdx.x);
  const int group = A.groupFastest ? bid % A.ngroups : bid / A.blocksPerGroup;
  const int chunk = A.groupFastest ? bid / A.ngroups : bid % A.blocksPerGroup;
  const int t = static_cast<int>(threadIdx.x);
  const int nPoints = A.nPoints, n = A.n;
  const unsigned char *base = A.frames + static_cast<size_t>(group) * A.hop * A.strideBytes;
  unsigned char *outRow = A.out + static_cast<size_t>(group) * A.outStride;
  unsigned char *supRow = A.support ? A.support + static_cast<size_t>(group) * A.supStride : nullptr;
  const int wholeUnits = nPoints / kFusePerLane, units = (nPoints + kFusePerLane - 1) / kFusePerLane;
  FuseSums S = {};
  for(int ub = chunk * kFuseThreads; ub < units; ub += A.blocksPerGroup * kFuseThreads)
  {
    const int u = ub + t;
    const bool whole = WIDE && u < wholeUnits;
    unsigned int d[4][NP];
    int pix[kFusePerLane];
    unsigned int live = 0u;
#pragma unroll
    for(int e = 0; e < kFusePerLane; e++)
    {
      pix[e] = WIDE ? u * kFusePerLane + e : ub * kFusePerLane + e * kFuseThreads + t;
      live |= pix[e] < nPoints ? 1u << e : 0u;
    }
    if(whole)
    {
#pragma unroll
      for(int j = 0; j < NP; j++)
      {
        const int jj = j < n ? j : n - 1;                              /* a padded frame: loaded all the same, then invalid */
        uint4 r = *reinterpret_cast<const uint4 *>(base + static_cast<size_t>(jj) * A.strideBytes + static_cast<size_t>(u) * 16);
        if(j >= n)
          r = make_uint4(0u, 0u, 0u, 0u);
        d[0][j] = r.x; d[1][j] = r.y; d[2][j] = r.z; d[3][j] = r.w;
      }
    }
    else
    {
#pragma unroll
      for(int j = 0; j < NP; j++)
      {
        const int jj = j < n ? j : n - 1;
        const unsigned short *dep = reinterpret_cast<const unsigned short *>(base + static_cast<size_t>(jj) * A.strideBytes);
        unsigned int v[kFusePerLane];
#pragma unroll
        for(int e = 0; e < kFusePerLane; e++)
        {
          const int p = pix[e] < nPoints ? pix[e] : nPoints - 1;       /* the load stays inside the frame */
          v[e] = dep[p];
          if(j >= n || pix[e] >= nPoints)
            v[e] = 0u;
        }
#pragma unroll
        for(int w = 0; w < 4; w++)
          d[w][j] = v[2 * w] | (v[2 * w + 1] << 16);
      }
    }
    unsigned int o[4], sp[4];
#pragma unroll
    for(int w = 0; w < 4; w++)
      fuse_pair<NP>(d[w], (live >> (2 * w)) & 3u, A.rule, o[w], sp[w], S);
    if(whole)
    {
      *reinterpret_cast<uint4 *>(outRow + static_cast<size_t>(u) * 16) = make_uint4(o[0], o[1], o[2], o[3]);
      if(supRow)
        *reinterpret_cast<uint2 *>(supRow + static_cast<size_t>(u) * 8) = make_uint2(sp[0] | (sp[1] << 16), sp[2] | (sp[3] << 16));
    }
    else
    {
#pragma unroll
      for(int e = 0; e < kFusePerLane; e++)
        if(pix[e] < nPoints)
        {
          reinterpret_cast<unsigned short *>(outRow)[pix[e]] = static_cast<unsigned short>(o[e >> 1] >> (16 * (e & 1)));
          if(supRow)
            supRow[pix[e]] = static_cast<unsigned char>(sp[e >> 1] >> (8 * (e & 1)));
        }
    }
  }
  /* the block's sums into the group's record */
  unsigned long long acc[kFuseWords - 1] = { S.cls[0], S.cls[1], S.cls[2], S.cls[3], S.valid, S.agree, S.dev };
#pragma unroll
  for(int i = 0; i < kFuseWords - 1; i++)
  {
#pragma unroll
    for(int o = 32; o >= 1; o >>= 1)
      acc[i] += __shfl_xor(acc[i], o);
  }
  unsigned long long *part = reinterpret_cast<unsigned long long *>(fuseLds);
  if((t & 63) == 0)
  {
#pragma unroll
    for(int i = 0; i < kFuseWords - 1; i++)
      part[(t >> 6) * kFuseWords + i] = acc[i];
  }
  __syncthreads();
  if(t < kFuseWords - 1)
  {
    unsigned long long sum = 0ull;
#pragma unroll
    for(int w = 0; w < kFuseWaves; w++)
      sum += part[w * kFuseWords + t];
    if(sum != 0ull)
      atomicAdd(A.stats + static_cast<size_t>(group) * kFuseWords + t, sum);
  }
}

} // namespace ssd

#endif /* SSD_K_FUSE_H_ */
