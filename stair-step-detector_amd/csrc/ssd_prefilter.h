/*
 * ssd_prefilter.h — the per-point pre-filter on the device, stated once for K1 (hist_block), k_inquad and k_labels (quad_decide).
 *
 * A point's range test, height bin, grid coordinate d and pixel are taken in single precision first; the constants and the proof
 * of their bounds are the host's (ssd_prexy.h: make_pre_xy, make_pre_z, make_pre_pixel; PreXY and PixelParams, ssd_device.h).  Each
 * answer is "in range for sure / outside for sure / ask the reference's doubles", and the doubles' side - the reference's rows,
 * compares, bin and pixel from a copy of the constants in LDS (K1Consts) - is here as well.  tests/prefilter_model.py is the same
 * logic as one Python function.  The tools' switches that leave a band with single precision (-DSSD_SABOTAGE_PRE, bits 1, 2, 8, 16
 * and the bin half of 32) stand here and nowhere else; the half-planes of a quadrilateral (bits 4 and 32) are quad_decide's.
 *
 * A header in its own right: F3 and kThreads are ssd_k_point.h's.  Everything is inlined into its caller: the masks are
 * the wave's 64-bit lane masks in scalar registers, the helpers take values and return values.
 */
#ifndef SSD_PREFILTER_H_
#define SSD_PREFILTER_H_
#include "ssd_k_point.h"

namespace ssd
{

/* ---- single instructions ---- */
typedef float f32x2 __attribute__((ext_vector_type(2)));
/* (d.x, d.y): the point's world x / y, centred on the measuring range and divided by its extent - three packed FMAs */
__device__ __forceinline__ f32x2 pre_xy(const PreXY &Q, const f32x2 c3, float x, float y, float z)
{
  f32x2 d = __builtin_elementwise_fma(f32x2{ Q.c[2][0], Q.c[2][1] }, f32x2{ z, z }, c3);
  d = __builtin_elementwise_fma(f32x2{ Q.c[1][0], Q.c[1][1] }, f32x2{ y, y }, d);
  d = __builtin_elementwise_fma(f32x2{ Q.c[0][0], Q.c[0][1] }, f32x2{ x, x }, d);
  return d;
}
/* single instructions with |.| on the operands (as builtins the compiler canonicalises fmaxf's operands first: v_max x, x) */
__device__ __forceinline__ float absmax2(float a, float b)
{
  float r;
  asm("v_max_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float absmax3(float a, float b, float c)
{
  float r;
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
/* truncating conversion that saturates (negative and NaN: 0) instead of being undefined */
__device__ __forceinline__ unsigned int cvt_u32_f32(float a)
{
  unsigned int r;
  asm("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(a));
  return r;
}
__device__ __forceinline__ float min3_f32(float a, float b, float c)
{
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float min_f32(float a, float b)
{
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float max_f32(float a, float b)
{
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

/* The lane's copies of the constants that are the SECOND scalar operand of an instruction (one is allowed): the z row's fourth
 * coefficient, the threshold's offset, the x / y rows' fourth pair - without them a v_mov per use and point.  The empty asm pins
 * them to vector registers: the compiler would otherwise fold them back into the scalar operands they came from. */
struct PreLane
{
  float zc3, zh0;
  f32x2 c3xy;
  __device__ __forceinline__ explicit PreLane(const PreXY &Q) : zc3(Q.zc[3]), zh0(Q.zH0), c3xy(f32x2{ Q.c[3][0], Q.c[3][1] })
  {
    asm volatile("" : "+v"(zc3), "+v"(zh0), "+v"(c3xy));
  }
};

/* ---- the range test and the bin in single precision ---- */

/* What single precision says about one point slot of the wave.  mValid: z > 0, a measurement (pointcloud.cpp:143-146).  mInSure: in
 * range for sure, and b is the reference's bin.  mSlow: possibly in range - neither test says "outside for sure" - with a test
 * unsure: those take the doubles.  Every other lane is out of range.  d: the point on K1's grid (pre_xy); M = max(|d.x|, |d.y|),
 * M3 = max(|x|, |y|, |z|): the magnitudes the bounds use. */
struct PreRange
{
  unsigned long long mValid, mInSure, mSlow;
  unsigned int b;
  f32x2 d;
  float M, M3;
};
/* The tests' outcomes are kept as the wave's 64-bit lane masks (one v_cmp each, straight into a scalar register pair) and combined
 * on the scalar unit; as `bool`s the compiler evaluated two of them in BOTH polarities - a second v_cmp each, 25 M vector
 * instructions per launch - where one s_andn2 does.  __builtin_amdgcn_inverse_ballot_w64 turns a mask back into the lanes' branch.
 * CHECKS: the rare configurations' tests (the launchers pick the instantiation, needs_checks()); LABELS: k_labels, for the tools'
 * switch that is its alone. */
template<bool CHECKS, bool LABELS>
__device__ __forceinline__ PreRange pre_range(const F3 &p, const PreXY &Q, const PreLane C)
{
  PreRange r;
  r.mValid = __ballot(p.z > 0.0f);
  /* x / y (round 5): inside for sure, outside for sure (M > hi), or the band between them (and NaNs) */
  r.d = pre_xy(Q, C.c3xy, p.x, p.y, p.z);
  r.M = absmax2(r.d.x, r.d.y);
  unsigned long long mInxy = __ballot(r.M < Q.lo);
  unsigned long long mMaybexy = ~__ballot(r.M > Q.hi);
  r.M3 = absmax3(p.x, p.y, p.z);
  if constexpr(CHECKS)
  {
    /* unless make_pre_xy() showed that larger inputs cannot read "inside" */
#if defined(SSD_SABOTAGE_PRE) && (SSD_SABOTAGE_PRE & 16)  /* tools: inputs beyond PreXY::maxInput NOT handed to the doubles - the tests built for it must fail */
    const unsigned long long mFar = 0ull;
#else
    const unsigned long long mFar = Q.checkInput ? ~__ballot(r.M3 <= Q.maxInput) : 0ull;
#endif
    mInxy &= ~mFar;
    mMaybexy |= mFar;
  }
  /* z (round 6, make_pre_z()): t = the height above zMin in bins.  Farther from every integer than the bound for this point's
   * magnitude: the bin is floor(t) and the z range is 0 < t < zTop, as the doubles would say */
  const float t = __builtin_fmaf(Q.zc[0], p.x, __builtin_fmaf(Q.zc[1], p.y, __builtin_fmaf(Q.zc[2], p.z, C.zc3)));
  const float g = __builtin_amdgcn_fractf(t) - 0.5f;
  const float h = __builtin_fmaf(r.M3, Q.zNegK, C.zh0);
  unsigned long long mSurez = __ballot(__builtin_fabsf(g) < h);      /* not for a NaN, nor for a magnitude whose bound exceeds half a bin */
  const unsigned long long mInz = __ballot(__float_as_uint(t) < Q.zTopBits);     /* +0 <= t < zTop on the bits (a negative t has the sign bit) */
  if constexpr(CHECKS)
  {
#if defined(SSD_SABOTAGE_PRE) && (SSD_SABOTAGE_PRE & 8)   /* tools: the band at the top of a z range that ends mid-bin NOT handed to the doubles */
    if(false)
#else
    if(Q.zCheckTop)
#endif
      mSurez &= __ballot(__builtin_fabsf(t - Q.zTop) > 0.5f - h);    /* the range's upper end is no bin edge: its own band */
  }
#if defined(SSD_SABOTAGE_PRE) && (SSD_SABOTAGE_PRE & 1)   /* tools: the band around the bin edges NOT handed to the doubles - the tests built for it must fail */
  mSurez = ~0ull;
#endif
#if defined(SSD_SABOTAGE_PRE) && (SSD_SABOTAGE_PRE & 32)  /* tools: k_labels alone keeps the single-precision bin inside the bin band */
  if(LABELS)
    mSurez = ~0ull;
#endif
  r.b = cvt_u32_f32(t);
  r.mInSure = r.mValid & mInz & mInxy & mSurez;
  r.mSlow = r.mValid & mMaybexy & (~mSurez | (mInz & ~mInxy));
  return r;
}

/* ---- the reference's doubles ---- */

/* The constants of the seldom-run pieces - the double-precision rows of a point the pre-filter cannot call - live in LDS, copied
 * there once per block: as kernel arguments of the plain k_hist they would sit in scalar registers through the whole point loop
 * for one lane in thousands (with them the loop's own constants were spilled and came back through a dozen v_readlane per point). */
struct K1Consts
{
  double a[9], b[3];                              /* CameraToWorld, all three rows */
  double xMin, xMax, yMin, yMax, zMin, zMax;
  double boxX, boxY;
  double recip;
  double xToImage, yToImage;                      /* Projection2D, for the pixel single precision cannot call (pre_pixel) */
};
/* one thread's work, before the block's barrier; X = nullptr: a kernel that asks for no pixel */
__device__ __forceinline__ void k1_consts_fill(K1Consts &c, const PointParams &P, const PixelParams *X)
{
#pragma unroll
  for(int i = 0; i < 9; i++)
    c.a[i] = P.a[i];
  c.b[0] = P.b[0]; c.b[1] = P.b[1]; c.b[2] = P.b[2];
  c.xMin = P.xMin; c.xMax = P.xMax; c.yMin = P.yMin; c.yMax = P.yMax; c.zMin = P.zMin; c.zMax = P.zMax;
  c.boxX = P.boxX; c.boxY = P.boxY;
  c.recip = P.recip;
  c.xToImage = X ? X->xToImage : 0.0; c.yToImage = X ? X->yToImage : 0.0;
}
/* the address of the block's copy, opaque to the compiler at every use: loads from it stay where they are written (hoisted
 * out of the point loop they would occupy thirty-two vector registers for its whole length) */
typedef const K1Consts __attribute__((address_space(3))) *K1ConstsLds;
__device__ __forceinline__ K1ConstsLds k1_consts(const K1Consts &c)
{
  K1ConstsLds p = (K1ConstsLds)(&c);
  asm volatile("" : "+v"(p));
  return p;
}

/* CameraToWorld as the reference computes it (transformation.h:59-64, world_point_flat): float promoted to double, row sums left to
 * right, then the translation.  WITH_Z = false: the x and y rows only (z is left 0), for a pixel. */
struct World3 { double x, y, z; };
template<bool WITH_Z = true>
__device__ __forceinline__ World3 world_rows(const K1ConstsLds c, const F3 &p)
{
  const double x = p.x, y = p.y, z = p.z;
  World3 w;
  w.x = (c->a[0] * x + c->a[1] * y) + c->a[2] * z;
  w.y = (c->a[3] * x + c->a[4] * y) + c->a[5] * z;
  w.z = 0.0;
  if constexpr(WITH_Z)
    w.z = (c->a[6] * x + c->a[7] * y) + c->a[8] * z;
  w.x = w.x + c->b[0];
  w.y = w.y + c->b[1];
  if constexpr(WITH_Z)
    w.z = w.z + c->b[2];
  return w;
}
/* the six strict compares of getPointsInRange (pointcloud.cpp:150-165), without short circuit */
__device__ __forceinline__ bool world_in_range(const K1ConstsLds c, const World3 &w)
{
  return (w.x > c->xMin) & (w.x < c->xMax) & (w.y > c->yMin) & (w.y < c->yMax) & (w.z > c->zMin) & (w.z < c->zMax);
}
/* calcHeights (pointcloud.cpp:175, height_bin); meaningless for a point out of range, as is d_from_world */
__device__ __forceinline__ int world_bin(const K1ConstsLds c, const World3 &w)
{
  return static_cast<int>((w.z - c->zMin) * c->recip);
}
/* d made again from the doubles: D rounded once, inside PreXY::dE0 */
__device__ __forceinline__ f32x2 d_from_world(const K1ConstsLds c, const World3 &w)
{
  return f32x2{ static_cast<float>((w.x - c->xMin) * c->boxX * 0.00390625 - 0.5), static_cast<float>((w.y - c->yMin) * c->boxY * 0.00390625 - 0.5) };
}

/* ---- the pixel ---- */

/* Projection2D::worldToImage (pointcloud.cpp:79-83) of an in-range point: from the single-precision d of the range test where that
 * is certain (round 6, make_pre_pixel()): px = (d.x + 1/2) W and py = (1/2 - d.y) H farther from every integer than the bound for
 * this point's magnitude M3 truncate to the reference's pixel - and lie inside the image, 0 and W / H being integers; the others
 * take the reference's rows and pixel in doubles, with the image's bounds.  Returns whether (ix, iy) lies inside the image; a
 * pixel outside it is the caller's to count (quirk Q5). */
__device__ __forceinline__ bool pre_pixel(const F3 &p, const f32x2 d, const float M3, const PixelParams &X, const K1Consts &kc, int &ix, int &iy)
{
  const float px = __builtin_fmaf(d.x, X.fW, X.fHalfW), py = __builtin_fmaf(d.y, X.fNegH, X.fHalfH);
  const f32x2 gg = f32x2{ __builtin_amdgcn_fractf(px), __builtin_amdgcn_fractf(py) } + f32x2{ -0.5f, -0.5f };      /* one packed add */
  const float hp = __builtin_fmaf(M3, X.pxNegK, X.pxH0);
  ix = static_cast<int>(cvt_u32_f32(px));
  iy = static_cast<int>(cvt_u32_f32(py));
  bool inside = true;
#if defined(SSD_SABOTAGE_PRE) && (SSD_SABOTAGE_PRE & 2)   /* tools: the band around the pixel edges NOT handed to the doubles - the tests built for it must fail */
  if(false)
#else
  if(!(absmax2(gg.x, gg.y) < hp))
#endif
  {
    /* rare */
    const K1ConstsLds c = k1_consts(kc);
    const World3 w = world_rows<false>(c, p);
    ix = static_cast<int>((w.x - c->xMin) * c->xToImage);
    iy = static_cast<int>((c->yMax - w.y) * c->yToImage);
    inside = (static_cast<unsigned int>(ix) < static_cast<unsigned int>(X.W)) & (static_cast<unsigned int>(iy) < static_cast<unsigned int>(X.H));
  }
  return inside;
}

/* ---- a frame's edge table for the single-precision half-planes (quad_decide) ---- */

/* Word w of the table in LDS from word e of FrameState::edgeLive: a row per live quadrilateral, m (word 12 of a row) with
 * PreXY::dE0 - the bound of d that does not depend on the point - folded in; the row behind the egWords live ones, the row of a
 * bin without quadrilateral, answers "not for sure" to everything. */
__device__ __forceinline__ float quad_edge_word(int w, int egWords, float e, float dE0)
{
  return w < egWords ? ((w & 15) == 12 ? e + dE0 : e) : ((w & 15) == 12 ? INFINITY : 0.0f);
}
/* the whole table, by the block (kThreads threads; the barrier is the caller's) */
__device__ __forceinline__ void stage_quad_edges(QuadEdgesF *dst, const QuadEdgesF *src, int egWords, float dE0)
{
  for(int w = threadIdx.x; w < egWords + 16; w += kThreads)
    reinterpret_cast<float *>(dst)[w] = quad_edge_word(w, egWords, w < egWords ? reinterpret_cast<const float *>(src)[w] : 0.0f, dE0);
}

} // namespace ssd

#endif /* SSD_PREFILTER_H_ */
