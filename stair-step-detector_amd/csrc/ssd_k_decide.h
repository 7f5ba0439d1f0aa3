/* ssd_k_decide.h - quad_decide: the per-point decision of k_inquad (K4, ssd_kernels.hip) and of every kernel that takes it once more for
 * the labels (K7 / K8: ssd_k_labels.h, ssd_k_moments.h, and the refit in ssd_kernels_refit.hip).  A template only: it may be included
 * anywhere in front of its first use.  DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_DECIDE_H_
#define SSD_K_DECIDE_H_
#include "ssd_prefilter.h"

namespace ssd
{

/* The per-point decision of k_inquad and k_labels, for one point slot of the wave: the live quadrilateral of the point's height bin
 * (q; kMaxLive = none) and whether the point counts.  LABELS = false (k_inquad): a ground point inside the ground quadrilateral, a
 * tread point outside its tread's; LABELS = true (k_labels): a point inside the quadrilateral of its bin, ground and treads alike.
 * Also d (the point on K1's grid), M / M3 (the magnitudes the bounds use), mSlow (the lanes that went through the doubles) and
 * mGround (the lanes whose bin is the ground's), which k_inquad's ground raster reads after it. */
template<bool CHECKS, bool LABELS>
__device__ __forceinline__ void quad_decide(const F3 &p, const PreXY &Q, const PreLane lc, const QuadEdgesF *edges,
                                            const unsigned char *lut, const QuadTest *qts, const K1Consts &kc,
                                            const int gSlot, f32x2 &dOut, float &MOut, float &M3Out, unsigned int &qOut,
                                            unsigned long long &mSlowOut, unsigned long long &mCountOut, unsigned long long &mGroundOut)
{
  /* Round 6: every decision in single precision first, as K1 takes them (ssd_prexy.h) - the x / y range, the z range and the
   * height bin, then the quadrilateral as four half-planes on the same d (ssd_quadtest.h, build_quad_edges) - and kept as the
   * wave's lane masks; the reference's doubles - all three rows, the compares, the bin, QuadrilateralTest with its box, map and
   * segments - only for the points within a bound of a limit, a bin edge or a quadrilateral's edge: one wave-uniform block, a wave
   * slot in twenty.  (Until here that test ran for every point of every cell an edge passes through, nested and divergent:
   * 169 vector instructions per point slot, two thirds of the kernel - profiles/r06_k4_ground_kernel.txt.) */
  const PreRange r = pre_range<CHECKS, LABELS>(p, Q, lc);
  const float M3 = r.M3;
  f32x2 d = r.d;
  unsigned long long mSlow = r.mSlow;
  /* the bin's quadrilateral (row kMaxLive: none) and its four edges on d */
  unsigned int q = kMaxLive;
  if(__builtin_amdgcn_inverse_ballot_w64(r.mInSure))
    q = SSD_CHK(28, r.b, kMaxBins) ? lut[r.b] : kMaxLive;
  const unsigned long long mLive = __ballot(q != static_cast<unsigned int>(kMaxLive));
  const QuadEdgesF &E = edges[q];
  const float4 gx = *reinterpret_cast<const float4 *>(E.gx), gy = *reinterpret_cast<const float4 *>(E.gy), g2 = *reinterpret_cast<const float4 *>(E.g2);
  f32x2 e01 = __builtin_elementwise_fma(f32x2{ gx.x, gx.y }, f32x2{ d.x, d.x }, f32x2{ g2.x, g2.y });
  f32x2 e23 = __builtin_elementwise_fma(f32x2{ gx.z, gx.w }, f32x2{ d.x, d.x }, f32x2{ g2.z, g2.w });
  e01 = __builtin_elementwise_fma(f32x2{ gy.x, gy.y }, f32x2{ d.y, d.y }, e01);
  e23 = __builtin_elementwise_fma(f32x2{ gy.z, gy.w }, f32x2{ d.y, d.y }, e23);
  const float emin = min3_f32(e01.x, e01.y, min_f32(e23.x, e23.y));
  const float hq = __builtin_fmaf(M3, Q.dK, E.m);              /* infinity for the row "none" and for a quadrilateral single precision does not serve */
  /* (Measured and not kept: a flag on the list for the cells that lie wholly inside their quadrilaterals - the ground's interior,
   * 58 % of the cells walked - and a wave-uniform branch around these twelve instructions: 0.62 -> 0.70 ms, the branch costs more
   * than it skips.) */
#if defined(SSD_SABOTAGE_PRE) && (SSD_SABOTAGE_PRE & 4)   /* tools: the band along the edges NOT handed to the doubles - the tests built for it must fail */
  const unsigned long long mSureQ = mLive;
#elif defined(SSD_SABOTAGE_PRE) && (SSD_SABOTAGE_PRE & 32)  /* tools: k_labels alone keeps the half-planes' answer inside the quadrilateral band */
  const unsigned long long mSureQ = LABELS ? mLive : __ballot(__builtin_fabsf(emin) > hq);
#else
  const unsigned long long mSureQ = __ballot(__builtin_fabsf(emin) > hq);
#endif
  const unsigned long long mOutQ = __ballot(emin < 0.0f);
  unsigned long long mGround = __ballot(q == static_cast<unsigned int>(gSlot));
  /* k_inquad: for the ground the points inside its quadrilateral count, for treads the points outside theirs (k_raster summed
   * the plateau whole); k_labels: the points inside, ground and treads alike */
  unsigned long long mCount = mSureQ & (LABELS ? ~mOutQ : (mGround ^ mOutQ));
  mSlow |= mLive & ~mSureQ;
  if(__builtin_expect(mSlow != 0ull, 0))
  {
    /* rare, wave-uniform so that the masks stay scalars: the reference's arithmetic, all of it, for the lanes it is for */
    const K1ConstsLds c = k1_consts(kc);
    const World3 w = world_rows(c, p);
    const bool mine = __builtin_amdgcn_inverse_ballot_w64(mSlow);
    const bool inRange = world_in_range(c, w);
    unsigned int qD = kMaxLive;
    bool counts = false;
    if(mine && inRange)
    {
      const int bD = world_bin(c, w);
      qD = SSD_CHK(29, bD, kMaxBins) ? lut[bD] : kMaxLive;
      if(qD != static_cast<unsigned int>(kMaxLive))
      {
        const QuadTest &tq = qts[qD];
        const bool fast = w.x >= tq.fx0 && w.x < tq.fx1 && w.y >= tq.fy0 && w.y < tq.fy1;
        const bool inside = fast || quad_test(tq, w.x, w.y);
        counts = LABELS ? inside : inside == (qD == static_cast<unsigned int>(gSlot));
      }
    }
    mCount = (mCount & ~mSlow) | __ballot(counts);
    mGround = (mGround & ~mSlow) | __ballot(qD == static_cast<unsigned int>(gSlot));
    q = mine ? qD : q;
    /* (each component inside its own conditional, as written: taken whole in front of them the wave's rare block costs
     * k_inquad four more vector registers) */
    d.x = mine ? d_from_world(c, w).x : d.x;
    d.y = mine ? d_from_world(c, w).y : d.y;
  }
  dOut = d; MOut = r.M; M3Out = M3; qOut = q;
  mSlowOut = mSlow; mCountOut = mCount; mGroundOut = mGround;
}

} // namespace ssd

#endif /* SSD_K_DECIDE_H_ */
