/*
 * ssd_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the per-frame point-cloud path.
 *
 * Pipeline over a batch of F frames resident in HBM (grid.x = frame everywhere: see the launch note on XCD balance):
 *   K1 k_hist      transform + crop + 1 cm height bin + histogram      (pointcloud.cpp:122-204)
 *   K1b k_peaks    peaks, filter, plateau pairs, bin->plateau LUT      (pointcloud.cpp:214-343, 399-418)
 *   K2 k_raster    top-down bit images of the step plateaus            (pointcloud.cpp:458-471)
 *   K3 k_outline   3x3 close + scans + best lines + corners            (segmentation.cpp:919-971)
 *   K3b k_quads    ground quadrilateral, point-in-quad tests           (pointcloud.cpp:431-443,489-512; quadrilateralTest.cpp:275-443)
 *   K4 k_inquad    in-quad filter, z sums, ground image                (pointcloud.cpp:560-581, 530-531)
 *                  (range, bin and quadrilateral in single precision first, round 6: ssd_prexy.h, ssd_quadtest.h build_quad_edges)
 *   K5 k_final     ground front edge, mean z, ToExternalWorld, result  (segmentation.cpp:879-917; pointcloud.cpp:532-547, 370-383)
 *
 * All floating-point work is fp64 with contraction off (the file is compiled with
 * -ffp-contract=off): the reference is built without FMA (CMakeLists.txt:23-28) and one
 * flipped bin or pixel moves a corner by more than the parity bar.
 * K1 is HBM-read bound (12 B per raw point), K2 / K4 re-read a third of the points and are VALU-issue bound; no MFMA anywhere.
 *
 * Batches of 64 XGA frames' worth of points and more (vertex input, the whole pipeline in one call) run the SINGLE PASS instead:
 *   K0 k_predict      histogram of a sample of the frame -> the height bins that may hold a step plateau, a plane (bit image) each
 *   K1 k_hist_planes  k_hist, and the raster of those bins' points into their planes
 *   K1b k_peaks       ... and which step plateaus the planes cover; the frames with others on k_raster's work list
 *   K2 k_raster       only the listed frames' uncovered plateaus
 *   K3 k_outline      reads a covered plateau's plane(s) in place of its step image
 * Nothing the predictor says can change a result ("The single pass").
 */
/* What the stages share stands in headers that compile alone - ssd_k_entry.h (SSD_ENTRY / SSD_BYVAL and the tools builds' macros),
 * ssd_k_point.h, ssd_k_cells.h, ssd_k_windows.h, ssd_prefilter.h - and the launch rules in ssd_launch_rules.h.  The chain's bodies,
 * K1, K0, K1b, K2, K3, K3b, K4 and K5, stand here; the extension stages are headers too, included where their text stood:
 * ssd_k_decide.h (quad_decide, K4's and the labels'), ssd_k_labels.h (K7) and ssd_k_moments.h (K8) behind K4, ssd_k_risers.h (K6) behind
 * K5 (with the reason why the place matters).  For the chain's bodies this file is still compiled twice: by itself
 * it is the one-calibration path, and ssd_kernels_cams.hip defines SSD_CAMERAS_TU and includes it for the device code alone
 * (ssd_k_entry.h says what the macro does to the kernels whose body stands in the entry point).  The entry points that only call a
 * stage's *_block, and the launchers, stand in one stretch at the end of the file: what that includer leaves out, and all that it
 * leaves out. */
#include "ssd_k_entry.h"
#include "ssd_k_point.h"
#include "ssd_k_cells.h"
#include "ssd_k_windows.h"
#include "ssd_prefilter.h"   /* the per-point pre-filter: pre_range, the doubles' rows from K1Consts, pre_pixel, the edge table */
#include "ssd_k_decide.h"    /* quad_decide: a template, so its place among the kernels is free */

namespace ssd
{

/* The streaming kernels are written as block bodies over an explicit LDS struct, (frame, chunk) given by the caller:
 * the kernels below pass blockIdx (tools and experiments have paired two bodies in one launch: DESIGN.md section 3). */

/* the cell's five reductions over the 16 lanes of a DPP row (groups: OR; the box: two minima, two maxima of the lanes' d), in one
 * block of twenty instructions behind a two-cycle no-op, the five chains interleaved so that no DPP operand is read within two instructions of its write
 * (the wait states the hardware asks for; the compiler does not see into the block) */
__device__ __forceinline__ void row_reduce_cell(unsigned int &groups, float &x0, float &x1, float &y0, float &y1)
{
  /* s_nop 1 first: the hazard recogniser does not look into the block, and nothing else guarantees that the instruction in front of
   * it has not just written one of the first two operands (a DPP read within two wait states of the write takes stale lanes) */
  asm("s_nop 1\n\t"
      "v_or_b32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %4, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
      "v_or_b32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %1, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %2, %2, %2 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %3, %3, %3 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %4, %4, %4 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
      "v_or_b32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %1, %1, %1 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %2, %2, %2 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %3, %3, %3 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %4, %4, %4 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
      "v_or_b32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %1, %1, %1 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %2, %2, %2 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_min_f32_dpp %3, %3, %3 row_ror:1 row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %4, %4, %4 row_ror:1 row_mask:0xf bank_mask:0xf"
      : "+v"(groups), "+v"(x0), "+v"(x1), "+v"(y0), "+v"(y1));
}
/* the cell's box from the extremes of d: rn(d * 256 + boxLo / boxHi) saturated to 0 .. 255, one byte each (ssd_prexy.h) */
__device__ __forceinline__ unsigned int cell_box_from_d(const PreXY &Q, float x0, float x1, float y0, float y1)
{
  /* (x0, x1) and (y0, y1) scaled and shifted by one packed FMA each */
  const f32x2 scale = f32x2{ 256.0f, 256.0f }, shift = f32x2{ Q.boxLo, Q.boxHi };
  const f32x2 bx = __builtin_elementwise_fma(f32x2{ x0, x1 }, scale, shift), by = __builtin_elementwise_fma(f32x2{ y0, y1 }, scale, shift);
  unsigned int box = __builtin_amdgcn_cvt_pk_u8_f32(bx.x, 0u, 0u);
  box = __builtin_amdgcn_cvt_pk_u8_f32(bx.y, 1u, box);
  box = __builtin_amdgcn_cvt_pk_u8_f32(by.x, 2u, box);
  box = __builtin_amdgcn_cvt_pk_u8_f32(by.y, 3u, box);
  return box;
}

/* what the single pass adds to K1's LDS */
struct SpecLds
{
  unsigned long long wins[kThreads / 64][kSpecWinWords];
  ImageBox boxes[kMaxPlanes];
  unsigned char plane[kMaxBins];                 /* FrameState::specPlane */
  unsigned char order[kMaxTilesPerBlock * (kTile / 256)];   /* STRIPS: the chunk's 256-point strips by (column band, index) */
  unsigned int oob[kMaxPlanes];
  unsigned long long ltot[kMaxPlanes][8];        /* sum of round(z * 2^40) per plane (this block's share) */
};
struct NoSpecLds {};

struct HistLds
{
  K1Consts kc;
  uint2 lInfo[kMaxCellsPerBlock];
  /* [bin][copy]: a vote goes to copy = lane & 31, i.e. LDS bank = copy: the 32 lanes the LDS serves per
   * cycle never collide, whatever their bins (a camera row sweeping one plateau puts all 64 lanes in one bin) */
  alignas(16) unsigned int lh[kMaxBins * kHistCopies];      /* 16-byte aligned: cleared and summed four copies at a time */
  unsigned int lNonZero;
};
static_assert(kHistCopies % 8 == 0 && (kMaxBins * kHistCopies / 4) % kThreads == 0 && kMaxBins * 2 == kThreads,
              "hist_block clears the LDS histogram in 16-byte pieces and sums a bin's copies with two threads");

/* SPEC (single pass): the block also rasters the points of the bins that have a plane (FrameState::specPlane, k_predict) into
 * the frame's planes, as k_raster does for the plateaus' bins: pixel (image_pixel), the plane's z sum and out-of-image count. */
template<int SRC, bool SPEC, bool STRIPS, bool CHECKS, typename SPECLDS>
__device__ __forceinline__ void hist_block(HistLds &L, SPECLDS &SL, const float *__restrict__ xyz, size_t strideFloats, const PointParams &P,
                                           const PreXY &Q, const PixelParams &X, FrameState *__restrict__ st, uint2 *__restrict__ tileMasks,
                                           unsigned long long *__restrict__ planeImg,
                                           size_t tileMaskStride, int chunkPoints, const DepthSrc &D, const int frame, const int chunkIdx)
{
  uint2 (&lInfo)[kMaxCellsPerBlock] = L.lInfo;
  unsigned int (&lh)[kMaxBins * kHistCopies] = L.lh;
  unsigned int &lNonZero = L.lNonZero;

  const int tid = threadIdx.x, lane = tid & 63;
  SpecWindow win;
  SpecMiss missed;
  int curT = -1;
  unsigned long long accT = 0;
  const unsigned int imgWords = static_cast<unsigned int>(X.H) * static_cast<unsigned int>(X.W64);
  unsigned long long *frameImg = nullptr;
  if constexpr(SPEC)
  {
    frameImg = planeImg + static_cast<size_t>(st[frame].planeBase) * imgWords;          /* the frame's planes in the pool (k_predict) */
    const unsigned char planeMine = tid < kMaxBins ? st[frame].specPlane[tid] : static_cast<unsigned char>(0xff);
    if(tid < kMaxBins)
      SL.plane[tid] = planeMine;
    if(tid < kMaxPlanes)
    {
      SL.boxes[tid] = ImageBox{ 0x7fffffff, -1, 0x7fffffff, -1 };
      SL.oob[tid] = 0u;
    }
    if(tid < kMaxPlanes * 8)
      (&SL.ltot[0][0])[tid] = 0ull;
    for(int i = tid; i < (kThreads / 64) * kSpecWinWords; i += kThreads)
      (&SL.wins[0][0])[i] = 0ull;
  }
  /* strideFloats counts floats, or 16-bit depth values for kSrcDepth16 */
  const float *base = SRC == kSrcDepth16
    ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(xyz) + static_cast<size_t>(frame) * strideFloats)
    : xyz + static_cast<size_t>(frame) * strideFloats;
  const int begin = chunkIdx * chunkPoints;
  const int end = min(begin + chunkPoints, P.nPoints);

  /* (16 bytes per store: a block's prologue and epilogue are ~14 % of K1's vector instructions, round 6) */
  for(int i = tid; i < kMaxBins * kHistCopies / 4; i += kThreads)
    reinterpret_cast<uint4 *>(lh)[i] = make_uint4(0u, 0u, 0u, 0u);
  if(tid == 0)
  {
    lNonZero = 0;
    k1_consts_fill(L.kc, P, SPEC ? &X : nullptr);
  }
  __syncthreads();

  unsigned int *mine = lh + (lane & (kHistCopies - 1));
  unsigned int nz = 0;                                               /* wave-uniform: the count of the whole wave (scalar popcounts) */
  int it = 0;
  int nStore = -1;                                                    /* cell records to store (STRIPS), else it * kCellsPerTile */

  const PreLane lc(Q);

  /* SPEC: a point of a candidate bin (in range, its bin has plane `plane`): its share of the plane's z sum, its pixel key.
   * projectToBinaryImage (pointcloud.cpp:458-471) for a bin that may turn out a plateau's.  The z sum takes the reference's doubles
   * (world_point_flat's z row), the pixel is pre_pixel()'s. */
  auto candidatePoint = [&](const F3 &q, const f32x2 dj, const int plane) -> unsigned int
  {
    if constexpr(!SPEC)
      return kNoPixel;
    else
    {
    const double x = q.x, y = q.y, z = q.z;
    double wz = (P.a[6] * x + P.a[7] * y) + P.a[8] * z;
    wz = wz + P.b[2];
    int ix, iy;
    const bool inside = pre_pixel(q, dj, absmax3(q.x, q.y, q.z), X, L.kc, ix, iy);
    if(!inside && SSD_CHK(14, plane, kMaxPlanes))
      atomicAdd(&SL.oob[plane], 1u);                     /* quirk Q5 */
    if(plane != curT)
    {
      if(curT >= 0 && SSD_CHK(13, curT, kMaxPlanes))
        atomicAdd(&SL.ltot[curT][lane & 7], accT);
      curT = plane;
      accT = 0;
    }
    accT += static_cast<unsigned long long>(z_plus_magic_bits(wz));      /* the bits of z + 6144; k_peaks takes the constant's share off (count x kMagicBits) */
    return inside ? pixel_key(plane, iy, ix) : kNoPixel;
    }
  };

  auto tileBody = [&](const F3 (&v)[kPts], const int cellAt)
  {
    unsigned int groups = 0u;
    /* extremes of d (pre_xy) over the lane's in-range points: the cell's box */
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    unsigned int planes[kPts] = { 0xffu, 0xffu, 0xffu, 0xffu };     /* SPEC: the plane of the point's bin (0xff: none, or the point is out of range) */
    /* SPEC: the points' d, for their pixels - kept where the registers are there (the tile loop on vertex input), made again otherwise */
    constexpr bool kKeepD = SPEC && !STRIPS && SRC != kSrcDepth16;
    f32x2 dk[kPts];
    unsigned int keys[kPts] = { kNoPixel, kNoPixel, kNoPixel, kNoPixel };
#pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      const F3 p{ v[j].x, v[j].y, v[j].z };
      const PreRange r = pre_range<CHECKS, false>(p, Q, lc);
      nz += static_cast<unsigned int>(__popcll(r.mValid));               /* pointcloud.cpp:143-146, counted per wave on the scalar unit */
      unsigned int b = r.b;
      f32x2 d = r.d;
      unsigned long long mIn = r.mInSure;
      if(r.mSlow != 0ull)
      {
        /* rare (one wave slot in fifty; a wave-uniform branch, so that the mask stays a scalar): the reference's arithmetic, all of it -
         * world_point_flat's rows and compares, height_bin - evaluated by the whole wave, taken by the lanes it is for */
        const K1ConstsLds c = k1_consts(L.kc);
        const World3 w = world_rows(c, p);
        mIn |= r.mSlow & __ballot(world_in_range(c, w));
        const bool mine = __builtin_amdgcn_inverse_ballot_w64(r.mSlow);
        const unsigned int bD = static_cast<unsigned int>(world_bin(c, w));
        const f32x2 dD = d_from_world(c, w);
        b = mine ? bD : b;
        d.x = mine ? dD.x : d.x;
        d.y = mine ? dD.y : d.y;
      }
      if(__builtin_amdgcn_inverse_ballot_w64(mIn))
      {
        if(SSD_CHK(11, b, P.nBins))
          atomicAdd(mine + b * kHistCopies, 1u);                          /* ++hist[bin], pointcloud.cpp:199-202 */
        groups |= 1u << (b / static_cast<unsigned int>(kBinsPerGroup));
        x0 = min_f32(x0, d.x); x1 = max_f32(x1, d.x);
        y0 = min_f32(y0, d.y); y1 = max_f32(y1, d.y);
        if constexpr(SPEC)
        {
          const unsigned int plane = SSD_CHK(12, b, kMaxBins) ? SL.plane[b] : 0xffu;
          if constexpr(STRIPS)
          {
            if(plane != 0xffu)
              keys[j] = candidatePoint(p, d, static_cast<int>(plane));
          }
          else
            planes[j] = plane;
        }
      }
      if constexpr(kKeepD)
        dk[j] = d;
    }
    if constexpr(SPEC && !STRIPS)
    {
      /* The points of the candidate bins, behind the tile's other work: one wave-uniform test per TILE skips all of it where no lane
       * holds one - most tiles (ground, risers, background).  A plane number is below 0xff, so the AND of the four is 0xff only
       * if all are.  (The sorted strips' walk - FHD stress: nearly every strip holds some - takes them point by point above: it
       * has no registers for a second loop.) */
      const unsigned int all4 = planes[0] & planes[1] & planes[2] & planes[3];
      SSD_CNT(0, 1);
      SSD_CNT(1, __ballot(all4 != 0xffu) != 0ull ? 1 : 0);
      SSD_CNT_LANES(6, planes[0] != 0xffu); SSD_CNT_LANES(6, planes[1] != 0xffu); SSD_CNT_LANES(6, planes[2] != 0xffu); SSD_CNT_LANES(6, planes[3] != 0xffu);
      /* (timed without the candidates' work, without the window and with a flush that sends no global atomics: profiles/r06_k1_variants.txt (b);
       * the three ablations' code: commit ad9a851) */
      if(__ballot(all4 != 0xffu) != 0ull)
      {
#pragma unroll
        for(int j = 0; j < kPts; j++)
        {
          const int plane = static_cast<int>(planes[j]);
          unsigned int key = kNoPixel;
          if(plane != 0xff)
            key = candidatePoint(v[j], kKeepD ? dk[j] : pre_xy(Q, lc.c3xy, v[j].x, v[j].y, v[j].z), plane);
          keys[j] = key;
        }
        specwin_emit(SL.wins[tid >> 6], missed, win, frameImg, imgWords, X.W64, SL.boxes, keys, lane);
      }
    }
    if constexpr(SPEC && STRIPS)
      specwin_emit(SL.wins[tid >> 6], missed, win, frameImg, imgWords, X.W64, SL.boxes, keys, lane);
    row_reduce_cell(groups, x0, x1, y0, y1);
    if((lane & 15) == 0 && SSD_CHK(15, cellAt, kMaxCellsPerBlock))    /* cell = 64 consecutive points = lanes 16q .. 16q+15 */
      lInfo[cellAt] = make_uint2(groups, cell_box_from_d(Q, x0, x1, y0, y1));
  };
  if constexpr(STRIPS)
  {
    /* Single pass at a width that does not divide a tile (FHD, VGA ..).  Walking the chunk tile by tile, a wave's 256 points
     * would sit in another band of camera columns every tile - its image window would be flushed and re-anchored every tile.
     * So the chunk's strips of 256 points are sorted by (column band of 256 pixels, index) and each wave takes a quarter of
     * the sorted list: it walks down one band, then part of the next.  Sorted by one wave with ballots (<= 128 strips,
     * <= 32 bands).  A strip that crosses the end of a camera row puts its tail into the first band: those pixels miss the
     * window and go to memory one by one - one strip in W / 256. */
    const int nStrips = (end - begin + 255) >> 8;
    if(tid < 64)
    {
      const int sLo = tid, sHi = tid + 64;
      const int bLo = sLo < nStrips ? ((begin + (sLo << 8)) % X.W) >> 8 : -1, bHi = sHi < nStrips ? ((begin + (sHi << 8)) % X.W) >> 8 : -1;
      const int nBands = (X.W + 255) >> 8;
      const unsigned long long below = (1ull << tid) - 1ull;
      int placed = 0;
      for(int b = 0; b < nBands; b++)
      {
        const unsigned long long mLo = __ballot(bLo == b), mHi = __ballot(bHi == b);
        if(bLo == b)
          SL.order[placed + __popcll(mLo & below)] = static_cast<unsigned char>(sLo);
        if(bHi == b)
          SL.order[placed + __popcll(mLo) + __popcll(mHi & below)] = static_cast<unsigned char>(sHi);
        placed += __popcll(mLo) + __popcll(mHi);
      }
    }
    __syncthreads();
    const int wave = tid >> 6;
    int k = wave * nStrips / kWavesPerBlock;
    const int kEnd = (wave + 1) * nStrips / kWavesPerBlock;
    if(k < kEnd)
    {
      /* loads by clamped addresses and the first look at them behind the strip before (first_use): the next strip's loads stay
       * in flight while this one is worked on; only a frame's last strip can reach beyond `end` (block-uniform test) */
      F3 va[kPts], vb[kPts];
      int sa = SL.order[k], sb = 0;
      const int lastStrip = SRC != kSrcDepth16 && ((end - begin) & 255) != 0 ? nStrips - 1 : -1;
      auto issue = [&](const int strip, F3 (&v)[kPts])
      {
        if constexpr(SRC == kSrcDepth16)
          load_points<SRC>(base, begin + (strip << 8) + kPts * lane, end, v, D);         /* deprojected where it is loaded */
        else
          load_points_clamped<SRC>(base, begin + (strip << 8) + kPts * lane, end, v);
      };
      issue(sa, va);
      while(true)
      {
        const bool more = k + 1 < kEnd;
        if(more)
        {
          sb = SL.order[k + 1];
          issue(sb, vb);
        }
        if(sa == lastStrip)
          zero_beyond(va, begin + (sa << 8) + kPts * lane, end);
        tileBody(va, sa * 4 + (lane >> 4));
        if(!more)
          break;
        first_use(vb);
        k++;
        sa = sb;
#pragma unroll
        for(int j = 0; j < kPts; j++)
          va[j] = vb[j];
      }
    }
    nStore = nStrips * (256 / kCell);           /* every strip's four cells were written */
  }
  else if(SRC == kSrcDepth16)
  {
    /* The depth stream: 8 bytes per lane and tile, and the maps.  A tile is 1024 consecutive pixels, so from tile to tile a
     * lane's row advances by 1024 / W and its column by 1024 % W (wrapping once at most): no division in the loop, and when
     * 1024 % W == 0 (XGA: a tile is one image row) the lane's four x-map entries never change - loaded once per block.  The
     * next tile's pixels and map values are requested before the current tile is processed, as the vertex input's tile
     * loop does ("one copy of the body", further down in this function).
     * (Round 3 went through load_points: per tile a division, five dependent map loads, ~90 instructions; K1 on depth input is
     * bound by instruction issue, not by its 2 bytes per point.) */
    const unsigned short *depth = reinterpret_cast<const unsigned short *>(base);
    const int dRow = kTile / D.W, dCol = kTile - dRow * D.W;
    int idx = begin + kPts * tid;
    int row = depth_row(D, idx), col = idx - row * D.W;
    float4 xm = *reinterpret_cast<const float4 *>(D.xmap + col);
    float ym = D.ymap[min(row, D.H - 1)];
    uint2 raw = idx < end ? *reinterpret_cast<const uint2 *>(depth + idx) : make_uint2(0u, 0u);
    while(true)
    {
      const bool more = idx - kPts * tid + kTile < end;                    /* block-uniform */
      uint2 rawN = make_uint2(0u, 0u);
      float4 xmN = xm;
      float ymN = ym;
      if(more)
      {
        idx += kTile;
        row += dRow; col += dCol;
        if(col >= D.W) { col -= D.W; row++; }
        if(idx < end)
          rawN = *reinterpret_cast<const uint2 *>(depth + idx);
        ymN = D.ymap[min(row, D.H - 1)];
        if(dCol != 0)
          xmN = *reinterpret_cast<const float4 *>(D.xmap + col);
      }
      F3 v[kPts];
      deproject4(raw, xm, ym, D.depthUnits, v);
      tileBody(v, it * kCellsPerTile + (tid >> 4));
      it++;
      if(!more)
        break;
      raw = rawN; xm = xmN; ym = ymN;
    }
  }
  else
  {
    auto tileInOrder = [&](const F3 (&v)[kPts])
    {
      tileBody(v, it * kCellsPerTile + (tid >> 4));
      it++;
    };
    /* One copy of the body.  The next tile's loads go out before the current tile is processed and are first looked at behind it
     * (first_use: until round 5's end the compiler waited for them right where they were issued - see load_points_full()), then
     * moved into place: twelve moves per tile.  Tiles wholly inside the chunk take the branch-free loads; a frame that ends in a
     * part of a tile gets that part by load_points().  Measured against two copies taken in turn (two register buffers used
     * alternately, the loop unrolled by two tiles, which keeps only one of its two prefetches in flight: the register allocator
     * copies the other out of the loaded tuples at once; the code: SSD_STREAM_LOOP in commit ad9a851), 1024 XGA frames: single pass
     * 2.06 against 2.18 ms, two passes 1.59 against 1.60. */
    {
      const int fullEnd = begin + (end - begin) / kTile * kTile;
      F3 va[kPts], vb[kPts];
      if(begin < fullEnd)
        load_points_full<SRC>(base, begin + kPts * tid, va);
      for(int i0 = begin; i0 < fullEnd; i0 += kTile)
      {
        const bool more = i0 + kTile < fullEnd;
        if(more)
          load_points_full<SRC>(base, i0 + kTile + kPts * tid, vb);
        tileInOrder(va);
        if(more)
        {
          first_use(vb);
#pragma unroll
          for(int j = 0; j < kPts; j++)
            va[j] = vb[j];
        }
      }
      if(fullEnd < end)
      {
        load_points<SRC>(base, fullEnd + kPts * tid, end, va, D);
        tileInOrder(va);
      }
    }
  }

  if constexpr(SPEC)
  {
    specwin_flush(SL.wins[tid >> 6], win, frameImg, imgWords, X.W64, SL.boxes, lane);
    specmiss_flush(missed, SL.boxes, lane);
    if(curT >= 0 && SSD_CHK(18, curT, kMaxPlanes))
      atomicAdd(&SL.ltot[curT][lane & 7], accT);
  }
  if(lane == 0 && nz)
    atomicAdd(&lNonZero, nz);
  __syncthreads();

  FrameState &fs = st[frame];
  if constexpr(SPEC)
  {
    if(tid < kMaxPlanes)
    {
      unsigned long long t = 0;
#pragma unroll
      for(int k = 0; k < 8; k++)
        t += SL.ltot[tid][k];
      if(t)
        atomicAdd(reinterpret_cast<unsigned long long *>(&fs.planeTotZ[tid]), t);
      if(SL.boxes[tid].yMax >= 0)
      {
        atomicMin(&fs.planeYMin[tid], SL.boxes[tid].yMin); atomicMax(&fs.planeYMax[tid], SL.boxes[tid].yMax);
        atomicMin(&fs.planeXMin[tid], SL.boxes[tid].xMin); atomicMax(&fs.planeXMax[tid], SL.boxes[tid].xMax);
      }
      if(SL.oob[tid])
        atomicAdd(&fs.planeOob[tid], SL.oob[tid]);
    }
  }
  {
    /* the bins' copies summed by all four waves: two threads per bin, half of the copies each in 16-byte reads (taken in an order
     * that changes from bin to bin: the bins' rows lie a whole number of bank cycles apart), the halves joined by one DPP step.
     * (Round 5: one thread per bin and 32 four-byte reads - the work of two waves of the four.) */
    const int b = tid >> 1, half = tid & 1;
    unsigned int s = 0;
    const uint4 *row = reinterpret_cast<const uint4 *>(lh + b * kHistCopies + half * (kHistCopies / 2));
#pragma unroll
    for(int k = 0; k < kHistCopies / 8; k++)
    {
      const uint4 q = row[(k + b) & (kHistCopies / 8 - 1)];
      s += (q.x + q.y) + (q.z + q.w);
    }
    s += static_cast<unsigned int>(__builtin_amdgcn_update_dpp(0, static_cast<int>(s), 0xb1, 0xf, 0xf, false));     /* quad_perm [1, 0, 3, 2]: the neighbour's half */
    if(half == 0 && b < P.nBins && s)
      atomicAdd(&fs.histAcc[b], s);
  }
  if(tid == 0 && lNonZero)
    atomicAdd(&fs.nNonZeroAcc, lNonZero);
  /* the block's cell records, in one burst */
  {
    uint2 *dst = tileMasks + static_cast<size_t>(frame) * tileMaskStride + static_cast<size_t>(begin / kCell);
    const int n = nStore >= 0 ? nStore : it * kCellsPerTile;
    for(int i = tid; i < n; i += kThreads)
      if(SSD_CHK(16, static_cast<size_t>(begin / kCell) + i, tileMaskStride) && SSD_CHK(17, i, kMaxCellsPerBlock))
        dst[i] = lInfo[i];       /* (written past the caches, __builtin_nontemporal_store: no cure, profiles/r06_box_spread.txt; K2 +0.12 ms, docs/HISTORY.md; the code: commit ad9a851) */
  }
}

/* blocks per SIMD that K1's single-pass entry point, k_hist_planes, is built for */
#ifndef SSD_K1S_WAVES
#define SSD_K1S_WAVES 5
#endif

/* K0 of a single-pass batch: which height bins may belong to a step plateau?  A histogram of a sample of the frame (vertex input: one
 * whole 128-byte line of every fifteen, at a place in its group that changes from group to group - ssd_predict.h; depth input: one run
 * of 16 pixels of every sixteen), the reference's peak filter (pointcloud.cpp:243-256) on it with
 * slack, a plane for each candidate peak's bin and its two neighbours (the plateau takes the peak bin and the fuller
 * neighbour: only the complete histogram decides which).  Nothing here has to be right: k_peaks checks the planes against the
 * plateaus it finds in the complete histogram, and a frame whose plateaus are not covered is rastered by k_raster.
 * Grid (frame, part): the blocks of a frame add their counts into FrameState::predHist; the last one to finish makes the table
 * and leaves the accumulators zero.  sabotage (tests): 1 = planes three bins above the right ones, 2 = no planes.
 * CHECKS: the pre-filter's tests of the rare configurations, as K1's (vertex input; the depth loop asks the doubles about every point). */
template<int SRC, bool CHECKS>
__device__ __forceinline__ void predict_block(const float *__restrict__ xyz, size_t strideFloats, const PointParams &P, const PreXY &Q,
                                              FrameState *__restrict__ st, const DepthSrc &D, int minHeight, int sabotage, int *__restrict__ fallback, int poolPlanes)
{
  __shared__ unsigned int sh[kMaxBins + 2];
  alignas(16) __shared__ unsigned int shc[kMaxBins * kHistCopies];        /* [bin][copy], as K1's: the lanes of a wave mostly vote for ONE bin */
  __shared__ K1Consts kc;                                                 /* vertex input: the doubles' constants, as K1 keeps them */
  __shared__ int sLast;
  const int frame = blockIdx.x, part = blockIdx.y, nParts = gridDim.y, tid = threadIdx.x;
  const float *base = SRC == kSrcDepth16
    ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(xyz) + static_cast<size_t>(frame) * strideFloats)
    : xyz + static_cast<size_t>(frame) * strideFloats;
  if(tid < kMaxBins + 2)
    sh[tid] = 0u;
  for(int i = tid; i < kMaxBins * kHistCopies / 4; i += kThreads)
    reinterpret_cast<uint4 *>(shc)[i] = make_uint4(0u, 0u, 0u, 0u);
  if(SRC != kSrcDepth16 && tid == 0)
    k1_consts_fill(kc, P, nullptr);
  __syncthreads();
  unsigned int *mine = shc + (tid & (kHistCopies - 1));
  if constexpr(SRC != kSrcDepth16)
  {
    /* The sample: whole 128-byte lines (ssd_predict.h).  One point per lane by a 12-byte load, ten lanes to a line, six lines to a
     * wave instruction (four lanes idle); a block takes 24 groups per step, the frame's blocks take turns.  A lane requests the points
     * of four steps before it looks at the first (a single dependent read pays the whole way to HBM; at most 24 lines per wave, 768 per
     * CU where eight blocks are resident - the residency is not measured): addresses clamped into the frame, no branch between the loads and their use; a lane without a point -
     * a line cut by the frame's ends, a group beyond the last - reads the frame's last point and blanks it (z = 0: no measurement).
     * The four are requested and counted within one trip of the loop: carried round it in registers, the compiler moves the loaded
     * y and z at the loop's head (pre_xy's packed FMAs want y in an even register) behind a wait for every load in flight.
     * The decisions are K1's: single precision first (pre_range), the band it cannot call through the reference's doubles by the
     * whole wave - the count is exact.  The price: 54 vector registers where the round-4 loop had 40 (still eight waves a SIMD), and
     * four lanes in 64 that issue for nothing. */
    constexpr int kLines = 64 / kPredictLinePoints, kDepth = 4;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slot = lane / kPredictLinePoints, k = lane - slot * kPredictLinePoints;
    const bool live = slot < kLines;
    const int step = nParts * (kThreads / 64) * kLines;
    const int gWave = (part * (kThreads / 64) + wave) * kLines;                  /* the wave's first group: wave-uniform, the loop's bound */
    const unsigned long long addr = reinterpret_cast<unsigned long long>(base);
    const int nGroups = predict_sample_groups(addr, P.nPoints);
    const PreLane lc(Q);
    for(int s = 0; gWave + s * step < nGroups; s += kDepth)
    {
      F3 v[kDepth];
      bool has[kDepth];
#pragma unroll
      for(int d = 0; d < kDepth; d++)
      {
        const PredictRun r = predict_sample_run(addr, P.nPoints, gWave + slot + (s + d) * step);
        has[d] = live & (k < r.count);
        v[d] = *reinterpret_cast<const F3 *>(base + 3 * static_cast<size_t>(min(r.first + k, P.nPoints - 1)));
      }
#pragma unroll
      for(int d = 0; d < kDepth; d++)
      {
        const F3 p{ v[d].x, v[d].y, has[d] ? v[d].z : 0.0f };
        const PreRange r = pre_range<CHECKS, false>(p, Q, lc);
        unsigned int b = r.b;
        unsigned long long mIn = r.mInSure;
        if(r.mSlow != 0ull)
        {
          /* rare, wave-uniform: the reference's rows, compares and bin (hist_block) */
          const K1ConstsLds c = k1_consts(kc);
          const World3 w = world_rows(c, p);
          mIn |= r.mSlow & __ballot(world_in_range(c, w));
          b = __builtin_amdgcn_inverse_ballot_w64(r.mSlow) ? static_cast<unsigned int>(world_bin(c, w)) : b;
        }
        if(__builtin_amdgcn_inverse_ballot_w64(mIn))
          if(SSD_CHK(32, b, P.nBins))
            atomicAdd(mine + b * kHistCopies, 1u);
      }
    }
  }
  else
  {
    /* depth input (not the product's path: it keeps two passes there): runs of 16 consecutive pixels (four lanes' loads), one of every
     * kSpecSample runs, at a place in its group of runs that changes from group to group.  (Whole cells of 64 points were tried first:
     * neighbouring pixels share a height bin, so a bin's count is really a count of runs - with 64-point runs a background bin's 150
     * samples were five runs and one bin in six passed the peak filter by chance.) */
#ifndef SSD_K0_RUN
#define SSD_K0_RUN 16
#endif
    constexpr int kRun = SSD_K0_RUN, kLanesPerRun = kRun / kPts;
    const int nRuns = (P.nPoints + kRun - 1) / kRun;
    const int nGroups = (nRuns + kSpecSample - 1) / kSpecSample;
    for(int g = part * (kThreads / kLanesPerRun) + tid / kLanesPerRun; g < nGroups; g += nParts * (kThreads / kLanesPerRun))
    {
      const int run = g * kSpecSample + ((g * 5) & (kSpecSample - 1));
      F3 v[kPts];
      load_points<SRC>(base, run * kRun + kPts * (tid % kLanesPerRun), P.nPoints, v, D);
#pragma unroll
      for(int j = 0; j < kPts; j++)
      {
        double wx, wy, wz;
        if(world_point_flat(P, v[j], wx, wy, wz))
          atomicAdd(mine + height_bin(P, wz) * kHistCopies, 1u);
      }
    }
  }
  __syncthreads();
  FrameState &fs = st[frame];
  if(tid < P.nBins)
  {
    unsigned int c = 0;
#pragma unroll
    for(int k = 0; k < kHistCopies; k++)
      c += shc[tid * kHistCopies + ((k + tid) & (kHistCopies - 1))];      /* rotated: conflict-free */
    /* The adds are taken WITH their results: a thread that holds the old value knows its add has been performed (device-scope
     * atomics act on the memory side, as does the exchange that reads the sums below), so after the barrier the block's
     * share is in place and its ticket may be drawn - without a __threadfence(), which on this part writes the whole L2
     * back: with two of them per block this kernel took 1.0 ms instead of 0.1. */
    if(c)
    {
      const unsigned int before = atomicAdd(&fs.predHist[tid], c);
      asm volatile("" :: "v"(before));
    }
  }
  __syncthreads();
  /* (Relaxed atomics throughout: the hand-over rests on returning device-scope atomics being performed at the memory side of
   * THIS part - gfx950, one L2 per XCD in front of the fabric's atomics -, not on the HIP memory model.  The build is pinned
   * to that part below, and the kernel's table is held against ssd_predict.h on every frame of four batches in the default
   * GPU tier: tests/test_gpu_single_pass.py::test_the_kernels_table_is_the_host_statements.  A table that differed would
   * cost the frame its planes - k_peaks checks them and k_raster steps in -, never a result.) */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_predict's hand-over between blocks is written for gfx950 (see the comment above)"
#endif
  if(tid == 0)
    sLast = atomicAdd(&fs.predDone, 1u) == static_cast<unsigned int>(nParts - 1) ? 1 : 0;
  __syncthreads();
  if(!sLast)
    return;
  /* the frame's sample is complete: sh[1 + bin] (a zero either side) */
  const unsigned int mineCount = tid < P.nBins ? atomicExch(&fs.predHist[tid], 0u) : 0u;
  __syncthreads();
  if(tid < kMaxBins)
  {
    sh[1 + tid] = mineCount;
    fs.predSample[tid] = mineCount;
  }
  if(tid == 0)
    sh[0] = sh[kMaxBins + 1] = 0u;
  __syncthreads();
  /* (the table as a plain function of the sample: ssd_predict.h - the tests hold this kernel's table against it) */
  /* candidate peak: filterPeaks' two conditions (>= 2000 points; twice the count exceeds the neighbours' sum by more than
   * half the count) on the sample: from 1200 points scaled up, the sharpness as it is plus a few samples.  (A tread stands
   * far above both thresholds.  Looser - the neighbours' sum below 1.75 counts - and a flat background of a few thousand
   * points per bin, a wall behind the stairs, passes in every sixth of its bins on sampling noise alone: more candidates
   * than planes.) */
  auto candidate = [&](int b) -> bool
  {
    if(b < max(minHeight, 1) || b >= P.nBins - 1)
      return false;
    const unsigned int c = sh[1 + b], l = sh[b], r = sh[2 + b];
    return c > l && c >= r && c * kSpecSample >= 1200u && (l + r) * 2u < 3u * c + 16u;     /* a local maximum: of a tread's two almost equally full bins, one */
  };
  /* at most kMaxPlanes / 3 candidates: the fullest ones (a sampled background still throws up a false peak here and there;
   * they cost planes and stray raster work, never results) */
  __shared__ unsigned int sCand[kMaxBins];
  const bool cand = tid < kMaxBins && sabotage != 2 && candidate(tid);
  /* The plateau is the peak's bin and the fuller of its neighbours (extractPlateauPoints, pointcloud.cpp:300-335; the upper
   * one on a tie).  Where the sample leaves no doubt which - one neighbour more than twice the other - the other gets no
   * plane: it holds no tread, only what lies at that height elsewhere in the image, points that would miss the windows. */
  unsigned int code = 0u;
  if(cand)
  {
    const unsigned int l = sh[tid], r = sh[2 + tid];
    code = 1u | (r > 2u * l + 8u ? 0u : 2u) | (l > 2u * r + 8u ? 0u : 4u);        /* chosen | lower neighbour | upper neighbour */
  }
  if(tid < kMaxBins)
    sCand[tid] = cand ? sh[1 + tid] : 0u;
  __syncthreads();
  if(tid < kMaxBins)
  {
    int fuller = 0;
    if(cand)
      for(int b = 0; b < kMaxBins; b++)
        fuller += (sCand[b] > sCand[tid] || (sCand[b] == sCand[tid] && b < tid)) ? 1 : 0;
    sh[1 + tid] = cand && fuller < kMaxPlanes / 3 ? code : 0u;        /* the table of chosen peaks, zeros either side as before */
  }
  __syncthreads();
  /* Bins to planes.  A peak whose fuller neighbour is beyond doubt shares ONE plane with it - the plateau's image as k_raster
   * would make it, the tread's pixels in one window however the range noise deals its points to the two bins; a peak with
   * neighbours too alike to call gets three planes (its own holds the tread; k_outline reads it together with the
   * neighbour k_peaks picks).  code(k): the chosen-peak code of bin k (0: none), shifted by the sabotage. */
  const int shift = sabotage == 1 ? 3 : 0;
  auto code_of = [&](int k) -> unsigned int
  {
    k -= shift;
    return k >= 0 && k < kMaxBins ? sh[1 + k] : 0u;
  };
  bool want = false, start = false;
  if(tid < kMaxBins)
  {
    auto wanted = [&](int k) { return k >= 0 && k < P.nBins && ((code_of(k - 1) & 4u) | (code_of(k) & 1u) | (code_of(k + 1) & 2u)) != 0u; };
    want = wanted(tid);
    /* shares the plane of the bin below: the upper neighbour of a peak sure of it, or a peak sure of its lower neighbour */
    const bool withBelow = want && wanted(tid - 1) && (code_of(tid - 1) == 5u || code_of(tid) == 3u);
    start = want && !withBelow;
  }
  __shared__ unsigned long long sStart[2];
  if(tid < 2 * 64)
  {
    const unsigned long long m = __ballot(start);
    if((tid & 63) == 0)
      sStart[tid >> 6] = m;
  }
  __syncthreads();
  const int total = __popcll(sStart[0]) + __popcll(sStart[1]);
  /* the frame's planes out of the workspace's pool: one returning add on the batch's counter (fallback[2]; k_peaks of this batch
   * leaves it zero again).  A frame the pool cannot serve - more candidates per frame than kPoolPlanesPerFrame over a whole
   * batch - gets no planes: k_peaks will find its plateaus uncovered and k_raster does it. */
  __shared__ int sBase;
  if(tid == 0)
  {
    int base = -1;
    if(total > 0 && total <= kMaxPlanes)
    {
      base = atomicAdd(&fallback[2], total);
      if(base + total > poolPlanes)
        base = -1;
    }
    sBase = base;
  }
  __syncthreads();
  const bool fits = sBase >= 0;
  if(tid < kMaxBins)
  {
    /* plane = starts at or below this bin, minus one */
    const unsigned long long upTo = tid < 64 ? (2ull << tid) - 1ull : ~0ull;
    const int n = tid < 64 ? __popcll(sStart[0] & upTo) : __popcll(sStart[0]) + __popcll(sStart[1] & ((2ull << (tid - 64)) - 1ull));
    fs.specPlane[tid] = (want && fits) ? static_cast<unsigned char>(n - 1) : static_cast<unsigned char>(0xff);
  }
  if(tid < kMaxPlanes)
  {
    fs.planeYMin[tid] = 0x7fffffff; fs.planeYMax[tid] = -1;
    fs.planeXMin[tid] = 0x7fffffff; fs.planeXMax[tid] = -1;
    fs.planeTotZ[tid] = 0;
    fs.planeOob[tid] = 0u;
    fs.planeUsed[tid] = 0;
  }
  if(tid == 0)
  {
    fs.nPlanes = fits ? total : 0;
    fs.planeBase = fits ? sBase : 0;
    fs.predDone = 0u;
    if(frame == 0)
    {
      fallback[0] = 0;                   /* k_raster's work list of this batch starts empty (k_peaks appends) */
      fallback[1] = 0;                   /* frames without step plateaus (k_peaks counts) */
    }
  }
}

/* ========================================================================= */
/* K1b: peaks, plateaus, LUT — one thread per frame (121 bins: trivial)        */

/* one wave per frame: the histogram is staged in LDS, lane 0 walks it (the peak / plateau logic is a
 * sequential scan with carried state), all lanes write the tables out */
SSD_ENTRY(__launch_bounds__(64), k_peaks, peaks_block)(SSD_BYVAL(Params) P, FrameState *__restrict__ st, int nframes, DebugFrame *__restrict__ dbg, int spec, int *__restrict__ fallback)
{
  __shared__ unsigned char sImgPlane[kMaxStepImages][2];
  __shared__ unsigned int sCovered;
  __shared__ unsigned int hist[kMaxBins + 1];
  __shared__ unsigned char lut[kMaxBins];
  __shared__ int plPeak[kMaxPlateaus], plLo[kMaxPlateaus], plHi[kMaxPlateaus], plEffLo[kMaxPlateaus], plEffHi[kMaxPlateaus], plN[kMaxPlateaus];
  __shared__ int dbgPeaks[kMaxPlateaus];
  __shared__ int sNPl, sNPeaks, sOverflow, sGround, sFirstStep, sNImg;

  const int frame = blockIdx.x, lane = threadIdx.x;
  if(frame >= nframes)
    return;
  FrameState &fs = st[frame];
  const int nb = P.nBins;

  unsigned int total = 0;
  for(int b = lane; b <= kMaxBins; b += 64)
  {
    /* K1's accumulator is taken over and left zero for the next call (FrameState::histAcc) */
    const unsigned int v = b < nb ? fs.histAcc[b] : 0u;
    hist[b] = v;
    total += v;
    if(b < kMaxBins)
    {
      lut[b] = 0xff;
      fs.hist[b] = v;
      if(b < nb)
        fs.histAcc[b] = 0u;
    }
  }
#pragma unroll
  for(int o = 32; o > 0; o >>= 1)
    total += __shfl_xor(total, o);
  __syncthreads();

  /* findPeaks (pointcloud.cpp:214-241) + filterPeaks (:243-256), all lanes: lane l looks at bins l and l + 64.  The
   * reference walks the bins with one carried flag: a bin is a peak when the count falls after it and the last CHANGE
   * before it was a rise (so a flat top reports its last index, quirk Q1).  Here: rise / fall bits of all bins by two
   * ballots each, then "the highest changed bin below me is a rise" by bit scans. */
  unsigned long long peakBits[2];
  {
    unsigned long long up[2], down[2];
#pragma unroll
    for(int w = 0; w < 2; w++)
    {
      const int i = lane + 64 * w;
      const bool inRange = i < nb - 1;
      const unsigned int c = hist[min(i, kMaxBins - 1)], succ = hist[min(i + 1, kMaxBins)];
      up[w] = __ballot(inRange && c < succ);
      down[w] = __ballot(inRange && c > succ);
    }
    const unsigned long long changed[2] = { up[0] | down[0], up[1] | down[1] };
#pragma unroll
    for(int w = 0; w < 2; w++)
    {
      const int i = lane + 64 * w;
      bool peak = false;
      if((down[w] >> lane) & 1ull)
      {
        const unsigned long long below = changed[w] & ((1ull << lane) - 1ull);
        bool lastWasRise = false;
        if(below)
          lastWasRise = (up[w] >> (63 - __clzll(static_cast<long long>(below)))) & 1ull;
        else if(w == 1 && changed[0])
          lastWasRise = (up[0] >> (63 - __clzll(static_cast<long long>(changed[0])))) & 1ull;
        if(lastWasRise)
        {
          const unsigned int np = hist[i];
          peak = np >= 2000u && (np * 2u - hist[i - 1] - hist[i + 1]) * 2u > np;     /* filterPeaks; i >= 1 after a rise */
        }
      }
      peakBits[w] = __ballot(peak);
    }
  }

  if(lane == 0)
  {
    int nPl = 0;
    int consumedUpTo = -1;           /* every bin <= this has already left pointsHt */
    bool overflow = false;
    int nPeaksDbg = 0;
    for(int w = 0; w < 2; w++)
      for(unsigned long long bits = peakBits[w]; bits; bits &= bits - 1ull)
      {
        const int i = 64 * w + __ffsll(static_cast<long long>(bits)) - 1;
        const unsigned int succ = hist[i + 1];
        if(nPeaksDbg < kMaxPlateaus)
          dbgPeaks[nPeaksDbg] = i;
        nPeaksDbg++;
        if(nPl >= kMaxPlateaus)
          overflow = true;
        else
        {
          /* extractPlateauPoints (:300-335): choose the pair, then take what is left of it */
          int hMin, hMax;
          if(hist[i - 1] > succ) { hMin = i - 1; hMax = i; }
          else { hMin = i; hMax = i + 1; }
          int lo, hi;
          if(hMin == 0)
          {
            /* quirk Q4: Height_t(heightMin - 1) wraps to 65535: everything goes to the remainder */
            lo = 1; hi = 0;
            consumedUpTo = nb;
          }
          else
          {
            lo = max(hMin, consumedUpTo + 1);
            hi = hMax;
            consumedUpTo = max(consumedUpTo, hMax);
          }
          unsigned int cnt = 0;
          for(int b = lo; b <= hi; b++)
          {
            cnt += hist[b];
            lut[b] = static_cast<unsigned char>(nPl);
          }
          plPeak[nPl] = i; plLo[nPl] = hMin; plHi[nPl] = hMax; plEffLo[nPl] = lo; plEffHi[nPl] = hi;
          plN[nPl] = static_cast<int>(cnt);
          nPl++;
        }
      }

    /* ground = most populous plateau below minHeight (pointcloud.cpp:402-418) */
    int groundInd = -1, i = 0;
    unsigned int maxGround = 0;
    for( ; i < nPl; i++)
    {
      if(plPeak[i] >= P.minHeight)
        break;
      if(maxGround < static_cast<unsigned int>(plN[i]))
      {
        maxGround = static_cast<unsigned int>(plN[i]);
        groundInd = i;
      }
    }
    int nImg = nPl - i;
    if(nImg > P.maxStepImages)
    {
      nImg = P.maxStepImages;
      overflow = true;
    }
    sNPl = nPl; sNPeaks = nPeaksDbg; sOverflow = overflow ? 1 : 0; sGround = groundInd; sFirstStep = i; sNImg = nImg;

    /* single pass: did k_predict give every bin of a step plateau a plane?  (A bin without points needs none.)  Plateau by
     * plateau: the covered ones are read from their planes, k_raster does the others of the frame (typically a weak last
     * peak at the top of the range that the sample did not show). */
    unsigned int covered = 0u;
    for(int slot = 0; spec && slot < nImg; slot++)
    {
      bool ok = spec != 0;
      unsigned char a = 0xff, b2 = 0xff;
      const int lo = plEffLo[i + slot], hi = plEffHi[i + slot];
      for(int b = lo; b <= hi; b++)                                        /* two bins at most */
      {
        const unsigned char p = spec ? fs.specPlane[b] : static_cast<unsigned char>(0xff);
        if(p == 0xff)
          ok = ok && hist[b] == 0u;
        else if(a == 0xff)
          a = p;
        else if(p != a)
          b2 = p;
      }
      /* a plane may hold two bins (k_predict): it must not bring points of a bin outside the plateau */
      if(spec && lo <= hi)
      {
        if(lo > 0 && fs.specPlane[lo - 1] != 0xff && (fs.specPlane[lo - 1] == a || fs.specPlane[lo - 1] == b2))
          ok = ok && hist[lo - 1] == 0u;
        if(hi + 1 < nb && fs.specPlane[hi + 1] != 0xff && (fs.specPlane[hi + 1] == a || fs.specPlane[hi + 1] == b2))
          ok = ok && hist[hi + 1] == 0u;
      }
      sImgPlane[slot][0] = a; sImgPlane[slot][1] = b2;
      covered |= ok ? 1u << slot : 0u;
    }
    sCovered = covered;
  }
  __syncthreads();

  const int nPl = sNPl, firstStep = sFirstStep, nImg = sNImg;
  unsigned int wanted = 0u;
  for(int b = lane; b < kMaxBins; b += 64)
  {
    const unsigned char l = lut[b];
    fs.lut[b] = l;
    const int slot = static_cast<int>(l) - firstStep;
    if(b < nb && l != 0xff && slot >= 0 && slot < nImg && !((sCovered >> slot) & 1u))      /* k_raster's gate: the plateaus it has to do */
      wanted |= 1u << (b / kBinsPerGroup);
  }
#pragma unroll
  for(int o = 32; o > 0; o >>= 1)
    wanted |= __shfl_xor(wanted, o);
  if(lane < nPl)
  {
    PlateauState &pl = fs.pl[lane];
    pl.peakBin = plPeak[lane];
    pl.binLo = plLo[lane];
    pl.binHi = plHi[lane];
    pl.effLo = plEffLo[lane];
    pl.effHi = plEffHi[lane];
    pl.nPoints = plN[lane];
    pl.isStep = plPeak[lane] >= P.minHeight ? 1 : 0;
    pl.outlineFound = 0;
    pl.valid = 0;
    for(int k = 0; k < 8; k++) { pl.quadImg[k] = 0.0; pl.quadWorld[k] = 0.0; }
  }
  /* The step images' boxes and z sums: empty / zero for k_raster to fill, or - single pass, every plateau covered - what
   * k_hist found in the planes of the plateau's bins (k_outline merges those planes into the image). */
  const unsigned int covered = sCovered;
  const bool specOk = nImg > 0 && covered == (nImg >= 32 ? 0xffffffffu : (1u << nImg) - 1u);
  unsigned int oobSum = 0u;
  if(lane <= kMaxStepImages)                          /* [kMaxStepImages] = the ground image */
  {
    int y0 = 0x7fffffff, y1 = -1, x0 = 0x7fffffff, x1 = -1;
    long long tz = 0;
    const bool mine = lane < nImg && ((covered >> lane) & 1u) != 0u;
    if(mine)
    {
#pragma unroll
      for(int k = 0; k < 2; k++)
      {
        const int p = sImgPlane[lane][k];
        if(p == 0xff)
          continue;
        if(fs.planeYMax[p] >= fs.planeYMin[p])
        {
          y0 = min(y0, fs.planeYMin[p]); y1 = max(y1, fs.planeYMax[p]);
          x0 = min(x0, fs.planeXMin[p]); x1 = max(x1, fs.planeXMax[p]);
        }
        tz += fs.planeTotZ[p];
        oobSum += fs.planeOob[p];
      }
      /* the planes hold sums of the bits of (z + 6144) over exactly the plateau's points (covered: every bin of it with
       * points has a plane, and no plane of it a point of another bin): minus the constant's bits per point, modulo 2^64,
       * this is the sum of round(z * 2^40) k_raster would have left (z_plus_magic_bits) */
      tz = static_cast<long long>(static_cast<unsigned long long>(tz) - static_cast<unsigned long long>(kMagicBits) * static_cast<unsigned long long>(plN[firstStep + lane]));
    }
    fs.imgYMin[lane] = y0; fs.imgYMax[lane] = y1;
    fs.imgXMin[lane] = x0; fs.imgXMax[lane] = x1;
    if(lane < kMaxStepImages)
    {
      fs.totZ[lane] = tz;                              /* k_raster's sums start from zero */
      fs.imgPlane[lane][0] = mine ? sImgPlane[lane][0] : static_cast<unsigned char>(0xff);
      fs.imgPlane[lane][1] = mine ? sImgPlane[lane][1] : static_cast<unsigned char>(0xff);
    }
  }
#pragma unroll
  for(int o = 32; o > 0; o >>= 1)
    oobSum += __shfl_xor(oobSum, o);
  if(spec && lane < kMaxPlanes)
  {
    bool used = false;
    for(int sl = 0; sl < nImg; sl++)
      used = used || (((covered >> sl) & 1u) != 0u && (sImgPlane[sl][0] == lane || sImgPlane[sl][1] == lane));
    fs.planeUsed[lane] = used ? 1 : 0;
  }
  if(lane == 0)
  {
    if(spec && !specOk && nImg > 0)
    {
      const int at = atomicAdd(&fallback[0], 1);
      if(SSD_CHK(25, at, nframes))
        fallback[kFallbackList + at] = frame;          /* k_raster's work list (k_predict zeroed the count) */
    }
    if(spec && frame == 0)
      fallback[2] = 0;                                                       /* the plane pool's counter: every k_predict block of this batch is long done */
    if(spec && nImg == 0)
      atomicAdd(&fallback[1], 1);                                            /* frames WITHOUT a step plateau (the rare kind where stairs are in sight: a thousand adds to one address cost k_peaks 10 us): what the single pass cannot gain on, ssd_fetch_back */
    fs.specOk = specOk ? 1 : 0;
    fs.slotCovered = covered;
    fs.nNonZero = fs.nNonZeroAcc;
    fs.nNonZeroAcc = 0u;
    fs.nOob = oobSum;
    fs.status = (sOverflow ? static_cast<unsigned int>(SSD_ST_OVERFLOW) : 0u) | (oobSum ? static_cast<unsigned int>(SSD_ST_OOB_PIXEL) : 0u);     /* the frame's status starts here */
    fs.nInRange = total;
    fs.nPlateaus = nPl;
    fs.groundInd = sGround;
    fs.firstStep = firstStep;
    fs.nStepImages = nImg;
    fs.firstValidInd = -1;
    fs.wantedSteps = wanted;
    fs.wantedQuads = 0u;
    fs.anyActive = 0u;
  }

  if(dbg)
  {
    ssd_debug_frame &d = dbg[frame].d;
    for(int b = lane; b < kMaxBins; b += 64)
      d.hist[b] = hist[b];
    if(lane < min(sNPeaks, kMaxPlateaus))
      d.peaks[lane] = dbgPeaks[lane];
    if(lane < nPl)
    {
      ssd_debug_plateau &p = d.plateaus[lane];
      p.peak_bin = plPeak[lane]; p.bin_lo = plLo[lane]; p.bin_hi = plHi[lane];
      p.eff_lo = plEffLo[lane]; p.eff_hi = plEffHi[lane];
      p.n_points = plN[lane];
      p.is_step = plPeak[lane] >= P.minHeight ? 1 : 0;
    }
    if(lane == 0)
    {
      d.n_nonzero = static_cast<int>(fs.nNonZero);
      d.n_inrange = static_cast<int>(total);
      d.n_bins = nb;
      d.min_height = P.minHeight;
      d.min_img_y_extent = P.minImgYExtent;
      d.n_peaks = sNPeaks;
      d.n_plateaus = nPl;
      d.first_step = firstStep;
      d.ground_ind = sGround;
    }
  }
}

/* ========================================================================= */
/* K2: raster the step plateaus into bit images                               */

struct RasterLds
{
  unsigned long long wins[kThreads / 64][kWinWords];
  unsigned int wmiss[kThreads / 64][kWaveMissWords];
  ImageBox boxes[kMaxStepImages];
  unsigned char lut[kMaxBins];
  unsigned int lOob;
  unsigned short cellList[kMaxCellsPerBlockRaster];
  unsigned int listScratch[2 * kWavesPerBlock];
  unsigned long long ltot[kMaxStepImages][8];       /* sum of round(z * 2^40) over ALL points of each step plateau (this block's share) */
};

template<int SRC>
__device__ __forceinline__ void raster_block(RasterLds &L, const float *__restrict__ xyz, size_t strideFloats, const PointParams &P,
                                             const PixelParams &X, FrameState *__restrict__ st,
                                             unsigned long long *__restrict__ stepImg,
                                             const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints, const DepthSrc &D,
                                             const int frame, const int chunkIdx)
{
  unsigned long long (&wins)[kThreads / 64][kWinWords] = L.wins;
  unsigned int (&wmiss)[kThreads / 64][kWaveMissWords] = L.wmiss;
  ImageBox (&boxes)[kMaxStepImages] = L.boxes;
  unsigned char (&lut)[kMaxBins] = L.lut;
  unsigned int &lOob = L.lOob;
  unsigned short (&cellList)[kMaxCellsPerBlockRaster] = L.cellList;
  unsigned int (&listScratch)[2 * kWavesPerBlock] = L.listScratch;
  unsigned long long (&ltot)[kMaxStepImages][8] = L.ltot;

  const int tid = threadIdx.x, lane = tid & 63;
  FrameState &fs = st[frame];
  /* all the block needs of the frame's state in one memory round trip (the image count decides whether there is work) */
  const int nImg = fs.nStepImages;
  const int firstStep = fs.firstStep;
  const unsigned char lutMine = tid < kMaxBins ? fs.lut[tid] : static_cast<unsigned char>(0xff);
  const unsigned int wantedSteps = fs.wantedSteps;
  const unsigned int slotCovered = fs.slotCovered;        /* single pass: plateaus k_hist has rastered already (k_peaks; 0 otherwise) */
  if(nImg == 0 || wantedSteps == 0u)
    return;
  BlockPhase ph(0);
  if(tid < kMaxBins)
  {
    /* bin -> image slot of a step plateau, 0xff = no image for this bin */
    const int sl = static_cast<int>(lutMine) - firstStep;
    lut[tid] = (lutMine != 0xff && sl >= 0 && sl < nImg && !((slotCovered >> sl) & 1u)) ? static_cast<unsigned char>(sl) : static_cast<unsigned char>(0xff);
  }
  if(tid < kMaxStepImages)
    boxes[tid] = ImageBox{ 0x7fffffff, -1, 0x7fffffff, -1 };
  if(tid < kMaxStepImages * 8)
    (&ltot[0][0])[tid] = 0ull;
  if(tid == 0)
    lOob = 0;
  for(int i = tid; i < (kThreads / 64) * kWinWords; i += kThreads)
    (&wins[0][0])[i] = 0ull;
  if(tid < kThreads / 64)
    wavemiss_init(wmiss[tid]);
  __syncthreads();
  ph.mark(0);

  /* strideFloats counts floats, or 16-bit depth values for kSrcDepth16 */
  const float *base = SRC == kSrcDepth16
    ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(xyz) + static_cast<size_t>(frame) * strideFloats)
    : xyz + static_cast<size_t>(frame) * strideFloats;
  const int begin = chunkIdx * chunkPoints;
  const int end = min(begin + chunkPoints, P.nPoints);
  const unsigned int imgWords = static_cast<unsigned int>(X.H) * X.W64;
  unsigned long long *frameImg = stepImg + static_cast<size_t>(frame) * X.maxStepImages * imgWords;
  unsigned long long *ww = wins[tid >> 6];
  unsigned int *wm = wmiss[tid >> 6];
  WaveWindow win;
  win.limitWords = static_cast<unsigned int>(X.maxStepImages) * imgWords;
  unsigned int oob = 0;
  /* The z sum of EVERY point of each step plateau, in and out of its outline (the count is the histogram's): k_inquad
   * then only has to visit the cells that can hold points OUTSIDE the quadrilateral and take those off again.  A lane
   * walks down a camera column, so its hits nearly always stay on one plateau: running sum in registers. */
  int curT = -1;
  unsigned long long accT = 0;
  auto flushT = [&]()
  {
    if(curT >= 0)
      atomicAdd(&ltot[curT][lane & 7], accT);
  };

  /* Only the cells that hold a bin of a step plateau are walked (cell_list_build), four per wave iteration, with the
   * loads of the NEXT group issued before the current one is processed: a wave that waits for its own loads each
   * iteration leaves the SIMD to seven others, which no longer cover the memory latency once the body is this short. */
  const int cell0 = begin / kCell;
  const int nCells = (end - begin + kCell - 1) / kCell;
  const int count = cell_list_build(tileMasks + static_cast<size_t>(frame) * tileMaskStride + cell0, nCells, X.cellCols,
                                    [&](const uint2 info) { return (info.x & wantedSteps) != 0u; }, cellList, listScratch);
  ph.mark(1);
  const int nGroups = (count + 3) >> 2;
  int g = (tid >> 6) * nGroups / kWavesPerBlock;
  const int gEnd = ((tid >> 6) + 1) * nGroups / kWavesPerBlock;
  if(g < gEnd)
  {
    F3 v[kPts], vn[kPts];
    load_cell<SRC>(base, cell0, cellList, 4 * g + (lane >> 4), count, lane, P.nPoints, v, D);
    while(true)
    {
    const bool more = g + 1 < gEnd;
    if(more)
      load_cell<SRC>(base, cell0, cellList, 4 * (g + 1) + (lane >> 4), count, lane, P.nPoints, vn, D);
    unsigned int key[kPts];
    #pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      /* few, flat decisions per point (see k_inquad) */
      key[j] = kNoPixel;
      double wx, wy, wz;
      const bool ok = world_point_flat(P, v[j], wx, wy, wz);
      const int bin = ok ? height_bin(P, wz) : 0;
      const int slot = SSD_CHK(30, bin, kMaxBins) ? lut[bin] : 0xff;
      if(!(ok & (slot != 0xff)))
        continue;
      int ix, iy;
      const bool inside = image_pixel(P, X, wx, wy, ix, iy);
      if(slot != curT)
      {
        flushT();
        curT = SSD_CHK(31, slot, kMaxStepImages) ? slot : -1;
        accT = 0;
      }
      accT += static_cast<unsigned long long>(z_to_fixed(wz));
      oob += inside ? 0u : 1u;                                /* quirk Q5 */
      key[j] = inside ? pixel_key(slot, iy, ix) : kNoPixel;
    }
    wavewin_emit(ww, wm, win, frameImg, imgWords, X.W64, X.winShift, boxes, key, lane);
    if(!more)
      break;
    g++;
#pragma unroll
    for(int j = 0; j < kPts; j++)
      v[j] = vn[j];
    }
  }
  ph.mark(2);
  wavewin_flush(ww, win, frameImg, imgWords, X.W64, X.winShift, boxes, lane);
  wavemiss_flush(wm, boxes, lane);
  flushT();
  if(oob)
    atomicAdd(&lOob, oob);
  ph.mark(5);
  __syncthreads();
  ph.mark(3);
  if(tid < nImg)
  {
    unsigned long long t = 0;
#pragma unroll
    for(int k = 0; k < 8; k++)
      t += ltot[tid][k];
    if(t)
      atomicAdd(reinterpret_cast<unsigned long long *>(&fs.totZ[tid]), t);
  }
  if(tid < nImg && boxes[tid].yMax >= 0)
  {
    atomicMin(&fs.imgYMin[tid], boxes[tid].yMin); atomicMax(&fs.imgYMax[tid], boxes[tid].yMax);
    atomicMin(&fs.imgXMin[tid], boxes[tid].xMin); atomicMax(&fs.imgXMax[tid], boxes[tid].xMax);
  }
  if(tid == 0 && lOob)
  {
    atomicAdd(&fs.nOob, lOob);
    atomicOr(&fs.status, static_cast<unsigned int>(SSD_ST_OOB_PIXEL));
  }
  ph.mark(4);
  ph.finish();
}

/* ========================================================================= */
/* BestLine (segmentation.cpp:409-487): a pair of points per lane, the waves dealt out over the lists */

/* (the residual of a pair's line, three forms: ssd_bestline.h — host + device code, the CPU suite runs its host build) */

/* line_residual_onepass for lists of at most 64 points held one per lane (myX, myY of lane i = point i): the walk over the
 * points reads them with v_readlane (a few cycles) instead of LDS (a round trip per point in a lone wave) */
__device__ __forceinline__ double line_residual_lanes(int myX, int myY, int m, int p, int q, LineI &line)
{
  line = line_through_i(__shfl(myX, p), __shfl(myY, p), __shfl(myX, q), __shfl(myY, q));
  return line_residual_onepass([&](int i, int &x, int &y) { x = __builtin_amdgcn_readlane(myX, i); y = __builtin_amdgcn_readlane(myY, i); }, m, line);
}

/* all 64 lanes of the calling wave take part, on the pairs tStart + lane, tStart + tStride + lane, ..: the best of them
 * (residual, pair index, line; pair index 0x7fffffff = none) is returned in every lane */
__device__ void wave_best_line_part(const int *px, const int *py, int m, int lane, bool smallImage, int tStart, int tStride,
                                    double &bestRes, int &bestT, LineI &bestLine)
{
  const int nPairs = m * (m - 1) / 2;
  bestRes = 1.0e300;
  bestT = 0x7fffffff;
  bestLine = LineI{ 0, 0, 0 };
  const bool inLanes = smallImage && m <= 64;
  const int myX = inLanes && lane < m ? px[lane] : 0, myY = inLanes && lane < m ? py[lane] : 0;
  /* every lane runs the same number of rounds (the lanes' points are exchanged by shuffles); a lane without a pair
   * works on pair 0 and discards the result */
  for(int t0 = tStart; t0 < nPairs; t0 += tStride)
  {
    const int t = t0 + lane;
    const bool real = t < nPairs;
    /* decode pair t in the order of the reference's double loop (p ascending, q > p ascending) */
    int p = 0, rem = real ? t : 0;
    while(rem >= m - 1 - p)
    {
      rem -= m - 1 - p;
      p++;
    }
    const int q = p + 1 + rem;
    LineI l;
    double r;
    if(inLanes)
      r = line_residual_lanes(myX, myY, m, p, q, l);
    else
      r = smallImage && m <= 128 ? line_residual_keys(px, py, m, p, q, l) : line_residual_generic(px, py, m, p, q, l);
    if(real && (bestT == 0x7fffffff || r < bestRes))     /* min_element: first of equal minima (t ascends per lane) */
    {
      bestRes = r;
      bestT = t;
      bestLine = l;
    }
  }
  /* butterfly: smallest residual, ties to the smaller pair index */
#pragma unroll
  for(int o = 32; o > 0; o >>= 1)
  {
    const double oRes = __shfl_xor(bestRes, o);
    const int oT = __shfl_xor(bestT, o);
    const int oa = __shfl_xor(bestLine.a, o), ob = __shfl_xor(bestLine.b, o), oc = __shfl_xor(bestLine.c, o);
    const bool mineValid = bestT != 0x7fffffff, otherValid = oT != 0x7fffffff;
    const bool take = otherValid && (!mineValid || oRes < bestRes || (oRes == bestRes && oT < bestT));
    if(take)
    {
      bestRes = oRes; bestT = oT; bestLine.a = oa; bestLine.b = ob; bestLine.c = oc;
    }
  }
}

/* one wave, all pairs */
__device__ LineI wave_best_line(const int *px, const int *py, int m, int lane, bool smallImage)
{
  double res;
  int t;
  LineI l;
  wave_best_line_part(px, py, m, lane, smallImage, 0, 64, res, t, l);
  return l;
}

/* ========================================================================= */
/* K3: outline of one step plateau image — one workgroup per (slot, frame)      */

/* (the image kernels' thread counts, kMaxCols and kMaxProbe: ssd_k_entry.h - the launch rules need them too) */

struct OutlineShared
{
  int yFirst[kMaxCols], ySecond[kMaxCols];
  int ex[4][kMaxCols], ey[4][kMaxCols];      /* the four point lists: FL, FR, BL, BR */
  int en[4];
  LineI line[4];
  int nRight, nLeft;
  int found;
  /* vertical edges */
  int vActive[2], vLeft[2], vRight[2], vYStart[2], vYEnd[2], vProbe[2];
  int vx[2][kMaxProbe];
  int vpx[2][kMaxProbe], vpy[2][kMaxProbe], vn[2];
  double vdist[2][kMaxProbe];
  int vBest[2];
  int sortStack[2][3][kSortStack];      /* gnu_sort_on's explicit recursion stack, one per side (lane 0 of the side's wave) */
  LineD baseLine;
  LineD nline[4];                            /* the edges' lines normalised, left edges reversed (calcBaseLine) */
  double partRes[kMaxImgWaves];                 /* BestLine: every wave's best over its share of its edge's pairs */
  int partT[kMaxImgWaves];
  LineI partLine[kMaxImgWaves];
  double bounds[4][2][2];
  unsigned int status;
};

template<int T>
SSD_ENTRY(__launch_bounds__(T), k_outline, outline_block)(SSD_BYVAL(Params) P, FrameState *__restrict__ st,
                                                      unsigned long long *__restrict__ stepImg,
                                                      unsigned long long *__restrict__ planeImg,
                                                      DebugFrame *__restrict__ dbg,
                                                      unsigned long long *__restrict__ dbgImg)
{
  __shared__ OutlineShared S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = blockIdx.y, frame = blockIdx.x;
  FrameState &fs = st[frame];
  const size_t imgWords = static_cast<size_t>(P.H) * P.W64;
  if(planeImg)
  {
    /* single pass: the planes no step image is made of (bins beside a plateau; every plane of a frame that k_raster had to
     * do) are cleared where k_hist set bits, and their boxes emptied - by the frame's blocks that have no image to work on */
    const int nBusy = min(fs.nStepImages, static_cast<int>(gridDim.y));
    const bool everyone = nBusy >= static_cast<int>(gridDim.y);              /* no block without an image: all share the duty */
    const int pFirst = everyone ? slot : slot - nBusy, pStep = everyone ? static_cast<int>(gridDim.y) : static_cast<int>(gridDim.y) - nBusy;
    for(int p = pFirst < 0 ? fs.nPlanes : pFirst; p < fs.nPlanes; p += pStep)
    {
      if(fs.planeUsed[p])
        continue;
      const int y0 = fs.planeYMin[p], y1 = fs.planeYMax[p], c0 = fs.planeXMin[p], c1 = fs.planeXMax[p];
      if(y1 < y0)
        continue;
      unsigned long long *pi = planeImg + (static_cast<size_t>(fs.planeBase) + p) * imgWords;
      const int bw = c1 - c0 + 1, n = bw * (y1 - y0 + 1);
      for(int t = tid; t < n; t += T)
      {
        const int y = y0 + t / bw, c = c0 + t % bw;
        if(SSD_CHK(20, static_cast<size_t>(y) * P.W64 + c, imgWords) && SSD_CHK(26, c, P.W64) && SSD_CHK(27, p, kMaxPlanes))
          pi[static_cast<size_t>(y) * P.W64 + c] = 0ull;
      }
      __syncthreads();                               /* everybody has read the box */
      if(tid == 0)
      {
        fs.planeYMin[p] = 0x7fffffff; fs.planeYMax[p] = -1;
        fs.planeXMin[p] = 0x7fffffff; fs.planeXMax[p] = -1;
      }
    }
  }
  if(slot >= fs.nStepImages)
    return;
  const int plIdx = fs.firstStep + slot;
  PlateauState &pl = fs.pl[plIdx];
  ssd_debug_plateau *dp = dbg ? &dbg[frame].d.plateaus[plIdx] : nullptr;

  /* The raw image: the step image k_raster filled, or - single pass, the frame's plateaus covered - the planes of the
   * plateau's (two) bins, read together (BitImg::w2).  Its box (k_peaks) is the union of the planes' boxes. */
  unsigned long long *img = stepImg + (static_cast<size_t>(frame) * P.maxStepImages + slot) * imgWords;
  unsigned long long *img2 = nullptr;
  const bool fromPlanes = planeImg && ((fs.slotCovered >> slot) & 1u) != 0u;
  if(fromPlanes)
  {
    const int pa = fs.imgPlane[slot][0], pb = fs.imgPlane[slot][1];
    if(pa != 0xff)
      img = planeImg + (static_cast<size_t>(fs.planeBase) + pa) * imgWords;
    if(pb != 0xff)
      img2 = planeImg + (static_cast<size_t>(fs.planeBase) + pb) * imgWords;
  }
  const BitImg im{ img, P.W, P.H, P.W64, img2 };
  SSD_PHASE(0, 0);

  /* scan columns: x_j = xr0 + 25 j; the centre column xc = W/2 is j = jc */
  const int xStep = 25;
  const int xc = P.W / 2;
  const int xr0 = xc % xStep;
  const int jc = xc / xStep;
  const int nCols = min(kMaxCols, (P.W - 1 - xr0) / xStep + 1);

  for(int j = tid; j < kMaxCols; j += T)
  {
    S.yFirst[j] = 0x7fffffff;
    S.ySecond[j] = -1;
  }
  if(tid == 0)
  {
    S.found = 0;
    S.status = 0;
    S.nRight = S.nLeft = 0;
    S.vActive[0] = S.vActive[1] = 0;
    S.vn[0] = S.vn[1] = 0;
    S.vProbe[0] = S.vProbe[1] = 0;
  }
  __syncthreads();
  SSD_PHASE(0, 1);

  /* ---- phase B: closed image, column extents (Scanner::probeVertical, segmentation.cpp:88-111) ---- */
  unsigned long long *dbgRaw = nullptr, *dbgClosed = nullptr;
  if(dbgImg)
  {
    dbgRaw = dbgImg + ((static_cast<size_t>(frame) * (P.maxStepImages + 1) + slot) * 2) * imgWords;
    dbgClosed = dbgRaw + imgWords;
  }
  /* Only the bounding box of the raw bits is visited (with debug capture on, the whole image, so that the
   * captured images are complete).  The closing of a set stays inside the set's bounding box — except along
   * the image border: the erosion ignores out-of-image pixels (segmentation.cpp:888,928, default border), so a
   * lit pixel one row / column away from the border closes the border pixel next to it as well. */
  int by0 = fs.imgYMin[slot], by1 = fs.imgYMax[slot], bc0 = fs.imgXMin[slot], bc1 = fs.imgXMax[slot];
  const bool emptyImg = by1 < by0;
  grow_box_to_border(P.W, P.H, P.W64, by0, by1, bc1);
  if(dbgImg)
  {
    by0 = 0; by1 = P.H - 1; bc0 = 0; bc1 = P.W64 - 1;
  }
  const int bw = emptyImg && !dbgImg ? 0 : bc1 - bc0 + 1, bh = emptyImg && !dbgImg ? 0 : by1 - by0 + 1;
  if(dbgImg)
  {
    /* debug capture: the raw and the closed image whole, word by word (thread -> word column, band of rows) */
    const int nBands = bw > 0 ? max(1, T / bw) : 0;
    const int bandRows = nBands > 0 ? (bh + nBands - 1) / nBands : 0;
    for(int t = tid; t < bw * nBands; t += T)
    {
      const int band = t / bw;
      const int c = bc0 + (t - band * bw);
      const int yA = by0 + band * bandRows, yB = min(yA + bandRows, by1 + 1);
      closed_column(im, c, yA, yB, true, [&](int y, unsigned long long cw)
      {
        dbgRaw[y * P.W64 + c] = raw_word(im, y, c);
        dbgClosed[y * P.W64 + c] = cw;
      });
    }
  }
  /* the scan columns inside the box, each cut into bands of rows: thread -> (column, band); first and last closed row of
   * the band in registers, one LDS atomic pair per thread */
  if(bw > 0)
  {
    const int xLo = 64 * bc0, xHi = min(64 * bc1 + 63, P.W - 1);
    const int jLo = xLo <= xr0 ? 0 : (xLo - xr0 + xStep - 1) / xStep;
    const int jHi = xHi < xr0 ? -1 : min(nCols - 1, (xHi - xr0) / xStep);
    const int nJ = jHi - jLo + 1;
    const int nBands = nJ > 0 ? max(1, T / nJ) : 0;
    const int bandRows = nBands > 0 ? (bh + nBands - 1) / nBands : 0;
    for(int t = tid; t < nJ * nBands; t += T)
    {
      const int band = t / nJ;
      const int j = jLo + (t - band * nJ);
      const int yA = by0 + band * bandRows, yB = min(yA + bandRows, by1 + 1);
      int yLo = 0x7fffffff, yHi = -1;
      closed_scan_column(im, xr0 + xStep * j, yA, yB, [&](int y)
      {
        yLo = min(yLo, y);
        yHi = y;
      });
      if(yHi >= 0)
      {
        atomicMin(&S.yFirst[j], yLo);
        atomicMax(&S.ySecond[j], yHi);
      }
    }
  }
  __syncthreads();
  SSD_PHASE(0, 2);

  /* ---- phase C: scans (Scanner::scan :59-85, HorizontalEdgesDetector::detect :607-620),
   *      point lists (Scanner::obtainLinePoints :129-156) ---- */
  {
    /* every wave counts for itself (ballots over the columns' "long enough" bits, no serial walk through LDS) */
    bool ok0 = false, ok1 = false;
    if(lane < nCols)
      ok0 = S.ySecond[lane] >= 0 && S.ySecond[lane] - S.yFirst[lane] >= P.minImgYExtent;
    if(lane + 64 < nCols)
      ok1 = S.ySecond[lane + 64] >= 0 && S.ySecond[lane + 64] - S.yFirst[lane + 64] >= P.minImgYExtent;
    const unsigned long long okLo = __ballot(ok0), okHi = __ballot(ok1);
    auto okAt = [&](int j) { return j >= 0 && j < nCols && (((j < 64 ? okLo : okHi) >> (j & 63)) & 1ull) != 0ull; };
    int nR = 0, nL = 0;
    while(okAt(jc + nR))
      nR++;
    if(nR > 0)
      while(okAt(jc - 1 - nL))
        nL++;
    const bool found = nR > 0 && nR + nL >= 3;
    /* The four point lists (Scanner::obtainLinePoints :129-156).  Its pushes come out as two runs of consecutive columns:
     * the right lists take the columns cR0, cR0 + 1, .. (nRl of them), the left lists cL0, cL0 - 1, .. (nLl), with
     * cR0 = cL0 = the column where the reference starts: as many columns of the longer side as put total/2 + 1 on it. */
    const int total = nR + nL;
    const int half = total / 2 + 1;
    int c0, nRl, nLl;
    if(nL >= half)
    {
      const int a = nL - half;
      c0 = jc - 1 - a;
      nRl = a + 1 + nR;
      nLl = half;
    }
    else
    {
      const int b = nR > half ? nR - half : 0;
      c0 = jc + b;
      nRl = nR - b;
      nLl = b + 1 + nL;
    }
    if(found)
    {
      for(int k = tid; k < nRl; k += T)
      {
        const int j = c0 + k, x = xr0 + xStep * j;
        S.ex[kFR][k] = x; S.ey[kFR][k] = S.ySecond[j];
        S.ex[kBR][k] = x; S.ey[kBR][k] = S.yFirst[j];
      }
      for(int k = tid; k < nLl; k += T)
      {
        const int j = c0 - k, x = xr0 + xStep * j;
        S.ex[kFL][k] = x; S.ey[kFL][k] = S.ySecond[j];
        S.ex[kBL][k] = x; S.ey[kBL][k] = S.yFirst[j];
      }
    }
    if(tid == 0)
    {
      S.nRight = nR;
      S.nLeft = nL;
      /* Scanner::scan asserts xStart >= 0 (segmentation.cpp:61): below 2 * xStep columns the left scans would start left of
       * the image; there are none */
      if(nR > 0 && xc < xStep)
        S.status |= SSD_ST_ASSERT;
      if(found)
      {
        S.found = 1;
        S.en[kFR] = S.en[kBR] = nRl;
        S.en[kFL] = S.en[kBL] = nLl;
      }
    }
  }
  __syncthreads();

  SSD_PHASE(0, 3);
  if(dp && tid == 0)
  {
    dp->n_scans_right = S.nRight;
    dp->n_scans_left = S.nLeft;
    for(int s = 0; s < S.nRight; s++)
    { dp->scans_right[s][0] = xr0 + xStep * (jc + s); dp->scans_right[s][1] = S.yFirst[jc + s]; dp->scans_right[s][2] = S.ySecond[jc + s]; }
    for(int s = 0; s < S.nLeft; s++)
    { dp->scans_left[s][0] = xr0 + xStep * (jc - 1 - s); dp->scans_left[s][1] = S.yFirst[jc - 1 - s]; dp->scans_left[s][2] = S.ySecond[jc - 1 - s]; }
  }

  if(S.found)
  {
    /* ---- BestLine per horizontal edge (HorizontalEdges::Edge :570-583): wave w works on edge w % 4; then the edge's
     *      BoundaryPoints (:521-552): the first and the last list point within 10 pixels of the line, by ballots ---- */
    static_assert((T / 64) % 4 == 0, "the waves are dealt out over the four edges");
    {
      /* wave w works on edge w % 4, on every ((T / 64) / 4)-th round of 64 pairs */
      constexpr int kParts = (T / 64) / 4;
      double res;
      int t;
      LineI l;
      wave_best_line_part(S.ex[wave & 3], S.ey[wave & 3], S.en[wave & 3], lane, 3ll * P.W * P.H < (1ll << 25), 64 * (wave >> 2), 64 * kParts, res, t, l);
      if(lane == 0)
      {
        S.partRes[wave] = res;
        S.partT[wave] = t;
        S.partLine[wave] = l;
      }
    }
    __syncthreads();
    if(wave < 4)
    {
      const int e = wave, n = S.en[e];
      /* the parts' bests combined: smallest residual, ties to the smaller pair index (min_element's first of equals) */
      int best = -1;
      for(int w = e; w < (T / 64); w += 4)
        if(S.partT[w] != 0x7fffffff && (best < 0 || S.partRes[w] < S.partRes[best] || (S.partRes[w] == S.partRes[best] && S.partT[w] < S.partT[best])))
          best = w;
      const LineI l = best >= 0 ? S.partLine[best] : LineI{ 0, 0, 0 };
      const double fm = static_cast<double>(-l.a) / l.b;       /* FlatLine :508-511 */
      const double fn = static_cast<double>(-l.c) / l.b;
      int first = -1, last = -1;
      for(int i0 = 0; i0 < n; i0 += 64)
      {
        const int i = i0 + lane;
        const bool near = i < n && fabs(S.ex[e][i < n ? i : 0] * fm + fn - S.ey[e][i < n ? i : 0]) < 10;
        const unsigned long long m = __ballot(near);
        if(m != 0ull)
        {
          if(first < 0)
            first = i0 + __ffsll(static_cast<long long>(m)) - 1;
          last = i0 + 63 - __clzll(static_cast<long long>(m));
        }
      }
      if(lane == 0)
      {
        S.line[e] = l;
        double in[2] = { -1.0, -1.0 }, out[2] = { -1.0, -1.0 };
        if(first >= 0)
        {
          in[0] = S.ex[e][first]; in[1] = S.ex[e][first] * fm + fn;
          out[0] = S.ex[e][last]; out[1] = S.ex[e][last] * fm + fn;
        }
        if((in[0] == -1.0 && in[1] == -1.0) || (out[0] == -1.0 && out[1] == -1.0))
          atomicOr(&S.status, static_cast<unsigned int>(SSD_ST_ASSERT));
        S.bounds[e][0][0] = in[0]; S.bounds[e][0][1] = in[1];
        S.bounds[e][1][0] = out[0]; S.bounds[e][1][1] = out[1];
        /* calcBaseLine's first step, one edge per wave: left edges reversed */
        const bool leftEdge = e == kFL || e == kBL;
        S.nline[e] = leftEdge ? normalized_line(-l.a, -l.b, -l.c) : normalized_line(l.a, l.b, l.c);
      }
    }
    __syncthreads();
    SSD_PHASE(0, 4);

    /* ---- base line (:672-679), detectEdge windows (:681-697) ---- */
    if(tid == 0)
    {
      /* calcBaseLine: bisectors of (reversed left, right) front and back lines, then of those two;
       * slope-corrected by xyRatio^2, perpendicular through the first front-left point */
      const LineD nfl = S.nline[kFL], nfr = S.nline[kFR], nbl = S.nline[kBL], nbr = S.nline[kBR];
      const LineD front{ nfl.a + nfr.a, nfl.b + nfr.b, nfl.c + nfr.c };
      const LineD back{ nbl.a + nbr.a, nbl.b + nbr.b, nbl.c + nbr.c };
      const LineD nf = normalized_line(front.a, front.b, front.c), nb = normalized_line(back.a, back.b, back.c);
      const LineD center{ nf.a + nb.a, nf.b + nb.b, nf.c + nb.c };
      const double corr = P.xyRatio * P.xyRatio;
      const double sa = center.a * corr, sb = center.b;
      const int p0x = S.ex[kFL][0], p0y = S.ey[kFL][0];
      S.baseLine = LineD{ -sb, sa, sb * p0x - sa * p0y };

      for(int side = 0; side < 2; side++)
      {
        const int fe = side == 0 ? kFL : kFR, be = side == 0 ? kBL : kBR;
        const double fx = S.bounds[fe][1][0], fy = S.bounds[fe][1][1];
        const double bx = S.bounds[be][1][0], by = S.bounds[be][1][1];
        int lft = static_cast<int>(fmin(fx, bx) - xStep);
        int rgt = static_cast<int>(fmax(fx, bx) + xStep);
        int yStart = static_cast<int>(fy - 10);
        int yEnd = static_cast<int>(by + 10);
        if(lft < 0) lft = 0;
        if(rgt >= P.W) rgt = P.W - 1;
        if(yStart >= P.H) yStart = P.H - 1;
        if(yEnd < 0) yEnd = 0;
        if(yStart < yEnd)
          continue;
        if(rgt - lft <= 0)
        {
          S.status |= SSD_ST_ASSERT;
          continue;
        }
        int np = (yStart - yEnd) / 10 + 1;
        if(np > kMaxProbe)
        {
          np = kMaxProbe;
          S.status |= SSD_ST_OVERFLOW;
        }
        S.vActive[side] = 1;
        S.vLeft[side] = lft; S.vRight[side] = rgt; S.vYStart[side] = yStart; S.vYEnd[side] = yEnd;
        S.vProbe[side] = np;
      }
    }
    __syncthreads();
    SSD_PHASE(0, 5);

    /* ---- phase D: row probes (VerticalEdgePointsDetector :243-312) on freshly closed rows ---- */
    {
      const int np0 = S.vProbe[0], np1 = S.vProbe[1];
      for(int t = tid; t < np0 + np1; t += T)
      {
        const int side = t < np0 ? 0 : 1;
        const int k = side == 0 ? t : t - np0;
        const int y = S.vYStart[side] - 10 * k;
        const int lft = S.vLeft[side], rgt = S.vRight[side];
        /* left edge: first lit pixel of [lft, rgt-1]; right edge: last lit pixel of [lft+1, rgt] */
        const int xa = side == 0 ? lft : lft + 1;
        const int xb = side == 0 ? rgt - 1 : rgt;
        int found = -1;
        if(side == 0)
        {
          for(int c = xa >> 6; c <= (xb >> 6) && found < 0; c++)
          {
            unsigned long long cw = closed_word(im, y, c);
            if(c == (xa >> 6)) cw &= ~0ull << (xa & 63);
            if(c == (xb >> 6)) cw &= ~0ull >> (63 - (xb & 63));
            if(cw)
              found = 64 * c + __ffsll(static_cast<long long>(cw)) - 1;
          }
        }
        else
        {
          for(int c = xb >> 6; c >= (xa >> 6) && found < 0; c--)
          {
            unsigned long long cw = closed_word(im, y, c);
            if(c == (xa >> 6)) cw &= ~0ull << (xa & 63);
            if(c == (xb >> 6)) cw &= ~0ull >> (63 - (xb & 63));
            if(cw)
              found = 64 * c + 63 - __clzll(static_cast<long long>(cw));
          }
        }
        S.vx[side][k] = found;
      }
    }
    __syncthreads();
    SSD_PHASE(0, 6);

    /* compact the probe hits in scan order (y descending), distances to the base line (:708-721): wave 0 the left
     * edge's, wave 1 the right edge's; places by ballot and prefix count */
    if(wave < 2)
    {
      const int side = wave, np = S.vProbe[side];
      int n = 0;
      for(int k0 = 0; k0 < np; k0 += 64)
      {
        const int k = k0 + lane;
        const int x = k < np ? S.vx[side][k] : -1;
        const unsigned long long m = __ballot(x >= 0);
        if(x >= 0)
        {
          const int at = n + __popcll(m & ((1ull << lane) - 1ull));
          const int y = S.vYStart[side] - 10 * k;
          S.vpx[side][at] = x;
          S.vpy[side][at] = y;
          S.vdist[side][at] = fabs(x * S.baseLine.a + y * S.baseLine.b + S.baseLine.c);
        }
        n += __popcll(m);
      }
      if(lane == 0)
      {
        S.vn[side] = n;
        S.vBest[side] = -1;
      }
    }
    __syncthreads();
    SSD_PHASE(0, 7);

    /* findBestPoint (segmentation.cpp:708-728): the element of rank 2n/3 by distance, by counting; ties see below */
    for(int t = tid; t < S.vn[0] + S.vn[1]; t += T)
    {
      const int side = t < S.vn[0] ? 0 : 1;
      const int i = side == 0 ? t : t - S.vn[0];
      const int n = S.vn[side];
      const double di = S.vdist[side][i];
      int rank = 0;
      for(int k = 0; k < n; k++)
      {
        const double dk = S.vdist[side][k];
        rank += (dk < di || (dk == di && k < i)) ? 1 : 0;
      }
      if(rank == 2 * n / 3)
        S.vBest[side] = i;
    }
    __syncthreads();
    SSD_PHASE(0, 8);

    /* The reference sorts with std::ranges::sort (segmentation.cpp:724), which is not stable: among points at exactly
     * the same distance, the one on rank 2n/3 is whatever libstdc++'s introsort leaves there.  Only when that can
     * matter — the selected distance is duplicated AND a duplicate would give another line — the keys are sorted the
     * way the library does it (ssd_sort.h; vdist in place, vx as the payload: neither is needed afterwards). */
    if(wave < 2 && S.vn[wave] > 0 && S.vBest[wave] >= 0)
    {
      const int side = wave, n = S.vn[side], best = S.vBest[side];
      const double D = S.vdist[side][best];
      const double cBest = -S.baseLine.a * S.vpx[side][best] - S.baseLine.b * S.vpy[side][best];
      bool mine = false;
      for(int k = lane; k < n; k += 64)
        if(k != best && S.vdist[side][k] == D && (-S.baseLine.a * S.vpx[side][k] - S.baseLine.b * S.vpy[side][k]) != cBest)
          mine = true;
      const bool ambiguous = __ballot(mine) != 0ull;
      if(ambiguous && lane == 0)
      {
        for(int k = 0; k < n; k++)
          S.vx[side][k] = k;
        gnu_sort_on(SortKeys{ S.vdist[side], S.vx[side] }, n, S.sortStack[side][0], S.sortStack[side][1], S.sortStack[side][2]);
        S.vBest[side] = S.vx[side][2 * n / 3];
      }
    }
    __syncthreads();
  }
  SSD_PHASE(0, 9);

  /* ---- Corners (:731-751), quadrilateral, isConvex (:758-772), imgPointsToWorld (pointcloud.cpp:476-487) ---- */
  if(tid == 0)
  {
    double quad[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    int valid = 0;
    int cornerFound[4] = { 0, 0, 0, 0 };
    LineD vl[2] = { { 0, 0, 0 }, { 0, 0, 0 } };
    int vFound[2] = { 0, 0 };
    if(S.found)
    {
      for(int side = 0; side < 2; side++)
        if(S.vActive[side] && S.vn[side] > 0 && S.vBest[side] >= 0)
        {
          const int bx = S.vpx[side][S.vBest[side]], by = S.vpy[side][S.vBest[side]];
          vl[side] = LineD{ S.baseLine.a, S.baseLine.b, -S.baseLine.a * bx - S.baseLine.b * by };   /* parallel(), :368-371 */
          vFound[side] = 1;
        }
      for(int e = 0; e < 4; e++)
      {
        const int side = (e == kFL || e == kBL) ? 0 : 1;
        double x = S.bounds[e][1][0], y = S.bounds[e][1][1];         /* value_or(bounds.outer) :947-953 */
        if(vFound[side])
        {
          const LineD hl{ static_cast<double>(S.line[e].a), static_cast<double>(S.line[e].b), static_cast<double>(S.line[e].c) };
          double ix, iy;
          if(intersect60(vl[side], hl, ix, iy))
          {
            x = ix; y = iy;
            cornerFound[e] = 1;
          }
        }
        quad[2 * e] = x;
        quad[2 * e + 1] = y;
      }
      /* isConvex: edge vectors q0->q1, q1->q3, q3->q2, q2->q0 must all turn the same way */
      const double vx[4] = { quad[2] - quad[0], quad[6] - quad[2], quad[4] - quad[6], quad[0] - quad[4] };
      const double vy[4] = { quad[3] - quad[1], quad[7] - quad[3], quad[5] - quad[7], quad[1] - quad[5] };
      auto pos = [&](int i, int k) { return vx[i] * vy[k] - vx[k] * vy[i] > 0; };
      const bool positive = pos(0, 1);
      valid = (positive == pos(1, 2) && positive == pos(2, 3) && positive == pos(3, 0)) ? 1 : 0;
    }
    pl.outlineFound = S.found;
    pl.valid = valid;
    for(int k = 0; k < 4; k++)
    {
      pl.quadImg[2 * k] = quad[2 * k];
      pl.quadImg[2 * k + 1] = quad[2 * k + 1];
      pl.quadWorld[2 * k] = P.xMin + quad[2 * k] * P.xToWorld;            /* Projection2D::imageToWorld :84-88 */
      pl.quadWorld[2 * k + 1] = P.yMax - quad[2 * k + 1] * P.yToWorld;
    }
    if(S.status)
      atomicOr(&fs.status, S.status);

    if(dp)
    {
      dp->outline_found = S.found;
      dp->valid = valid;
      for(int k = 0; k < 8; k++) { dp->quad_img[k] = pl.quadImg[k]; dp->quad_world[k] = pl.quadWorld[k]; }
      if(S.found)
      {
        for(int e = 0; e < 4; e++)
        {
          dp->n_edge_pts[e] = S.en[e];
          dp->line[e][0] = S.line[e].a; dp->line[e][1] = S.line[e].b; dp->line[e][2] = S.line[e].c;
          for(int io = 0; io < 2; io++) { dp->bounds[e][io][0] = S.bounds[e][io][0]; dp->bounds[e][io][1] = S.bounds[e][io][1]; }
          dp->corner_found[e] = cornerFound[e];
        }
        dp->base_line[0] = S.baseLine.a; dp->base_line[1] = S.baseLine.b; dp->base_line[2] = S.baseLine.c;
        for(int side = 0; side < 2; side++)
        {
          dp->vedge_found[side] = vFound[side];
          dp->n_vpts[side] = S.vn[side];
          for(int k = 0; k < S.vn[side]; k++) { dp->vpts[side][k][0] = S.vpx[side][k]; dp->vpts[side][k][1] = S.vpy[side][k]; }
          if(vFound[side])
          {
            dp->best_pt[side][0] = S.vpx[side][S.vBest[side]]; dp->best_pt[side][1] = S.vpy[side][S.vBest[side]];
            dp->vline[side][0] = vl[side].a; dp->vline[side][1] = vl[side].b; dp->vline[side][2] = vl[side].c;
          }
        }
      }
    }
  }
  __syncthreads();
  SSD_PHASE(0, 10);

  /* leave the raw image zeroed for the next batch (all its bits lie inside the bounding box) */
  if(!emptyImg)
  {
    const int cy0 = fs.imgYMin[slot], cc0 = fs.imgXMin[slot];
    const int cw = fs.imgXMax[slot] - cc0 + 1, ch = fs.imgYMax[slot] - cy0 + 1;
    for(int idx = tid; idx < cw * ch; idx += T)
    {
      const int ry = idx / cw;
      const size_t o = static_cast<size_t>(cy0 + ry) * P.W64 + cc0 + (idx - ry * cw);
      if(!SSD_CHK(21, o, imgWords))
        continue;
      img[o] = 0ull;                                 /* unconditionally: a load first would make every word a round trip */
      if(img2)
        img2[o] = 0ull;
    }
    if(fromPlanes && tid < 2)
    {
      /* the planes' boxes go with their bits (k_predict resets them as well; this keeps "box empty = plane zero" at all times) */
      const int p = fs.imgPlane[slot][tid];
      if(p != 0xff)
      {
        fs.planeYMin[p] = 0x7fffffff; fs.planeYMax[p] = -1;
        fs.planeXMin[p] = 0x7fffffff; fs.planeXMax[p] = -1;
      }
    }
  }
  SSD_PHASE(0, 11);
}

/* ========================================================================= */
/* K3b: ground quadrilateral and the prepared quadrilateral tests              */

/* Thresholds of k_inquad's cell classification for one live quadrilateral, on the grid of K1's cell boxes.  A cell's box
 * [x0, x1] x [y0, y1] holds points with xMin + x0 / boxX <= x < xMin + (x1 + 1) / boxX (K1 truncates).  Ground: the box lies
 * wholly outside the quadrilateral's strict bounding box iff x1 <= b.x, x0 >= b.y, y1 <= b.z or y0 >= b.w; tread: wholly inside
 * the constant cell iff x0 >= b.x, x1 <= b.y, y0 >= b.z, y1 <= b.w — with a 1e-9 m margin against the truncation's rounding. */
__device__ __forceinline__ int4 live_box_thresholds(const QuadTest &t, bool ground, const PointParams &P)
{
  const double m = 1.0e-9;
  int4 b;
  if(ground)
  {
    b.x = static_cast<int>(floor((t.bxLo - P.xMin - m) * P.boxX)) - 1;
    b.y = static_cast<int>(ceil((t.bxUp - P.xMin + m) * P.boxX));
    b.z = static_cast<int>(floor((t.byLo - P.yMin - m) * P.boxY)) - 1;
    b.w = static_cast<int>(ceil((t.byUp - P.yMin + m) * P.boxY));
  }
  else
  {
    b.x = static_cast<int>(ceil((t.fx0 - P.xMin + m) * P.boxX));
    b.y = static_cast<int>(floor((t.fx1 - P.xMin - m) * P.boxX)) - 1;
    b.z = static_cast<int>(ceil((t.fy0 - P.yMin + m) * P.boxY));
    b.w = static_cast<int>(floor((t.fy1 - P.yMin - m) * P.boxY)) - 1;
  }
  return b;
}

/* one wave per frame: lane k < kMaxPlateaus builds the test of plateau k, lane kGroundAcc the ground's */
SSD_ENTRY(__launch_bounds__(64), k_quads, quads_block)(SSD_BYVAL(Params) P, FrameState *__restrict__ st, int nframes, DebugFrame *__restrict__ dbg)
{
  static_assert(kMaxPlateaus + 1 <= 64, "one lane per accumulator");
  const int frame = blockIdx.x, lane = threadIdx.x;
  if(frame >= nframes)
    return;
  FrameState &fs = st[frame];
  SSD_PHASE(1, 0);
  if(lane <= kMaxPlateaus)
  {
    fs.sumZ[lane] = 0;
    fs.cnt[lane] = 0;
  }
  for(int i = lane; i < kMaxGroundStrips; i += 64)
    fs.groundStripMax[i] = -1;
  const int first = fs.firstStep, last = fs.firstStep + fs.nStepImages;
  const int groundInd = fs.groundInd;
  const bool mine = lane >= first && lane < last && lane < kMaxPlateaus;
  /* every lane with an image fetches its quadrilateral before anyone knows whether it is valid: one round trip for both */
  double quad[8];
#pragma unroll
  for(int k = 0; k < 8; k++)
    quad[k] = mine ? fs.pl[lane].quadWorld[k] : 0.0;
  const bool valid = mine && fs.pl[lane].valid;
  const unsigned long long validMask = __ballot(valid);
  const int firstValid = validMask ? __ffsll(static_cast<long long>(validMask)) - 1 : -1;
  const bool groundLane = lane == kGroundAcc && firstValid >= 0 && groundInd >= 0;
  int err = 0;
  /* the live tests once more in LDS, for the check of their maps (quad_cell_unsound) that all lanes share below */
  __shared__ QuadTest sT[kMaxLive];
  __shared__ QuadEdgesD sW[kMaxLive];
  __shared__ unsigned int sBad[kMaxLive];
  QuadEdgesF ef;
  int mySlot = -1;
  SSD_PHASE_IF(lane == firstValid, 1, 1);
  {
    /* calcGroundQuadrilateral (pointcloud.cpp:489-512) from the front edge of the first valid step */
    const int srcLane = firstValid >= 0 ? firstValid : 0;
    double q[4];
#pragma unroll
    for(int k = 0; k < 4; k++)
      q[k] = __shfl(quad[k], srcLane);
    if(groundLane)
    {
      const double yMin = P.yMin;
      if(q[1] < q[3])
      {
        quad[0] = q[0]; quad[1] = yMin;
        quad[2] = q[2] + (q[3] - yMin) * (q[3] - q[1]) / (q[2] - q[0]); quad[3] = yMin;
      }
      else
      {
        quad[0] = q[0] + (q[1] - yMin) * (q[1] - q[3]) / (q[0] - q[2]); quad[1] = yMin;
        quad[2] = q[2]; quad[3] = yMin;
      }
      quad[4] = q[0]; quad[5] = q[1];
      quad[6] = q[2]; quad[7] = q[3];
#pragma unroll
      for(int k = 0; k < 8; k++)
        fs.groundQuadWorld[k] = quad[k];
    }
  }
  SSD_PHASE_IF(lane == firstValid, 1, 2);
  if(groundLane || valid)
  {
    /* built in registers (ssd_quadtest.h), stored to the frame's table once */
    QuadTest t;
    SSD_PHASE_IF(lane == firstValid, 1, 3);
    build_quad_test(quad, t);
    err = t.err;
    SSD_PHASE_IF(lane == firstValid, 1, 4);
    /* one quadrilateral the reference would throw on ends the frame (quadrilateralTest.cpp:283-372) */
    const bool threwHere = __ballot(err != 0) != 0ull;
    /* The live quadrilaterals go into a compact table (at most one per image slot + the ground): k_inquad copies it
     * whole, without asking which entries matter.  Slot order = accumulator order (treads ascending, ground last). */
    const unsigned long long liveMask = threwHere ? 0ull : __ballot(true);
    if(!threwHere)
    {
      const int slot = __popcll(liveMask & ((1ull << lane) - 1ull));
      if(slot < kMaxLive)
      {
        fs.qtLive[slot] = t;
        QuadGridSegs sg;
        build_grid_segs(t, P.pt.xMin, P.pt.yMin, P.pt.boxX, P.pt.boxY, sg);
        fs.segLive[slot] = sg;
        QuadEdgesD w;
        quad_edges_coeffs(t, sg.ok, P.pt.xMin, P.pt.xMax, P.pt.yMin, P.pt.yMax, w, ef);
        sT[slot] = t;
        sW[slot] = w;
        sBad[slot] = 0u;
        mySlot = slot;
        fs.liveBox[slot] = live_box_thresholds(t, groundLane, P.pt);
        fs.liveAcc[slot] = static_cast<unsigned char>(lane);
        /* the groups of 4 height bins this accumulator's plateau occupies (matched against the cells' masks) */
        const PlateauState &pl = fs.pl[groundLane ? groundInd : lane];
        unsigned int groups = 0u;
        const int effLo = pl.effLo, effHi = pl.effHi;
        for(int b = effLo; b <= effHi; b++)
          groups |= 1u << (b / kBinsPerGroup);
        fs.liveGroups[slot] = groups;
      }
    }
  }
  {
    /* k_inquad's single-precision edge tests (ssd_quadtest.h, build_quad_edges): the reference's map of each live quadrilateral is
     * checked cell by cell - nine cells each, dealt out to the wave's lanes (one lane doing its own quadrilateral's nine: 0.086 ms
     * per launch of 1024 frames against 0.031) - and a quadrilateral whose map accepts points beyond an edge gets no margin */
    const int nL = __popcll(__ballot(mySlot >= 0));
    __syncthreads();
    for(int item = lane; item < nL * 9; item += 64)
    {
      const int sl = item / 9, cell = item - 9 * sl;
      if(sW[sl].fine != 0 && quad_cell_unsound(sT[sl], sW[sl], cell / 3, cell % 3))
        atomicOr(&sBad[sl], 1u);
    }
    __syncthreads();
    if(mySlot >= 0)
    {
      ef.m = quad_edges_margin(sW[mySlot], sBad[mySlot] != 0u);
      fs.edgeLive[mySlot] = ef;
    }
  }
  SSD_PHASE_IF(lane == firstValid, 1, 5);
  const bool threw = __ballot(err != 0) != 0ull;
  const bool active = (groundLane || valid) && !threw;
  if(lane <= kMaxPlateaus)
    fs.accActive[lane] = active ? 1 : 0;
  const unsigned long long activeMask = __ballot(active);
  /* bin -> slot of the live table (0xff = no live quadrilateral takes this bin) */
  for(int b = lane; b < kMaxBins; b += 64)
  {
    const int p = b < P.nBins ? fs.lut[b] : 0xff;
    const int acc = p == groundInd ? kGroundAcc : p;
    const bool live = p != 0xff && ((activeMask >> acc) & 1ull);
    fs.lutLive[b] = live ? static_cast<unsigned char>(__popcll(activeMask & ((1ull << acc) - 1ull))) : static_cast<unsigned char>(0xff);
  }

  SSD_PHASE_IF(lane == firstValid, 1, 6);
  unsigned int wanted = 0u;
  for(int b = lane; b < P.nBins; b += 64)
  {
    const int p = fs.lut[b];
    if(p != 0xff && ((activeMask >> (p == groundInd ? kGroundAcc : p)) & 1ull))
      wanted |= 1u << (b / kBinsPerGroup);
  }
#pragma unroll
  for(int o = 32; o > 0; o >>= 1)
    wanted |= __shfl_xor(wanted, o);
  if(lane == 0)
  {
    fs.firstValidInd = firstValid;
    if(threw)
      fs.status |= SSD_ST_THROW;
    fs.wantedQuads = wanted;
    fs.anyActive = activeMask != 0ull ? 1u : 0u;
    fs.nLive = min(__popcll(activeMask), kMaxLive);
  }
  SSD_PHASE_IF(lane == firstValid, 1, 7);
  if(dbg)
  {
    ssd_debug_frame &d = dbg[frame].d;
    if(lane == 0)
      d.first_valid_ind = firstValid;
    if(lane == kGroundAcc)
    {
      for(int k = 0; k < 8; k++)
        d.ground_quad_world[k] = groundLane ? fs.groundQuadWorld[k] : 0.0;
      d.ground_quad_err = groundLane ? err : 0;
    }
    if(lane >= first && lane < last && lane < kMaxPlateaus)
      d.plateaus[lane].quad_err = valid ? err : 0;
  }
}

/* ========================================================================= */
/* K4: in-quadrilateral filter, z sums, ground image                           */

/* What of the ground image is ever looked at: detectFrontEdge (segmentation.cpp:879-917) closes it and BottomScanner
 * (:159-241) probes the pixel columns x_j = W/2 + 50 k bottom-up, stopping at the image centre.  A closed pixel is a function
 * of the raw 5 x 5 neighbourhood (ssd_closing.h, closed_scan_column), so k_final reads raw pixels only in the columns
 * x_j - 2 .. x_j + 2 and the rows >= H/2 - 1.  Outside debug capture k_inquad therefore sets just those: a twentieth of the
 * ground pixels, few enough to go to memory one atomic each — no LDS windows, no flushes, no keys in the production kernel.
 * (kGroundScanStep = BottomScanner's column distance; the same constants are k_final's.) */
constexpr int kGroundScanStep = 50;
__device__ __forceinline__ int ground_scan_x0(int W) { return (W / 2) % kGroundScanStep; }
__device__ __forceinline__ int ground_strip_row0(int H) { return H / 2 - 1; }
/* is pixel column ix within two of a scan column x_j = x0 + 50 j, j any integer (also j = -1 and beyond the last scanned
 * column: k_final clears those strips with the others)?  u / 50 by multiply-high with a constant that IS exact over the whole
 * range a pixel column can take (ix < 8192: u < 8300; proven at compile time below — round 3's 1311 >> 16 was off by one from
 * u = 4699 on and only the predicate happened to survive it). */
constexpr unsigned int strip_div50(unsigned int u) { return (u * 5243u) >> 18; }
constexpr bool strip_div50_exact()
{
  for(unsigned int u = 0; u < 16384u; u++)
    if(strip_div50(u) != u / 50u)
      return false;
  return true;
}
static_assert(strip_div50_exact(), "strip_div50 must equal u / 50 for every pixel column of an image up to 8192 wide");
__device__ __forceinline__ bool ground_strip_column(int ix, int x0)
{
  const unsigned int u = static_cast<unsigned int>(ix + 2 - x0 + kGroundScanStep);       /* >= 3 */
  const unsigned int r = u - kGroundScanStep * strip_div50(u);
  return r <= 4u;
}
/* the same with the strip's number (0 = the strip left of the first scan column; below kMaxGroundStrips for any width up to
 * 8192) and whether ix is the strip's CENTRE column, i.e. a scan column itself */
__device__ __forceinline__ bool ground_strip_of(int ix, int x0, int &strip, bool &centre)
{
  const unsigned int u = static_cast<unsigned int>(ix + 2 - x0 + kGroundScanStep);
  const unsigned int q = strip_div50(u), r = u - kGroundScanStep * q;
  strip = static_cast<int>(q);
  centre = r == 2u;
  return r <= 4u;
}
static_assert((8191 + 2 + kGroundScanStep) / kGroundScanStep < kMaxGroundStrips, "a strip number for every pixel column");

template<bool FULL>
struct InquadLds
{
  unsigned long long wins[FULL ? kThreads / 64 : 1][FULL ? kWinWords : 1];
  unsigned int wmiss[FULL ? kThreads / 64 : 1][kWaveMissWords];
  ImageBox box[1];
  QuadTest qts[kMaxLive];                       /* FrameState::qtLive: slot k = accumulator liveAcc[k] */
  QuadGridSegs segs[kMaxLive];                  /* FrameState::segLive */
  QuadEdgesF edges[kMaxLive + 1];               /* FrameState::edgeLive with PreXY::dE0 folded into m; row kMaxLive ("no quadrilateral"): m = infinity */
  K1Consts kc;                                  /* what only the rare double-precision paths need (as K1) */
  unsigned char lut[kMaxBins];                  /* bin -> live slot, kMaxLive = none */
  unsigned long long lsum[kMaxLive][8];
  unsigned int lcnt[kMaxLive][8];
  unsigned int lOob;
  unsigned short cellList[kMaxCellsPerBlockInquad];
  unsigned int listScratch[2 * kWavesPerBlock];
  unsigned int liveGroups[kMaxLive];
  int4 liveBox[kMaxLive];                       /* per live quadrilateral: thresholds of the cell classification on K1's grid */
  unsigned char liveAcc[kMaxLive];
  int nLive, groundSlot;
  int nextGroup;                                /* the walk's groups of four cells are dealt out to the waves as they come free */
  int stripMax[kMaxGroundStrips];               /* FrameState::groundStripMax as the block found it, raised by its own centre-column pixels */
};

template<int SRC, bool FULL, bool CHECKS>
__device__ __forceinline__ void inquad_block(InquadLds<FULL> &L, const float *__restrict__ xyz, size_t strideFloats, const PointParams &P,
                                             const PreXY &Q, const PixelParams &X, FrameState *__restrict__ st,
                                             unsigned long long *__restrict__ groundImg,
                                             const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints, const DepthSrc &D,
                                             const int frame, const int chunkIdx)
{
  auto &wins = L.wins;
  auto &wmiss = L.wmiss;
  ImageBox (&box)[1] = L.box;
  QuadTest (&qts)[kMaxLive] = L.qts;
  QuadGridSegs (&segs)[kMaxLive] = L.segs;
  unsigned char (&lut)[kMaxBins] = L.lut;
  unsigned long long (&lsum)[kMaxLive][8] = L.lsum;
  unsigned int (&lcnt)[kMaxLive][8] = L.lcnt;
  unsigned int &lOob = L.lOob;
  unsigned short (&cellList)[kMaxCellsPerBlockInquad] = L.cellList;
  unsigned int (&listScratch)[2 * kWavesPerBlock] = L.listScratch;
  unsigned int (&liveGroups)[kMaxLive] = L.liveGroups;
  int4 (&liveBox)[kMaxLive] = L.liveBox;
  unsigned char (&liveAcc)[kMaxLive] = L.liveAcc;
  int &nLive = L.nLive;
  int &groundSlot = L.groundSlot;

  const int tid = threadIdx.x, lane = tid & 63;
  FrameState &fs = st[frame];
  /* Everything the block needs of the frame's state is requested at once, the "anything to do?" flag first: one memory round
   * trip for the lot (as code in sequence — flag, early exit, tables — it was two, a tenth of a block's life). */
  const unsigned int anyActive = fs.anyActive;              /* block-uniform: set by k_quads */
  const unsigned char lutMine = tid < kMaxBins ? fs.lutLive[tid] : static_cast<unsigned char>(0xff);
  const unsigned char accMine = tid < kMaxLive ? fs.liveAcc[tid] : static_cast<unsigned char>(0);
  const unsigned int groupsMine = tid < kMaxLive ? fs.liveGroups[tid] : 0u;
  const int stripMaxMine = (!FULL && tid < kMaxGroundStrips) ? fs.groundStripMax[tid] : -1;
  const int4 boxMine = tid < kMaxLive ? fs.liveBox[tid] : make_int4(0, 0, 0, 0);
  const int nLiveG = fs.nLive;
  const unsigned char groundActive = fs.accActive[kGroundAcc];
  constexpr int qtWords = kMaxLive * static_cast<int>(sizeof(QuadTest) / 4), sgWords = kMaxLive * static_cast<int>(sizeof(QuadGridSegs) / 4);
  constexpr int qtPer = (qtWords + kThreads - 1) / kThreads, sgPer = (sgWords + kThreads - 1) / kThreads;
  unsigned int qtw[qtPer], sgw[sgPer];
  constexpr int egWords = kMaxLive * static_cast<int>(sizeof(QuadEdgesF) / 4);
  static_assert(sizeof(QuadEdgesF) == 64 && egWords + 16 <= 2 * kThreads, "two words of the edge table per thread");
  float edgeMine[2];
#pragma unroll
  for(int k = 0; k < 2; k++)
    edgeMine[k] = tid + k * kThreads < egWords ? reinterpret_cast<const float *>(fs.edgeLive)[tid + k * kThreads] : 0.0f;
  {
    /* the live quadrilateral tests as 32-bit words: the whole table, unconditionally — asking "how many are live?" first
     * would make every element two dependent round trips */
    const unsigned int *src = reinterpret_cast<const unsigned int *>(fs.qtLive);
    const unsigned int *srcS = reinterpret_cast<const unsigned int *>(fs.segLive);
#pragma unroll
    for(int k = 0; k < qtPer; k++)
      qtw[k] = tid + k * kThreads < qtWords ? src[tid + k * kThreads] : 0u;
#pragma unroll
    for(int k = 0; k < sgPer; k++)
      sgw[k] = tid + k * kThreads < sgWords ? srcS[tid + k * kThreads] : 0u;
  }
  if(!anyActive)
    return;
  BlockPhase ph(1);
  if(tid == 0)
  {
    box[0] = ImageBox{ 0x7fffffff, -1, 0x7fffffff, -1 };
    lOob = 0;
    nLive = nLiveG;
    groundSlot = (nLiveG > 0 && groundActive) ? nLiveG - 1 : -1;     /* the ground is the last accumulator */
    L.nextGroup = 0;
    k1_consts_fill(L.kc, P, &X);
  }
  if(tid < kMaxBins)
    lut[tid] = lutMine == 0xff ? static_cast<unsigned char>(kMaxLive) : lutMine;      /* bin -> slot of the live table, kMaxLive = nothing to do for this bin */
  /* the edges for the single-precision test: stage_quad_edges() by hand, because the words were asked for above, in the one round
   * trip with everything else the block reads of the frame */
#pragma unroll
  for(int k = 0; k < 2; k++)
  {
    const int w = tid + k * kThreads;
    if(w < egWords + 16)
      reinterpret_cast<float *>(L.edges)[w] = quad_edge_word(w, egWords, edgeMine[k], Q.dE0);
  }
  if(!FULL && tid < kMaxGroundStrips)
    L.stripMax[tid] = stripMaxMine;
  if(tid < kMaxLive)
  {
    liveAcc[tid] = accMine;
    liveGroups[tid] = groupsMine;
    liveBox[tid] = boxMine;                     /* thresholds of the cell classification (k_quads, live_box_thresholds) */
  }
  for(int i = tid; i < kMaxLive * 8; i += kThreads)
  {
    (&lsum[0][0])[i] = 0ull;
    (&lcnt[0][0])[i] = 0u;
  }
  if(FULL)
  {
    for(int i = tid; i < (kThreads / 64) * kWinWords; i += kThreads)
      (&wins[0][0])[i] = 0ull;
    if(tid < kThreads / 64)
      wavemiss_init(wmiss[tid]);
  }
  {
    unsigned int *dst = reinterpret_cast<unsigned int *>(qts);
    unsigned int *dstS = reinterpret_cast<unsigned int *>(segs);
#pragma unroll
    for(int k = 0; k < qtPer; k++)
      if(tid + k * kThreads < qtWords)
        dst[tid + k * kThreads] = qtw[k];
#pragma unroll
    for(int k = 0; k < sgPer; k++)
      if(tid + k * kThreads < sgWords)
        dstS[tid + k * kThreads] = sgw[k];
  }
  __syncthreads();
  ph.mark(0);                                               /* tables in LDS */

  /* strideFloats counts floats, or 16-bit depth values for kSrcDepth16 */
  const float *base = SRC == kSrcDepth16
    ? reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(xyz) + static_cast<size_t>(frame) * strideFloats)
    : xyz + static_cast<size_t>(frame) * strideFloats;
  const int begin = chunkIdx * chunkPoints;
  const int end = min(begin + chunkPoints, P.nPoints);
  unsigned long long *gimg = groundImg + static_cast<size_t>(frame) * X.H * X.W64;
  const int copy = lane & 7;
  const unsigned int imgWords = static_cast<unsigned int>(X.H) * X.W64;
  unsigned long long *ww = wins[FULL ? tid >> 6 : 0];
  unsigned int *wm = wmiss[FULL ? tid >> 6 : 0];
  WaveWindow win;
  win.limitWords = imgWords;                   /* the ground image: one per frame */
  /* strips only (!FULL): the scan columns' offset, the first row of interest, the lane's rows written so far */
  const int stripX0 = ground_scan_x0(X.W), stripRow0 = ground_strip_row0(X.H);
  int gy0 = 0x7fffffff, gy1 = -1;
  unsigned int *gimg32 = reinterpret_cast<unsigned int *>(gimg);

  /* calcAverageZ (pointcloud.cpp:574-581) as an order-independent fixed-point sum: a thread walks down a
   * camera column, so consecutive hits nearly always belong to the same quadrilateral — the running sum
   * stays in registers and goes to LDS only when the quadrilateral changes */
  int curQ = -1;
  unsigned long long accZ = 0;                               /* modulo 2^64: see z_plus_magic_bits */
  unsigned int accN = 0, oob = 0;
  auto flushAcc = [&]()
  {
    if(curQ >= 0 && accN)
    {
      atomicAdd(&lsum[curQ][copy], accZ - static_cast<unsigned long long>(accN) * static_cast<unsigned long long>(kMagicBits));
      atomicAdd(&lcnt[curQ][copy], accN);
    }
  };

  /* only the cells that hold a bin of a live quadrilateral are walked, four per wave iteration (cell_list_build) */
  const int cell0 = begin / kCell;
  const int nCells = (end - begin + kCell - 1) / kCell;
  /* A cell is walked only if it can change a sum.  Ground: its points INSIDE the ground quadrilateral are added (and
   * rastered) — a cell whose bounding box lies outside the quadrilateral's (strict) bounding box has none.  Treads: k_raster
   * already summed every point of the plateau, so the points OUTSIDE the quadrilateral are taken off here — a cell whose
   * bounding box lies inside the quadrilateral's large constant cell (QuadTest::fx0 ..) has none.  The box covers all
   * in-range points of the cell, whatever their plateau: conservative for each of them. */
  const unsigned int wantedQuads = fs.wantedQuads;
  const int gSlot = groundSlot;
  const int count = cell_list_build(tileMasks + static_cast<size_t>(frame) * tileMaskStride + cell0, nCells, X.cellCols,
                                    [&](const uint2 info)
                                    {
                                      if((info.x & wantedQuads) == 0u)
                                        return false;
                                      /* the box on K1's 256 x 256 grid against each live quadrilateral's thresholds on the
                                       * same grid (liveBox, computed once per block from the doubles,
                                       * margin included) */
                                      const int x0 = info.y & 0xffu, x1 = (info.y >> 8) & 0xffu, y0 = (info.y >> 16) & 0xffu, y1 = info.y >> 24;
                                      bool need = false;
                                      for(int q = 0; q < nLive; q++)
                                      {
                                        if((info.x & liveGroups[q]) == 0u)
                                          continue;
                                        const int4 b = liveBox[q];
                                        if(q == gSlot)
                                          need = need || !(x1 <= b.x || x0 >= b.y || y1 <= b.z || y0 >= b.w);      /* not wholly outside */
                                        else
                                        {
                                          /* wholly inside the constant cell, or inside all four edges (the tread is turned
                                           * against the axes) */
                                          const bool in = (x0 >= b.x && x1 <= b.y && y0 >= b.z && y1 <= b.w) || grid_box_inside(segs[q], x0, x1, y0, y1);
                                          need = need || !in;
                                        }
                                      }
                                      return need;
                                    }, cellList, listScratch);
  ph.mark(1);                                               /* cell list */
  const int nGroups = (count + 3) >> 2;
  /* The groups of four listed cells go to the waves as they come free (a counter in LDS, one returning atomic per group,
   * asked for one group ahead so that its latency and the group's loads hide behind the current group's arithmetic): a
   * quarter of the list each left the block waiting 8 % of its life for its slowest wave — treads' edges cost several
   * times the ground's interior. */
  auto grab = [&]()
  {
    int v = 0;
    if(lane == 0)
      v = atomicAdd(&L.nextGroup, 1);
    return __builtin_amdgcn_readfirstlane(v);
  };
  int g = grab();
  F3 v[kPts], vn[kPts];
  const PreLane lc(Q);
  /* the coarse test "can the bottom scan see this ground pixel, can it lie outside the image?" on d (see the loop): within two
   * pixels of the border; a row from the strips' first less one on; a column within 3.5 of a strip's centre (strip: 2.5 either
   * side), as the distance of (px + 2 - x0 + 50 - 2.5) / 50 from the nearest integer */
  const float pixBorder = 0.5f - 2.0f / static_cast<float>(min(X.W, X.H));
  const float pixRowThr = 0.5f - static_cast<float>(stripRow0 - 1) / static_cast<float>(X.H);
  const float pixColA = static_cast<float>(X.W) * 0.02f;
  const float pixColB = (0.5f * static_cast<float>(X.W) + static_cast<float>(2 - stripX0 + kGroundScanStep) - 2.5f) * 0.02f + 0.5f;
  if(g < nGroups)
    load_cell<SRC>(base, cell0, cellList, 4 * g + (lane >> 4), count, lane, P.nPoints, v, D);
  while(g < nGroups)
  {
    const int gNext = grab();
    if(gNext < nGroups)
      load_cell<SRC>(base, cell0, cellList, 4 * gNext + (lane >> 4), count, lane, P.nPoints, vn, D);
    unsigned int key[kPts];
    #pragma unroll
    for(int j = 0; j < kPts; j++)
    {
      key[j] = kNoPixel;
      const F3 p{ v[j].x, v[j].y, v[j].z };
      f32x2 d;
      float M, M3;
      unsigned int q;
      unsigned long long mSlow, mCount, mGround;
      quad_decide<CHECKS, false>(p, Q, lc, L.edges, lut, qts, L.kc, gSlot, d, M, M3, q, mSlow, mCount, mGround);
      if(__builtin_amdgcn_inverse_ballot_w64(mCount))
      {
        /* calcAverageZ's summand in the reference's doubles (world_z_flat's row) */
        double wz = (P.a[6] * static_cast<double>(p.x) + P.a[7] * static_cast<double>(p.y)) + P.a[8] * static_cast<double>(p.z);
        wz = wz + P.b[2];
        if(static_cast<int>(q) != curQ)
        {
          flushAcc();
          curQ = static_cast<int>(q); accZ = 0; accN = 0;
        }
        accZ += static_cast<unsigned long long>(z_plus_magic_bits(wz));                        /* the constant's bits come off at the flush */
        accN++;
      }
      /* projectToBinaryImage(pointsInQuadri) (pointcloud.cpp:531) for the counted ground points.  Outside debug capture only the
       * pixels the bottom scan can see are wanted (above), and a pixel outside the image (quirk Q5) is counted: on the same d, a
       * point whose row lies above the strips' first by more than a pixel, or whose column lies more than a pixel off every strip,
       * and that is not within two pixels of the image's border, needs no pixel at all - five instructions say so for nineteen
       * ground points in twenty */
      unsigned long long mPixel = mCount & mGround;
      if(!FULL)
      {
        /* (no branch around these six for the waves without a counted ground point: a branch costs this loop more) */
        const unsigned long long mBorder = __ballot(M > pixBorder);
        const unsigned long long mRow = __ballot(d.y <= pixRowThr);
        const float gc = __builtin_amdgcn_fractf(__builtin_fmaf(d.x, pixColA, pixColB)) - 0.5f;
        const unsigned long long mCol = __ballot(__builtin_fabsf(gc) < 0.07f);
        mPixel &= mSlow | mBorder | (mRow & mCol);
      }
      if(FULL ? mPixel != 0ull : __builtin_expect(mPixel != 0ull, 0))
      {
        if(__builtin_amdgcn_inverse_ballot_w64(mPixel))
        {
          int ix, iy;
          const bool inside = pre_pixel(p, d, M3, X, L.kc, ix, iy);
          oob += inside ? 0u : 1u;                              /* quirk Q5 */
          if(FULL)
            key[j] = inside ? pixel_key(0, iy, ix) : kNoPixel;
          else if(inside && iy >= stripRow0)
          {
            int strip;
            bool centre;
            if(ground_strip_of(ix, stripX0, strip, centre))
            {
              /* One of the few pixels the bottom scan can see.  It looks, per scan column, for the BOTTOM-most lit pixel of the
               * closed image, which lies at or below the bottom-most raw pixel of the column itself (closing only adds) and is a
               * function of the raw rows within two of it: a pixel more than two rows above a centre-column pixel already seen
               * in its strip cannot matter and stays unwritten (round 4: the blocks run from the bottom of the camera image up,
               * so after a frame's first blocks nearly nothing is written: 4.5 k -> a few hundred global atomics per frame). */
              const int seen = SSD_CHK(24, strip, kMaxGroundStrips) ? L.stripMax[strip] : 0x7fffffff;
              if(iy >= seen - 2)
              {
                if(SSD_CHK(23, static_cast<unsigned int>(iy) * (2u * X.W64) + (static_cast<unsigned int>(ix) >> 5), 2u * static_cast<unsigned int>(X.H) * X.W64))
                  atomicOr(gimg32 + (static_cast<unsigned int>(iy) * (2u * X.W64) + (static_cast<unsigned int>(ix) >> 5)), 1u << (ix & 31));
                gy0 = min(gy0, iy);
                gy1 = max(gy1, iy);
                if(centre && iy > seen)
                  atomicMax(&L.stripMax[strip], iy);
              }
            }
          }
        }
      }
    }
    if(FULL)
      wavewin_emit(ww, wm, win, gimg, imgWords, X.W64, X.winShiftGround, box, key, lane);
    g = gNext;
#pragma unroll
    for(int j = 0; j < kPts; j++)
      v[j] = vn[j];
  }
  if(FULL)
  {
    wavewin_flush(ww, win, gimg, imgWords, X.W64, X.winShiftGround, box, lane);
    wavemiss_flush(wm, box, lane);
  }
  else
  {
    /* the rows this wave wrote; all strips of those rows are k_final's to read and to clear (word columns: the whole row) */
    gy1 = wave_max_i(gy1);
    if(gy1 >= 0)
    {
      gy0 = wave_min_i(gy0);
      if(lane == 0)
      {
        atomicMin(&box[0].yMin, gy0); atomicMax(&box[0].yMax, gy1);
        atomicMin(&box[0].xMin, 0); atomicMax(&box[0].xMax, X.W64 - 1);
      }
    }
  }
  ph.mark(2);                                               /* the walk */
  flushAcc();
  if(oob)
    atomicAdd(&lOob, oob);
  __syncthreads();
  if(!FULL && tid < kMaxGroundStrips && L.stripMax[tid] > stripMaxMine)
    atomicMax(&fs.groundStripMax[tid], L.stripMax[tid]);       /* for the frame's blocks still to come */
  ph.mark(3);                                               /* waiting for the block's other waves */
  if(tid < nLive)
  {
    unsigned long long s = 0;
    unsigned int c = 0;
    for(int k = 0; k < 8; k++)
    {
      s += lsum[tid][k];
      c += lcnt[tid][k];
    }
    if(c)
    {
      const int acc = liveAcc[tid];
      atomicAdd(reinterpret_cast<unsigned long long *>(&fs.sumZ[acc]), s);
      atomicAdd(&fs.cnt[acc], c);
    }
  }
  if(tid == 0)
  {
    if(box[0].yMax >= 0)
    {
      atomicMin(&fs.imgYMin[kMaxStepImages], box[0].yMin); atomicMax(&fs.imgYMax[kMaxStepImages], box[0].yMax);
      atomicMin(&fs.imgXMin[kMaxStepImages], box[0].xMin); atomicMax(&fs.imgXMax[kMaxStepImages], box[0].xMax);
    }
    if(lOob)
    {
      atomicAdd(&fs.nOob, lOob);
      atomicOr(&fs.status, static_cast<unsigned int>(SSD_ST_OOB_PIXEL));
    }
  }
  ph.mark(4);                                               /* sums out */
  ph.finish();
}

} // namespace ssd

/* K7 and K8 (extensions), at their place in the order of definitions: the labels, then the surface moments */
#include "ssd_k_labels.h"
#include "ssd_k_moments.h"

namespace ssd
{

/* ========================================================================= */
/* K5: ground front edge and the per-frame result — one workgroup per frame     */

/* calcAverageZ (pointcloud.cpp:574-581): sum / points.size().  A quadrilateral that accepted no point makes that 0.0 / 0.0,
 * which on the reference's x86 is the DEFAULT NaN with the sign bit SET (0xfff8...): the line then reads "-nan"
 * (stairs.cpp:43 through operator<<).  This GPU's 0.0 / 0.0 is the positive quiet NaN — so the empty case is stated, not divided. */
__device__ __forceinline__ double mean_of_fixed(long long sumFixed, unsigned int n)
{
  if(n == 0u)
    return __longlong_as_double(static_cast<long long>(0xfff8000000000000ull));
  return (static_cast<double>(sumFixed) / static_cast<double>(1ll << kZFixShift)) / n;
}

struct FinalShared
{
  int yEdge[kMaxCols];
  int px[kMaxCols], py[kMaxCols];
  int n;
  LineI line;
  double partRes[kMaxImgWaves];             /* BestLine: every wave's best over its share of the pairs */
  int partT[kMaxImgWaves];
  LineI partLine[kMaxImgWaves];
  double stepsWorld[SSD_MAX_STEPS][9];       /* z, 4 x (x,y) in camera-dependent world coordinates; thread 0 only:
                                                in LDS because a private array would live in scratch memory */
};

template<int T>
SSD_ENTRY(__launch_bounds__(T), k_final, final_block)(SSD_BYVAL(Params) P, FrameState *__restrict__ st,
                                                    unsigned long long *__restrict__ groundImg,
                                                    ssd_frame_result *__restrict__ results,
                                                    DebugFrame *__restrict__ dbg,
                                                    unsigned long long *__restrict__ dbgImg)
{
  __shared__ FinalShared S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int frame = blockIdx.x;
  FrameState &fs = st[frame];
  ssd_frame_result &res = results[frame];
  const bool threw = (fs.status & SSD_ST_THROW) != 0;
  const bool haveGround = !threw && fs.firstValidInd >= 0 && fs.groundInd >= 0;

  const size_t imgWords = static_cast<size_t>(P.H) * P.W64;
  unsigned long long *img = groundImg + static_cast<size_t>(frame) * imgWords;
  const BitImg im{ img, P.W, P.H, P.W64 };

  /* bottom-scan columns: x_j = xr0 + 50 j, centre column j = jc */
  const int xStep = kGroundScanStep;
  const int xc = P.W / 2;
  const int xr0 = ground_scan_x0(P.W);
  const int jc = xc / xStep;
  const int nCols = min(kMaxCols, (P.W - 1 - xr0) / xStep + 1);
  SSD_PHASE(2, 0);

  for(int j = tid; j < kMaxCols; j += T)
    S.yEdge[j] = -1;
  if(tid == 0)
    S.n = 0;
  /* k_inquad's record of the strips' bottom-most centre pixels has served (this frame's strip raster is complete): left at
   * "none" for whichever k_inquad comes next, also one of a partial run that k_quads — its other resetter — does not precede */
  for(int j = tid; j < kMaxGroundStrips; j += T)
    fs.groundStripMax[j] = -1;
  __syncthreads();

  if(haveGround)
  {
    /* BottomScanner::probeBottomUp (segmentation.cpp:225-241): lowest lit pixel with y > H/2 */
    const int yStop = P.H / 2;
    unsigned long long *dbgRaw = nullptr, *dbgClosed = nullptr;
    if(dbgImg)
    {
      dbgRaw = dbgImg + ((static_cast<size_t>(frame) * (P.maxStepImages + 1) + P.maxStepImages) * 2) * imgWords;
      dbgClosed = dbgRaw + imgWords;
    }
    int by0 = fs.imgYMin[kMaxStepImages], by1 = fs.imgYMax[kMaxStepImages];
    int bc0 = fs.imgXMin[kMaxStepImages], bc1 = fs.imgXMax[kMaxStepImages];
    const bool emptyImg = by1 < by0;
    grow_box_to_border(P.W, P.H, P.W64, by0, by1, bc1);
    if(dbgImg)
    {
      by0 = 0; by1 = P.H - 1; bc0 = 0; bc1 = P.W64 - 1;
    }
    else if(by0 <= yStop)
      by0 = yStop + 1;                               /* only rows below the image centre are probed */
    const int bw = (emptyImg && !dbgImg) || by1 < by0 ? 0 : bc1 - bc0 + 1, bh = by1 - by0 + 1;
    if(dbgImg)
    {
      /* debug capture: the raw and the closed image whole, word by word */
      const int nBands = bw > 0 ? max(1, T / bw) : 0;
      const int bandRows = nBands > 0 ? (bh + nBands - 1) / nBands : 0;
      for(int t = tid; t < bw * nBands; t += T)
      {
        const int band = t / bw;
        const int c = bc0 + (t - band * bw);
        const int yA = by0 + band * bandRows, yB = min(yA + bandRows, by1 + 1);
        closed_column(im, c, yA, yB, true, [&](int y, unsigned long long cw)
        {
          dbgRaw[y * P.W64 + c] = img[y * P.W64 + c];
          dbgClosed[y * P.W64 + c] = cw;
        });
      }
    }
    /* the scan columns inside the box in bands of rows, as in k_outline: the last closed row below the image centre */
    if(bw > 0)
    {
      const int yTop = max(by0, yStop + 1);
      const int nRowsBelow = by1 - yTop + 1;
      const int xLo = 64 * bc0, xHi = min(64 * bc1 + 63, P.W - 1);
      const int jLo = xLo <= xr0 ? 0 : (xLo - xr0 + xStep - 1) / xStep;
      const int jHi = xHi < xr0 ? -1 : min(nCols - 1, (xHi - xr0) / xStep);
      const int nJ = nRowsBelow > 0 ? jHi - jLo + 1 : 0;
      const int nBands = nJ > 0 ? max(1, T / nJ) : 0;
      const int bandRows = nBands > 0 ? (nRowsBelow + nBands - 1) / nBands : 0;
      for(int t = tid; t < nJ * nBands; t += T)
      {
        const int band = t / nJ;
        const int j = jLo + (t - band * nJ);
        const int yA = yTop + band * bandRows, yB = min(yA + bandRows, by1 + 1);
        int yHi = -1;
        closed_scan_column(im, xr0 + xStep * j, yA, yB, [&](int y) { yHi = y; });
        if(yHi >= 0)
          atomicMax(&S.yEdge[j], yHi);
      }
    }
    __syncthreads();
    SSD_PHASE(2, 1);

    /* BottomScanner::scan (:170-222): first hit rightwards from the centre (else leftwards), then
     * contiguous hits to the right of it, then to the left of it */
    {
      /* every wave for itself: the columns' hit bits by ballot, the run around the first hit by bit scans */
      const bool h0 = lane < nCols && S.yEdge[lane] >= 0, h1 = lane + 64 < nCols && S.yEdge[lane + 64] >= 0;
      const unsigned long long hLo = __ballot(h0), hHi = __ballot(h1);
      auto hitAt = [&](int j) { return j >= 0 && j < nCols && (((j < 64 ? hLo : hHi) >> (j & 63)) & 1ull) != 0ull; };
      int jStart = jc;
      while(jStart < nCols && !hitAt(jStart))
        jStart++;
      if(jStart >= nCols)
      {
        jStart = jc - 1;
        while(jStart >= 0 && !hitAt(jStart))
          jStart--;
      }
      int nRight = 0, nLeft = 0;                 /* hits to the right of the start column, to the left of it */
      if(jStart >= 0)
      {
        while(hitAt(jStart + 1 + nRight))
          nRight++;
        while(hitAt(jStart - 1 - nLeft))
          nLeft++;
      }
      const int n = jStart >= 0 ? 1 + nRight + nLeft : 0;
      /* point k: the start column, then rightwards, then leftwards */
      for(int k = tid; k < n; k += T)
      {
        const int j = k <= nRight ? jStart + k : jStart - (k - nRight);
        S.px[k] = xr0 + xStep * j;
        S.py[k] = S.yEdge[j];
      }
      if(tid == 0)
        S.n = n;
    }
    __syncthreads();
    SSD_PHASE(2, 2);
    if(S.n >= 2)
    {
      /* BestLine: the pairs dealt out over the block's waves, the waves' bests combined in pair order */
      double res;
      int t;
      LineI l;
      wave_best_line_part(S.px, S.py, S.n, lane, 3ll * P.W * P.H < (1ll << 25), 64 * wave, T, res, t, l);
      if(lane == 0)
      {
        S.partRes[wave] = res;
        S.partT[wave] = t;
        S.partLine[wave] = l;
      }
    }
    __syncthreads();
    if(S.n >= 2 && tid == 0)
    {
      int best = -1;
      for(int w = 0; w < T / 64; w++)
        if(S.partT[w] != 0x7fffffff && (best < 0 || S.partRes[w] < S.partRes[best] || (S.partRes[w] == S.partRes[best] && S.partT[w] < S.partT[best])))
          best = w;
      S.line = best >= 0 ? S.partLine[best] : LineI{ 0, 0, 0 };
    }
    __syncthreads();
  }
  SSD_PHASE(2, 3);

  /* ---- the emitted surfaces, one lane each (wave 0): lane 0 the ground (calcGround, pointcloud.cpp:528-547), lane 1 + i the
   *      plateau firstValidInd + i (calcStairStep :549-558); every lane fetches its own sums and corners (one round trip
   *      for all), its place in the result is the count of emitted surfaces before it; then the detectStairs tail
   *      (:370-383): ToExternalWorld (transformation.cpp:190-194), straight from the lane's registers ---- */
  static_assert(kMaxPlateaus + 1 <= 64 && SSD_MAX_STEPS <= 64, "one lane per surface");
  if(wave == 0)
  {
    const bool any = !threw && fs.firstValidInd >= 0;
    const int firstValidInd = fs.firstValidInd, firstStep = fs.firstStep, last = fs.firstStep + fs.nStepImages;
    const bool groundLane = any && lane == 0 && fs.groundInd >= 0;
    const int k = firstValidInd + lane - 1;
    const bool stepLane = any && lane >= 1 && k < last && fs.pl[k < last ? max(k, 0) : 0].valid;
    double sW[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };         /* z, 4 x (x, y): camera-dependent world coordinates */
    if(groundLane)
    {
      /* "return {}" when no front edge is found (quirk Q6): the ground stays all zero */
      const bool valid = S.n >= 2;
      fs.groundFrontValid = valid ? 1 : 0;
      const double meanZ = mean_of_fixed(fs.sumZ[kGroundAcc], fs.cnt[kGroundAcc]);
      double fimg[4] = { 0, 0, 0, 0 };
      if(valid)
      {
        /* detectFrontEdge tail (segmentation.cpp:896-906) */
        const LineI l = S.line;
        const double fm = static_cast<double>(-l.a) / l.b, fn = static_cast<double>(-l.c) / l.b;
        int xl = S.px[0], xr = S.px[0];
        for(int i = 1; i < S.n; i++) { xl = min(xl, S.px[i]); xr = max(xr, S.px[i]); }
        fimg[0] = xl; fimg[1] = xl * fm + fn;
        fimg[2] = xr; fimg[3] = xr * fm + fn;
        const double flx = P.xMin + fimg[0] * P.xToWorld, fly = P.yMax - fimg[1] * P.yToWorld;
        const double frx = P.xMin + fimg[2] * P.xToWorld, fry = P.yMax - fimg[3] * P.yToWorld;
        const LineD frontLine = line_through_d(flx, fly, frx, fry);
        const double *g = fs.groundQuadWorld;
        const LineD leftSide = line_through_d(g[0], g[1], g[4], g[5]);
        const LineD rightSide = line_through_d(g[2], g[3], g[6], g[7]);
        /* StairsDetector::Line::intersection (pointcloud.cpp:520-525) */
        const double dl = frontLine.a * leftSide.b - leftSide.a * frontLine.b;
        const double dr = frontLine.a * rightSide.b - rightSide.a * frontLine.b;
        sW[0] = meanZ;
        sW[1] = (frontLine.b * leftSide.c - leftSide.b * frontLine.c) / dl;
        sW[2] = (leftSide.a * frontLine.c - frontLine.a * leftSide.c) / dl;
        sW[3] = (frontLine.b * rightSide.c - rightSide.b * frontLine.c) / dr;
        sW[4] = (rightSide.a * frontLine.c - frontLine.a * rightSide.c) / dr;
        sW[5] = g[4]; sW[6] = g[5];
        sW[7] = g[6]; sW[8] = g[7];
      }
      if(dbg)
      {
        ssd_debug_frame &d = dbg[frame].d;
        d.ground_front_valid = valid ? 1 : 0;
        d.ground_n_in_quad = static_cast<int>(fs.cnt[kGroundAcc]);
        d.ground_mean_z = meanZ;
        d.ground_n_pts = S.n;
        for(int i = 0; i < S.n; i++) { d.ground_pts[i][0] = S.px[i]; d.ground_pts[i][1] = S.py[i]; }
        if(valid)
        {
          d.ground_line[0] = S.line.a; d.ground_line[1] = S.line.b; d.ground_line[2] = S.line.c;
          for(int i = 0; i < 4; i++) d.ground_front_img[i] = fimg[i];
        }
      }
    }
    if(stepLane)
    {
      /* calcAverageZ over the plateau's points inside its quadrilateral = all of them (k_raster's sum, the histogram's
       * count) minus the ones outside (k_inquad's sum and count) */
      const long long inZ = fs.totZ[k - firstStep] - fs.sumZ[k];
      const unsigned int inN = static_cast<unsigned int>(fs.pl[k].nPoints) - fs.cnt[k];
      const double meanZ = mean_of_fixed(inZ, inN);
      sW[0] = meanZ;
#pragma unroll
      for(int c = 0; c < 8; c++)
        sW[1 + c] = fs.pl[k].quadWorld[c];
      if(dbg)
      {
        ssd_debug_plateau &p = dbg[frame].d.plateaus[k];
        p.n_in_quad = static_cast<int>(inN);
        p.sum_z_fix = inZ;
        p.mean_z = meanZ;
      }
    }
    const unsigned long long emitted = __ballot(groundLane || stepLane);
    const int place = __popcll(emitted & ((1ull << lane) - 1ull));
    const int n = min(__popcll(emitted), SSD_MAX_STEPS);
    if((groundLane || stepLane) && place < SSD_MAX_STEPS)
    {
      /* transformation.cpp:209-211; a NaN mean keeps its sign through the sum on x86 (the operand NaN is propagated) */
      res.steps[place].height = sW[0] != sW[0] ? sW[0] : P.worldZ + sW[0];
#pragma unroll
      for(int c = 0; c < 4; c++)
      {
        const double x = sW[1 + 2 * c], y = sW[2 + 2 * c];
        double ex = P.r2[0] * x + P.r2[1] * y;
        double ey = P.r2[2] * x + P.r2[3] * y;
        ex = ex + P.t2[0];
        ey = ey + P.t2[1];
        res.steps[place].quad[2 * c] = ex;
        res.steps[place].quad[2 * c + 1] = ey;
      }
#pragma unroll
      for(int c = 0; c < 9; c++)
        S.stepsWorld[place][c] = sW[c];              /* for the risers below */
    }
    if(lane >= n && lane < SSD_MAX_STEPS)            /* unused slots are zero, so results compare bytewise */
    {
      res.steps[lane].height = 0.0;
#pragma unroll
      for(int c = 0; c < 8; c++)
        res.steps[lane].quad[c] = 0.0;
    }
    if(lane == 0)
    {
      S.n = n;                                       /* from here on: the number of emitted surfaces */
      res.n_steps = n;
      res.status = static_cast<int>(fs.status);
      if(dbg)
      {
        dbg[frame].d.status = static_cast<int>(fs.status);
        dbg[frame].d.n_oob = static_cast<int>(fs.nOob);
      }
    }
  }
  SSD_PHASE(2, 4);
  __syncthreads();
  if(P.risers && tid == 0)
  {
    const int n = S.n;
    double (&stepsWorld)[SSD_MAX_STEPS][9] = S.stepsWorld;
    {
      /* vertical faces (extension, include/ssd_hip.h): one riser under the front edge of every emitted surface but
       * the lowest; its evidence is gathered by k_risers from the bins of no plateau between the two heights */
      for(int b = 0; b < kMaxBins; b++)
        fs.riserOfBin[b] = -1;
      unsigned int wanted = 0u;
      const int nR = n > 1 ? n - 1 : 0;
      for(int i = 0; i < nR; i++)
      {
        const double *lower = stepsWorld[i], *upper = stepsWorld[i + 1];
        RiserState &R = fs.riser[i];
        R.leftX = upper[1]; R.leftY = upper[2]; R.rightX = upper[3]; R.rightY = upper[4];
        R.zBottom = lower[0]; R.zTop = upper[0];
        const double dx = R.rightX - R.leftX, dy = R.rightY - R.leftY;
        const double len = sqrt(dx * dx + dy * dy);
        R.ox = R.leftX; R.oy = R.leftY;
        R.zLo = lower[0] + P.heightInterval;
        R.zHi = upper[0] - P.heightInterval;
        const bool usable = len > 0.0 && R.zLo < R.zHi;
        R.ux = usable ? dx / len : 0.0;
        R.uy = usable ? dy / len : 0.0;
        R.len = usable ? len : -1.0;                        /* no point has 0 <= t <= -1 */
        if(usable)
        {
          int bLo = static_cast<int>((R.zLo - P.zMin) * P.pt.recip), bHi = static_cast<int>((R.zHi - P.zMin) * P.pt.recip);
          bLo = max(0, min(bLo, P.nBins - 1));
          bHi = max(0, min(bHi, P.nBins - 1));
          for(int b = bLo; b <= bHi; b++)
            if(fs.lut[b] == 0xff && fs.riserOfBin[b] < 0)
            {
              fs.riserOfBin[b] = static_cast<signed char>(i);
              wanted |= 1u << (b / kBinsPerGroup);
            }
        }
      }
      for(int i = 0; i < kMaxRisers; i++)
      {
        fs.rSum[i] = 0;
        fs.rCnt[i] = 0u;
      }
      fs.nRisers = nR;
      fs.wantedRisers = wanted;
    }
  }
  __syncthreads();
  SSD_PHASE(2, 5);

  /* leave the ground image zeroed for the next batch (all its bits lie inside the bounding box) */
  if(fs.imgYMax[kMaxStepImages] >= fs.imgYMin[kMaxStepImages])
  {
    const int cy0 = fs.imgYMin[kMaxStepImages], cc0 = fs.imgXMin[kMaxStepImages];
    const int cw = fs.imgXMax[kMaxStepImages] - cc0 + 1, ch = fs.imgYMax[kMaxStepImages] - cy0 + 1;
    if(P.px.groundFull)
    {
      for(int idx = tid; idx < cw * ch; idx += T)
      {
        const int ry = idx / cw;
        const size_t o = static_cast<size_t>(cy0 + ry) * P.W64 + cc0 + (idx - ry * cw);
        if(SSD_CHK(22, o, static_cast<size_t>(P.H) * P.W64))
          img[o] = 0ull;                                 /* unconditionally: a load first would make every word a round trip */
      }
    }
    else
    {
      /* k_inquad set strip pixels only (ground_strip_column: within two of x_j for ANY integer j, also j = -1 and one past the
       * last scanned column): the one or two 32-bit words of every such strip, rows cy0 .. */
      unsigned int *img32 = reinterpret_cast<unsigned int *>(img);
      const int nStrips = (P.W - 1 + 2 - xr0) / xStep + 3;           /* j = -1 .. (W + 1 - xr0) / 50 */
      const int words32 = 2 * P.W64;
      for(int idx = tid; idx < ch * nStrips * 2; idx += T)
      {
        const int ry = idx / (nStrips * 2), rest = idx - ry * (nStrips * 2);
        const int x = xr0 + xStep * ((rest >> 1) - 1) + ((rest & 1) ? 2 : -2);
        const int w = x >> 5;                                          /* arithmetic shift: negative stays negative */
        if(x >= 0 && w < words32)
          img32[static_cast<size_t>(cy0 + ry) * words32 + w] = 0u;
      }
    }
  }
  SSD_PHASE(2, 6);
}

} // namespace ssd

/* K6 (extension), the riser passes: behind every other stage, so that k_riser_results stays the unit's last kernel that is no template */
#include "ssd_k_risers.h"


#include "ssd_launch_rules.h"

/* What follows is the one-calibration path's own, and the one stretch that an including unit leaves out: the entry points that call a
 * stage's *_block with blockIdx, as ssd_kernels_cams.hip's call it with the frame's camera record, and the launchers. */
#ifndef SSD_CAMERAS_TU
namespace ssd
{

template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads, 6) void k_hist(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q,
                                                   FrameState *__restrict__ st, uint2 *__restrict__ tileMasks,
                                                   size_t tileMaskStride, int chunkPoints, DepthSrc D)
{
  __shared__ HistLds L;
  NoSpecLds none;
  hist_block<SRC, false, false, CHECKS>(L, none, xyz, strideFloats, P, Q, PixelParams{}, st, tileMasks, nullptr, tileMaskStride, chunkPoints, D, blockIdx.x, blockIdx.y);   /* frame on the fast grid axis: see launch note on XCD balance */
}

/* K1 of a single-pass batch: histogram, cell records AND the planes of the candidate bins.  31 KiB of LDS: five blocks per CU
 * (4 .. 6 measure the same). */
template<int SRC, bool STRIPS, bool CHECKS>
__global__ __launch_bounds__(kThreads, SSD_K1S_WAVES) void k_hist_planes(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q, PixelParams X,
                                                   FrameState *__restrict__ st, uint2 *__restrict__ tileMasks,
                                                   unsigned long long *__restrict__ planeImg,
                                                   size_t tileMaskStride, int chunkPoints, DepthSrc D)
{
  __shared__ HistLds L;
  __shared__ SpecLds SL;
  /* (other walks of the (frame, chunk) grid than "frame fast" - frames walking their chunks in rotated orders, a frame's chunks in a
   * row over all XCDs, each XCD a frame at a time - changed nothing: profiles/r06_k1_variants.txt (d), profiles/r06_box_spread.txt;
   * the code: commit ad9a851) */
  const int chunkIdx = static_cast<int>(blockIdx.y);
  const int frameIdx = static_cast<int>(blockIdx.x);
  hist_block<SRC, true, STRIPS, CHECKS>(L, SL, xyz, strideFloats, P, Q, X, st, tileMasks, planeImg, tileMaskStride, chunkPoints, D, frameIdx, chunkIdx);
}

/* K0; launch_predict picks by needs_checks(), as launch_hist does */
template<int SRC>
__global__ __launch_bounds__(kThreads) void k_predict(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q, FrameState *__restrict__ st, DepthSrc D,
                                                      int minHeight, int sabotage, int *__restrict__ fallback, int poolPlanes)
{
  predict_block<SRC, false>(xyz, strideFloats, P, Q, st, D, minHeight, sabotage, fallback, poolPlanes);
}
template<int SRC>
__global__ __launch_bounds__(kThreads) void k_predict_checks(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q, FrameState *__restrict__ st, DepthSrc D,
                                                             int minHeight, int sabotage, int *__restrict__ fallback, int poolPlanes)
{
  predict_block<SRC, true>(xyz, strideFloats, P, Q, st, D, minHeight, sabotage, fallback, poolPlanes);
}

/* LIST (single pass): the grid's x blocks share the frames k_peaks listed in `fallback` (count, then frame indices) - the
 * frames whose step plateaus the planes did not cover; none, as a rule, and then every block leaves after one cached load.
 * A template flag, not a run-time test: with both forms in one kernel the two-pass instantiation - the one every depth-16,
 * small, backed-off or partial call takes - paid for the list's loop with 13 - 17 vector registers in scratch (round 4).  The
 * list's own instantiation runs a handful of frames per batch: built for five waves per SIMD, which leaves it the registers
 * its loop wants (no scratch either). */
template<int SRC, bool LIST>
__global__ __launch_bounds__(kThreads, LIST ? 5 : SSD_K2_WAVES) void k_raster(const float *__restrict__ xyz, size_t strideFloats, PointParams P,
                                                        PixelParams X, FrameState *__restrict__ st,
                                                        unsigned long long *__restrict__ stepImg,
                                                        const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints, DepthSrc D,
                                                        const int *__restrict__ fallback)
{
  __shared__ RasterLds L;
  if constexpr(LIST)
  {
    const int n = fallback[0];
    for(int e = blockIdx.x; e < n; e += gridDim.x)
    {
      raster_block<SRC>(L, xyz, strideFloats, P, X, st, stepImg, tileMasks, tileMaskStride, chunkPoints, D, fallback[kFallbackList + e], blockIdx.y);
      __syncthreads();
    }
  }
  else
    raster_block<SRC>(L, xyz, strideFloats, P, X, st, stepImg, tileMasks, tileMaskStride, chunkPoints, D, blockIdx.x, blockIdx.y);
}

template<int SRC, bool FULL, bool CHECKS>
__global__ __launch_bounds__(kThreads, FULL ? 4 : SSD_K4_WAVES) void k_inquad(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q,
                                                        PixelParams X, FrameState *__restrict__ st,
                                                        unsigned long long *__restrict__ groundImg,
                                                        const uint2 *__restrict__ tileMasks, size_t tileMaskStride, int chunkPoints, DepthSrc D)
{
  __shared__ InquadLds<FULL> L;
  /* The chunks at the bottom of the camera image first (an eighth of them, bottom-most first): the ground nearest to the camera,
   * whose pixels decide what the strip raster may leave out (see there); then the others top-down as ever.  (All chunks
   * bottom-up: XGA 0.79 -> 0.73 ms like this order, FHD stress 0.55 -> 0.59 — its eight treads, the heavy blocks, came last.) */
  const int nChunks = static_cast<int>(gridDim.y), first = max(1, nChunks / 8), by = static_cast<int>(blockIdx.y);
  const int chunkIdx = by < first ? nChunks - 1 - by : by - first;
  inquad_block<SRC, FULL, CHECKS>(L, xyz, strideFloats, P, Q, X, st, groundImg, tileMasks, tileMaskStride, chunkPoints, D, blockIdx.x, chunkIdx);
}

template<int SRC, bool CHECKS>
__global__ __launch_bounds__(kThreads) void k_surface_moments(const float *__restrict__ xyz, size_t strideFloats, PointParams P, PreXY Q,
                                                              const FrameState *__restrict__ st, const uint2 *__restrict__ tileMasks,
                                                              size_t tileMaskStride, int chunkPoints, DepthSrc D,
                                                              ssd_frame_moments *__restrict__ out)
{
  __shared__ SurfaceLds S;
  labelled_moments_block<SRC, CHECKS, false>(S, nullptr, xyz, strideFloats, P, Q, st, tileMasks, tileMaskStride, chunkPoints, D, nullptr, out);
}

void launch_predict(const Batch &B, int *fallback, int poolPlanes, int sabotage)
{
  if(B.cams)
    return launch_predict_cams(B, fallback, poolPlanes, sabotage);
  const Params &P = B.P;
  with_predict(B, [&](auto src, auto checks, const DepthSrc &D)
  {
    constexpr int SRC = decltype(src)::value;
    if constexpr(decltype(checks)::value)
      hipLaunchKernelGGL(k_predict_checks<SRC>, grid_predict(B), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.pre, B.st, D, P.minHeight, sabotage, fallback, poolPlanes);
    else
      hipLaunchKernelGGL(k_predict<SRC>, grid_predict(B), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.pre, B.st, D, P.minHeight, sabotage, fallback, poolPlanes);
  });
}
void launch_hist(const Batch &B, int chunkPoints, unsigned long long *planeImg)
{
  if(B.cams)
    return launch_hist_cams(B, chunkPoints, planeImg);
  const Params &P = B.P;
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &D)
  {
    constexpr int SRC = decltype(src)::value;
    constexpr bool CHECKS = decltype(checks)::value;
    if(planeImg)
      with_bool(hist_strips(B, planeImg), [&](auto sorted)
      {
        hipLaunchKernelGGL((k_hist_planes<SRC, decltype(sorted)::value, CHECKS>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.pre, P.px, B.st, B.tileMasks, planeImg, B.tileMaskStride, chunkPoints, D);
      });
    else
      hipLaunchKernelGGL((k_hist<SRC, CHECKS>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.pre, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, D);
  });
}
void launch_peaks(const Batch &B, DebugFrame *dbg, int *fallback)
{
  if(B.cams)
    return launch_peaks_cams(B, dbg, fallback);
  hipLaunchKernelGGL(k_peaks, grid_frames(B), dim3(64), 0, B.s, B.P, B.st, B.nframes, dbg, fallback ? 1 : 0, fallback);
}
void launch_raster(const Batch &B, int chunkPoints, unsigned long long *stepImg, const int *fallback)
{
  if(B.cams)
    return launch_raster_cams(B, chunkPoints, stepImg, fallback);
  with_src(B, [&](auto src, const DepthSrc &D)
  {
    with_bool(fallback != nullptr, [&](auto listed)
    {
      hipLaunchKernelGGL((k_raster<decltype(src)::value, decltype(listed)::value>), grid_raster(B, chunkPoints, fallback != nullptr), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.P.pt, B.P.px, B.st, stepImg, B.tileMasks, B.tileMaskStride, chunkPoints, D, fallback);
    });
  });
}
void launch_outline(const Batch &B, unsigned long long *stepImg, unsigned long long *planeImg, DebugFrame *dbg, unsigned long long *dbgImg)
{
  if(B.cams)
    return launch_outline_cams(B, stepImg, planeImg, dbg, dbgImg);
  with_img_threads(B, [&](auto t)
  {
    hipLaunchKernelGGL(k_outline<decltype(t)::value>, grid_images(B), dim3(decltype(t)::value), 0, B.s, B.P, B.st, stepImg, planeImg, dbg, dbgImg);
  });
}
void launch_quads(const Batch &B, DebugFrame *dbg)
{
  if(B.cams)
    return launch_quads_cams(B, dbg);
  hipLaunchKernelGGL(k_quads, grid_frames(B), dim3(64), 0, B.s, B.P, B.st, B.nframes, dbg);
}
void launch_inquad(const Batch &B, int chunkPoints, unsigned long long *groundImg)
{
  if(B.cams)
    return launch_inquad_cams(B, chunkPoints, groundImg);
  const Params &P = B.P;
  with_inquad(B, [&](auto src, auto full, auto checks, const DepthSrc &D)
  {
    hipLaunchKernelGGL((k_inquad<decltype(src)::value, decltype(full)::value, decltype(checks)::value>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.pre, P.px, B.st, groundImg, B.tileMasks, B.tileMaskStride, chunkPoints, D);
  });
}
void launch_final(const Batch &B, unsigned long long *groundImg, ssd_frame_result *results, DebugFrame *dbg, unsigned long long *dbgImg)
{
  if(B.cams)
    return launch_final_cams(B, groundImg, results, dbg, dbgImg);
  with_img_threads(B, [&](auto t)
  {
    hipLaunchKernelGGL(k_final<decltype(t)::value>, grid_frames(B), dim3(decltype(t)::value), 0, B.s, B.P, B.st, groundImg, results, dbg, dbgImg);
  });
}
void launch_labels(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride)
{
  if(B.cams)
    return launch_labels_cams(B, chunkPoints, labels, labelStride);
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &D)
  {
    hipLaunchKernelGGL((k_labels<decltype(src)::value, decltype(checks)::value>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.P.pt, B.P.pre, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, D, labels, labelStride);
  });
}
void launch_surface_moments(const Batch &B, int chunkPoints, ssd_frame_moments *out)
{
  if(B.cams)
    return launch_surface_moments_cams(B, chunkPoints, out);
  with_src_checks(B, [&](auto src, auto checks, const DepthSrc &D)
  {
    hipLaunchKernelGGL((k_surface_moments<decltype(src)::value, decltype(checks)::value>), grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, B.P.pt, B.P.pre, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, D, out);
  });
}
static void launch_riser_results(const Batch &B, ssd_frame_risers *out)
{
  hipLaunchKernelGGL(k_riser_results, grid_frame_threads(B), dim3(64), 0, B.s, B.P, B.st, out, B.nframes);
}
void launch_risers(const Batch &B, int chunkPoints, ssd_frame_risers *out)
{
  if(B.cams)
    return launch_risers_cams(B, chunkPoints, out);
  const Params &P = B.P;
  with_src(B, [&](auto src, const DepthSrc &D)
  {
    hipLaunchKernelGGL(k_risers<decltype(src)::value>, grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.riserTol, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, P.px.cellCols, D);
  });
  launch_riser_results(B, out);
}
void launch_riser_moments(const Batch &B, int chunkPoints, ssd_frame_risers *out, ssd_frame_moments *moments)
{
  if(B.cams)
    return launch_riser_moments_cams(B, chunkPoints, out, moments);
  const Params &P = B.P;
  with_src(B, [&](auto src, const DepthSrc &D)
  {
    hipLaunchKernelGGL(k_riser_moments<decltype(src)::value>, grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.riserTol, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, P.px.cellCols, D, moments);
  });
  launch_riser_results(B, out);
}
void launch_riser_labels(const Batch &B, int chunkPoints, unsigned char *labels, size_t labelStride)
{
  if(B.cams)
    return launch_riser_labels_cams(B, chunkPoints, labels, labelStride);
  const Params &P = B.P;
  with_src(B, [&](auto src, const DepthSrc &D)
  {
    hipLaunchKernelGGL(k_riser_labels<decltype(src)::value>, grid_stream(B, chunkPoints), dim3(kThreads), 0, B.s, B.xyz, B.strideFloats, P.pt, P.riserTol, B.st, B.tileMasks, B.tileMaskStride, chunkPoints, P.px.cellCols, D, labels, labelStride);
  });
}

} // namespace ssd

#ifdef SSD_COUNT
/* tools only: reads and clears K1's counters (tiles, tiles with candidates, window moves, words flushed, pixels, pixels that missed, candidate points) */
extern "C" int ssd_tools_k1_counters(unsigned long long *out)
{
  unsigned long long zero[8] = { 0 };
  if(hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out, HIP_SYMBOL(ssd::ssd_k1_counters), sizeof(zero)) != hipSuccess)
    return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(ssd::ssd_k1_counters), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif

#include "ssd_phase_readers.h"
#endif /* SSD_CAMERAS_TU */
