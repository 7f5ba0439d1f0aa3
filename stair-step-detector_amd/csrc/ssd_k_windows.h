/* ssd_k_windows.h - LDS image windows, pixel keys, fixed-point z, the single pass's plane window (specwin_*): shared by K1, K2 and K4.
 * Device code of the per-frame path, cut by stage: DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_WINDOWS_H_
#define SSD_K_WINDOWS_H_
#include "ssd_k_cells.h"

namespace ssd
{

/* ========================================================================= */
/* LDS image windows, pixel keys, fixed-point z: shared by K1 (single pass), K2 and K4 */

/* Write-combining LDS windows for the rasterising kernels — one per WAVE, no barriers.
 *
 * Setting one bit per point with global atomics costs more than the whole fp64 path (memory-side atomics:
 * ~1.9 ms of K2's 3.8 ms per 1024 XGA frames, profiles/r01).  A wave owns 256 consecutive camera pixels of
 * every camera row of its block's chunk; on one plateau those land on a patch of a few 64-bit word columns
 * that creeps down the top-down image by one or two rows per camera row.  So each wave keeps a window of
 * kWinRows x kWinCols words of ONE image (slot, row0, col0 — wave-uniform) in LDS, ORs bits into it with LDS
 * atomics (no global traffic, no vmcnt) and writes the non-zero words out with global atomics only when the
 * window moves and at the end.  Bits outside the window go straight to memory, so the result never depends
 * on where the window is; when more lanes missed than hit during a tile the wave flushes and re-anchors at
 * the lowest missing (image, row).  Everything is decided with ballots and shuffles inside the wave. */
constexpr int kWinWords = 256;      /* 2 KiB per wave; shaped (256 >> winShift) rows x (1 << winShift) word columns, see PixelParams::winShift */

struct ImageBox { int yMin, yMax, xMin, xMax; };

struct WaveWindow
{
  int slot = -1, row0 = 0, col0 = 0;     /* wave-uniform */
  unsigned int limitWords = 0xffffffffu; /* 64-bit words of the frame's images behind `images` (SSD_CHECKED builds compare) */
};

/* Bits that miss the window go straight to memory; their bounding box is kept per WAVE in LDS (wm[2..5] = row min /
 * max, word column min / max; wm[6] = the image slots touched; wm[0..1], wm[7] unused): four LDS
 * min/max per miss, no per-lane state.  One box for all slots of the wave: a wave that misses in several images
 * (outliers) widens each of them to the union — boxes only bound the region K3 / K5 visit and clear. */
constexpr int kWaveMissWords = 8;
__device__ __forceinline__ void wavemiss_init(unsigned int *wm)
{
  wm[0] = 0xffffffffu; wm[1] = 0u;
  wm[2] = 0x7fffffffu; wm[3] = 0xffffffffu;              /* as int: INT_MAX, -1 */
  wm[4] = 0x7fffffffu; wm[5] = 0xffffffffu;
  wm[6] = 0u; wm[7] = 0u;
}
/* end of the kernel, whole wave: the wave's miss box into the block's per-slot boxes */
__device__ __forceinline__ void wavemiss_flush(unsigned int *wm, ImageBox *boxes, int lane)
{
  const unsigned int slots = wm[6];
  if(lane < 32 && ((slots >> lane) & 1u))
  {
    const int *b = reinterpret_cast<const int *>(wm);
    atomicMin(&boxes[lane].yMin, b[2]); atomicMax(&boxes[lane].yMax, b[3]);
    atomicMin(&boxes[lane].xMin, b[4]); atomicMax(&boxes[lane].xMax, b[5]);
  }
}

/* signed minimum / maximum over the wave: rows by DPP, the four rows by v_readlane */
__device__ __forceinline__ int wave_min_i(int v)
{
  v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x128, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x124, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x122, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(0x7fffffff, v, 0x121, 0xf, 0xf, false));
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wave_max_i(int v)
{
  v = max(v, __builtin_amdgcn_update_dpp(static_cast<int>(0x80000000u), v, 0x128, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(static_cast<int>(0x80000000u), v, 0x124, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(static_cast<int>(0x80000000u), v, 0x122, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(static_cast<int>(0x80000000u), v, 0x121, 0xf, 0xf, false));
  return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

/* writes the wave's window out (non-zero words only), clears it, extends the image's bounding box; all 64 lanes */
__device__ __forceinline__ void wavewin_flush(unsigned long long *ww, const WaveWindow &w, unsigned long long *__restrict__ images,
                                              unsigned int imgWords, int W64, int winShift, ImageBox *boxes, int lane)
{
  if(w.slot < 0)
    return;
  unsigned long long *img = images + static_cast<size_t>(w.slot) * imgWords;
  int y0 = 0x7fffffff, y1 = -1, x0 = 0x7fffffff, x1 = -1;
#pragma unroll
  for(int k = 0; k < kWinWords / 64; k++)
  {
    const int i = k * 64 + lane;
    const unsigned long long v = ww[i];
    if(v)
    {
      const int y = w.row0 + (i >> winShift), x = w.col0 + (i & ((1 << winShift) - 1));
      if(SSD_CHK(1, static_cast<size_t>(w.slot) * imgWords + static_cast<size_t>(y) * W64 + x, w.limitWords) && SSD_CHK(2, x, W64))
        atomicOr(img + static_cast<size_t>(y) * W64 + x, v);
      ww[i] = 0ull;
      y0 = min(y0, y); y1 = max(y1, y);
      x0 = min(x0, x); x1 = max(x1, x);
    }
  }
  y1 = wave_max_i(y1);
  if(y1 >= 0)
  {
    y0 = wave_min_i(y0); x0 = wave_min_i(x0); x1 = wave_max_i(x1);
    if(lane == 0)
    {
      atomicMin(&boxes[w.slot].yMin, y0); atomicMax(&boxes[w.slot].yMax, y1);
      atomicMin(&boxes[w.slot].xMin, x0); atomicMax(&boxes[w.slot].xMax, x1);
    }
  }
}

/* A lit pixel as one sortable word: image slot (5 bits) | row (13) | column (13); width and height <= 8192 (ssd_create).
 * kNoPixel sorts last.  (key >> 6) names the pixel's 64-bit image word. */
constexpr unsigned int kNoPixel = 0xffffffffu;
__device__ __forceinline__ unsigned int pixel_key(int slot, int iy, int ix)
{
  return (static_cast<unsigned int>(slot) << 26) | (static_cast<unsigned int>(iy) << 13) | static_cast<unsigned int>(ix);
}

/* minimum over the wave, the same in every lane (and uniform to the compiler): the rows by DPP, the four rows by v_readlane
 * (round 4: six ds_bpermute steps per value) */
__device__ __forceinline__ unsigned int wave_min_u32(unsigned int v)
{
  v = row_min_u32(v);
  return min(min(static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(v), 0)), static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(v), 16))),
             min(static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(v), 32)), static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(v), 48))));
}

/* The window's origin as a pixel_key (slot, row0, 64 * col0): for a pixel key k of the same image at or beyond the origin,
 * d = k - base is (row - row0) << 13 | (column - 64 * col0); a pixel of another image, a higher row, or a column left of
 * the origin borrows into the upper fields and fails the bounds below (64 * col0 + window width <= 8192), so one
 * subtraction and two compares decide "inside the window".  kNoWindow (bit 31, which no pixel key has) fails for all. */
constexpr unsigned int kNoWindow = 0x80000000u;
__device__ __forceinline__ unsigned int window_base(const WaveWindow &w)
{
  return w.slot < 0 ? kNoWindow : pixel_key(w.slot, w.row0, w.col0 << 6);
}
/* rows (kWinWords >> winShift) and pixel columns (64 << winShift) of a window are powers of two, so "row offset below the
 * rows and column offset below the columns" is "d has no bit outside the two offset fields": one AND and one compare with
 * zero (round 3: two shifts / masks and two compares) */
__device__ __forceinline__ bool window_hit(unsigned int d, int winShift)
{
  const unsigned int inside = (((static_cast<unsigned int>(kWinWords) >> winShift) - 1u) << 13) | ((64u << winShift) - 1u);
  return (d & ~inside) == 0u;
}

/* Before a tile's pixels go out, all 64 lanes; `first` = the lane's lowest pixel_key of this tile (kNoPixel: none).
 * When more than half of the lanes that have pixels would miss the window, it is flushed and re-anchored at the lowest
 * such key FIRST — deciding only after the tile had gone out (round 1 / 2a) sent every wave's first tile and the tile
 * after each change of cell column straight to memory: 10.5 % of all words, 2.2 % now (tools/window_sim.py). */
__device__ __forceinline__ void wavewin_prepare(unsigned long long *ww, WaveWindow &w, unsigned long long *__restrict__ images,
                                                unsigned int imgWords, int W64, int winShift, ImageBox *boxes, unsigned int first, int lane)
{
  const bool has = first != kNoPixel;
  const bool miss = has && !window_hit(first - window_base(w), winShift);
  const unsigned long long missing = __ballot(miss);
  if(missing == 0ull || 2 * __popcll(missing) <= __popcll(__ballot(has)))
    return;
  const unsigned int lowest = __builtin_amdgcn_readfirstlane(wave_min_u32(miss ? first : kNoPixel));
  wavewin_flush(ww, w, images, imgWords, W64, winShift, boxes, lane);
  w.slot = static_cast<int>(lowest >> 26);
  w.row0 = static_cast<int>((lowest >> 13) & 0x1fffu);
  w.col0 = max(0, min(static_cast<int>((lowest & 0x1fffu) >> 6) - 1, W64 - (1 << winShift)));
}

/* A lane's (up to four) pixels of one tile, as keys; all 64 lanes (wavewin_prepare votes).  One 32-bit LDS atomic per pixel
 * (the window's 64-bit words as pairs of halves), no merging of the lane's neighbouring pixels first: with range noise
 * they shared a word only 1.4 to 1, and the bookkeeping for it cost more instructions than the atomics it saved.  A pixel
 * outside the window goes straight to memory (the bounding box of those is kept per wave, wavemiss_*), so the result never
 * depends on where the window is. */
__device__ __forceinline__ void wavewin_emit(unsigned long long *ww, unsigned int *wm, WaveWindow &w, unsigned long long *__restrict__ images,
                                             unsigned int imgWords, int W64, int winShift, ImageBox *boxes, const unsigned int (&key)[4], int lane)
{
  wavewin_prepare(ww, w, images, imgWords, W64, winShift, boxes, min(min(key[0], key[1]), min(key[2], key[3])), lane);
  const unsigned int base = window_base(w);
  unsigned int *ww32 = reinterpret_cast<unsigned int *>(ww);
#pragma unroll
  for(int j = 0; j < 4; j++)
  {
    const unsigned int k = key[j], d = k - base;
    const unsigned int bit = 1u << (k & 31u);
    if(window_hit(d, winShift))
    {
      if(SSD_CHK(3, ((d >> 13) << (winShift + 1)) + ((d & 0x1fffu) >> 5), 2 * kWinWords))
        atomicOr(&ww32[((d >> 13) << (winShift + 1)) + ((d & 0x1fffu) >> 5)], bit);
    }
    else if(k != kNoPixel)
    {
      const unsigned int slot = k >> 26, iy = (k >> 13) & 0x1fffu, ix = k & 0x1fffu, xw = ix >> 6;
      if(SSD_CHK(4, static_cast<unsigned long long>(slot) * imgWords + iy * static_cast<unsigned int>(W64) + xw, w.limitWords) && SSD_CHK(5, xw, W64))
        atomicOr(reinterpret_cast<unsigned int *>(images + (slot * imgWords + iy * static_cast<unsigned int>(W64) + xw)) + ((ix >> 5) & 1u), bit);
      int *b = reinterpret_cast<int *>(wm);
      atomicMin(&b[2], static_cast<int>(iy)); atomicMax(&b[3], static_cast<int>(iy));
      atomicMin(&b[4], static_cast<int>(xw)); atomicMax(&b[5], static_cast<int>(xw));
      atomicOr(&wm[6], 1u << slot);
    }
  }
}

/* Projection2D::worldToImage (pointcloud.cpp:79-83); false = outside the image (quirk Q5) */
__device__ __forceinline__ bool image_pixel(const PointParams &P, const PixelParams &X, double wx, double wy, int &ix, int &iy)
{
  ix = static_cast<int>((wx - P.xMin) * X.xToImage);
  iy = static_cast<int>((P.yMax - wy) * X.yToImage);
  /* two unsigned compares: a negative coordinate is a huge unsigned one */
  return (static_cast<unsigned int>(ix) < static_cast<unsigned int>(X.W)) & (static_cast<unsigned int>(iy) < static_cast<unsigned int>(X.H));
}

/* round(z * 2^40) without a double->int64 conversion (a long software sequence on this ISA): adding
 * 1.5 * 2^12 puts z (|z| < 2048) on the 2^-40 grid of [4096, 8192), rounded to nearest even by the add;
 * the mantissa difference to the constant is the integer.  Same value as llrint(z * 2^40). */
__device__ __forceinline__ long long z_to_fixed(double z)
{
  const double magic = 6144.0;
  return __double_as_longlong(z + magic) - __double_as_longlong(magic);
}
/* the same in two halves for running sums: n values of z_plus_magic_bits minus n * kMagicBits */
__device__ __forceinline__ long long z_plus_magic_bits(double z)
{
  return __double_as_longlong(z + 6144.0);
}
constexpr long long kMagicBits = 0x40B8000000000000ll;       /* bits of 6144.0 */

/* ---- single pass: K1's window spans FOUR planes ----
 * K1 rasters the points of the bins k_predict chose, one bit image ("plane") per height bin: which two adjacent bins make a
 * plateau is only known once the histogram is complete (k_peaks), and range noise spreads a tread over two or three bins
 * whose pixels interleave.  A window over one image would send every pixel of the minority bins to memory; this one
 * holds the same patch of 2^kSpecPlaneBits consecutive planes, 2^kSpecRowBits rows x 8 words each (2 x 16 x 8: 2 KiB per wave;
 * 4 planes x 16 rows, 2 x 32 and 1 x 32 measured the same or slower, 4 x 32 - three blocks per CU - much slower:
 * profiles/r04_single_pass_ab.txt).  Keys as pixel_key with the plane in the slot field, "inside" by one subtraction and one
 * AND as window_hit.  Since k_predict gives a tread whose fuller neighbour bin is beyond doubt ONE plane for both bins, most
 * treads live in a single plane anyway. */
#ifndef SSD_SPEC_PLANE_BITS
#define SSD_SPEC_PLANE_BITS 1
#endif
#ifndef SSD_SPEC_ROW_BITS
#define SSD_SPEC_ROW_BITS 4
#endif
constexpr int kSpecPlaneBits = SSD_SPEC_PLANE_BITS, kSpecRowBits = SSD_SPEC_ROW_BITS;
constexpr int kSpecWinPlanes = 1 << kSpecPlaneBits, kSpecWinRows = 1 << kSpecRowBits, kSpecWinCols = 8;
constexpr int kSpecWinWords = kSpecWinPlanes * kSpecWinRows * kSpecWinCols;
constexpr unsigned int kSpecInside = (static_cast<unsigned int>(kSpecWinPlanes - 1) << 26) | (static_cast<unsigned int>(kSpecWinRows - 1) << 13)
                                     | static_cast<unsigned int>(64 * kSpecWinCols - 1);
static_assert(kSpecWinCols == 8, "the index arithmetic below is written for eight word columns");
static_assert(kMaxPlanes <= 32 - kSpecWinPlanes, "a plane offset that borrows must fall outside the window's planes");

struct SpecWindow
{
  int plane0 = -1, row0 = 0, col0 = 0;   /* wave-uniform */
};
__device__ __forceinline__ unsigned int specwin_base(const SpecWindow &w)
{
  return w.plane0 < 0 ? kNoWindow : pixel_key(w.plane0, w.row0, w.col0 << 6);
}
__device__ __forceinline__ bool specwin_hit(unsigned int d)
{
  return (d & ~kSpecInside) == 0u;
}
/* OR over the wave, result in every lane's SGPR copy: rows by DPP, the four rows by readlane */
__device__ __forceinline__ unsigned int wave_or_u32(unsigned int v)
{
  v = row_or_u32(v);
  return static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(v), 0) | __builtin_amdgcn_readlane(static_cast<int>(v), 16)
                                   | __builtin_amdgcn_readlane(static_cast<int>(v), 32) | __builtin_amdgcn_readlane(static_cast<int>(v), 48));
}
/* Round 6: the window's rows are a RING - image row r of the window's range [row0, row0 + kSpecWinRows) lives in slot
 * r & (kSpecWinRows - 1) - so that the window can SLIDE down the image by half its height, writing out only the rows it leaves,
 * instead of standing still until more than half of a tile's pixels miss it and then being written out whole: measured on the
 * bench's frames, 98 % of the wave-tiles' pixels span fewer than 16 rows, yet 5 % of all pixels missed the standing window
 * "below" - in the tiles before each move - and went to memory one by one (tools/k1count.py, profiles/r06_k1_windows.txt).
 *
 * NROWS rows from image row rBegin (within the window's range) out - non-zero words only - and cleared.  One pass per plane
 * and 8 rows: lane = (row, word column).  The rows and columns that held bits come from the ballot of the non-zero words on the
 * scalar unit (no reductions over the wave), and extend the plane's box.  All 64 lanes. */
template<int NROWS>
__device__ __forceinline__ void specwin_flush_rows(unsigned long long *ww, const SpecWindow &w, const int rBegin, unsigned long long *__restrict__ planes,
                                                   unsigned int imgWords, int W64, ImageBox *boxes, int lane)
{
  static_assert(NROWS % 8 == 0 && NROWS <= kSpecWinRows, "whole passes of 8 rows");
  if(w.plane0 < 0)
    return;
#pragma unroll
  for(int pl = 0; pl < kSpecWinPlanes; pl++)
  {
    unsigned long long *img = planes + static_cast<size_t>(w.plane0 + pl) * imgWords;
#pragma unroll
    for(int k = 0; k < NROWS / 8; k++)
    {
      const int y = rBegin + 8 * k + (lane >> 3), x = w.col0 + (lane & 7);
      const int at = pl * (kSpecWinRows * kSpecWinCols) + ((y & (kSpecWinRows - 1)) << 3) + (lane & 7);
      const unsigned long long v = ww[at];
      const unsigned long long nz = __ballot(v != 0ull);         /* bit 8 r + c: row rBegin + 8 k + r, word column col0 + c */
      SSD_CNT(3, __popcll(nz));
      if(v)
      {
        if(SSD_CHK(6, static_cast<size_t>(w.plane0 + pl) * imgWords + static_cast<size_t>(y) * W64 + x, static_cast<size_t>(kMaxPlanes) * imgWords) && SSD_CHK(7, x, W64))
          atomicOr(img + static_cast<size_t>(y) * W64 + x, v);
        ww[at] = 0ull;
      }
      if(nz != 0ull)
      {
        unsigned long long r = nz | (nz >> 4);
        r |= r >> 2;
        r |= r >> 1;
        r &= 0x0101010101010101ull;                               /* bit 8 r: row r held bits */
        unsigned long long c = nz | (nz >> 32);
        c |= c >> 16;
        c |= c >> 8;
        c &= 0xffull;                                             /* bit c: column c held bits */
        const int rLo = (__ffsll(static_cast<long long>(r)) - 1) >> 3, rHi = (63 - __clzll(static_cast<long long>(r))) >> 3;
        const int cLo = __ffsll(static_cast<long long>(c)) - 1, cHi = 63 - __clzll(static_cast<long long>(c));
        if(lane == 0)
        {
          ImageBox &bx = boxes[w.plane0 + pl];
          atomicMin(&bx.yMin, rBegin + 8 * k + rLo); atomicMax(&bx.yMax, rBegin + 8 * k + rHi);
          atomicMin(&bx.xMin, w.col0 + cLo); atomicMax(&bx.xMax, w.col0 + cHi);
        }
      }
    }
  }
}
/* the whole window out (before it is re-anchored, and at the end of the block's loop) */
__device__ __forceinline__ void specwin_flush(unsigned long long *ww, const SpecWindow &w, unsigned long long *__restrict__ planes,
                                              unsigned int imgWords, int W64, ImageBox *boxes, int lane)
{
  specwin_flush_rows<kSpecWinRows>(ww, w, w.row0, planes, imgWords, W64, boxes, lane);
}
/* Before a tile's pixels go out, all 64 lanes; first / last: the lane's lowest and highest pixel_key of this tile (kNoPixel: none;
 * last as a signed number: kNoPixel is -1 and sorts below every key).
 *   - enough lanes (kSpecSlideLanes) whose last pixel lies in the half window BELOW the window - same planes, same columns -
 *     while no more than half of the lanes miss it altogether: the window slides down by half its height (the rows it leaves
 *     are written out);
 *   - more than half of the lanes that have pixels miss it: written out whole and re-anchored - one plane below the lowest
 *     plane of the tile's pixels (a tread's minority bin may lie on either side of the bin seen first), the lowest missing row,
 *     one word left of the lowest missing column. */
constexpr int kSpecSlideLanes = 6;
constexpr int kSpecSlideRows = kSpecWinRows / 2;
static_assert(kSpecSlideRows % 8 == 0, "a slide writes whole passes of 8 rows");
__device__ __forceinline__ void specwin_prepare(unsigned long long *ww, SpecWindow &w, unsigned long long *__restrict__ planes,
                                                unsigned int imgWords, int W64, ImageBox *boxes, unsigned int first, int last, int lane)
{
  const unsigned int base = specwin_base(w);
  const bool has = first != kNoPixel;
  const bool miss = has && !specwin_hit(first - base);
  /* "below": the difference to the origin has the row offset's next bit set and nothing else outside the window's fields, with
   * the offset below 1.5 windows: rows [kSpecWinRows, kSpecWinRows + kSpecSlideRows) */
  const unsigned int dl = static_cast<unsigned int>(last) - base;
  const bool below = last >= 0 && (dl & ~(kSpecInside & ~(static_cast<unsigned int>(kSpecSlideRows) << 13))) == (static_cast<unsigned int>(kSpecWinRows) << 13);
  const unsigned long long missing = __ballot(miss);
  const int nMissing = __popcll(missing), nHas = __popcll(__ballot(has));
  if(2 * nMissing <= nHas)
  {
    if(__popcll(__ballot(below)) >= kSpecSlideLanes)
    {
      SSD_CNT(2, 1);
      specwin_flush_rows<kSpecSlideRows>(ww, w, w.row0, planes, imgWords, W64, boxes, lane);
      w.row0 += kSpecSlideRows;
    }
    return;
  }
  const unsigned int loPlane = __builtin_amdgcn_readfirstlane(wave_min_u32(has ? first >> 26 : 31u));     /* of ALL the tile's pixels: the planes of a tread alternate */
  const unsigned int loRow = __builtin_amdgcn_readfirstlane(wave_min_u32(miss ? (first >> 13) & 0x1fffu : 0x1fffu));
  const unsigned int loCol = __builtin_amdgcn_readfirstlane(wave_min_u32(miss ? first & 0x1fffu : 0x1fffu));
  SSD_CNT(2, 1);
  specwin_flush(ww, w, planes, imgWords, W64, boxes, lane);
  w.plane0 = max(0, min(static_cast<int>(loPlane) - (kSpecWinPlanes > 2 ? 1 : 0), kMaxPlanes - kSpecWinPlanes));
  w.row0 = static_cast<int>(loRow);
  w.col0 = max(0, min(static_cast<int>(loCol >> 6) - 1, W64 - kSpecWinCols));
}
/* The pixels a lane sent straight to memory because they missed the window: their bounding box and planes, in the lane's
 * registers (K2 / K4 keep them per wave in LDS with five LDS atomics per miss, wavemiss_*; here two or three times as many
 * pixels miss - the points of a candidate bin that lie elsewhere in the image, on a wall behind the stairs - and the lane
 * has registers to spare).  specmiss_flush, end of the block's loop: reduced over the wave, into the block's boxes. */
struct SpecMiss
{
  int y0 = 0x7fffffff, y1 = -1, x0 = 0x7fffffff, x1 = -1;
  unsigned int planes = 0u;
};
__device__ __forceinline__ void specmiss_flush(const SpecMiss &m, ImageBox *boxes, int lane)
{
  const unsigned int planes = wave_or_u32(m.planes);
  if(planes == 0u)
    return;
  const int y0 = wave_min_i(m.y0), y1 = wave_max_i(m.y1), x0 = wave_min_i(m.x0), x1 = wave_max_i(m.x1);
  if(lane < 32 && ((planes >> lane) & 1u))
  {
    atomicMin(&boxes[lane].yMin, y0); atomicMax(&boxes[lane].yMax, y1);
    atomicMin(&boxes[lane].xMin, x0); atomicMax(&boxes[lane].xMax, x1);
  }
}
/* as wavewin_emit; the window's word of a pixel: (plane offset, row slot = row & (rows - 1), half word) */
__device__ __forceinline__ void specwin_emit(unsigned long long *ww, SpecMiss &miss, SpecWindow &w, unsigned long long *__restrict__ planes,
                                             unsigned int imgWords, int W64, ImageBox *boxes, const unsigned int (&key)[4], int lane)
{
  specwin_prepare(ww, w, planes, imgWords, W64, boxes, min(min(key[0], key[1]), min(key[2], key[3])),
                  max(max(static_cast<int>(key[0]), static_cast<int>(key[1])), max(static_cast<int>(key[2]), static_cast<int>(key[3]))), lane);
  const unsigned int base = specwin_base(w);
  unsigned int *ww32 = reinterpret_cast<unsigned int *>(ww);
#pragma unroll
  for(int j = 0; j < 4; j++)
  {
    const unsigned int k = key[j], d = k - base;
    const unsigned int bit = 1u << (k & 31u);
    SSD_CNT_LANES(4, k != kNoPixel);
    SSD_CNT_LANES(5, k != kNoPixel && !specwin_hit(d));
    if(specwin_hit(d))
    {
      const unsigned int at = ((d >> 26) << (kSpecRowBits + 4)) | (((k >> 13) & (kSpecWinRows - 1u)) << 4) | ((d & 0x1fffu) >> 5);
      if(SSD_CHK(8, at, 2 * kSpecWinWords))
        atomicOr(&ww32[at], bit);
    }
    else if(k != kNoPixel)
    {
      const unsigned int slot = k >> 26, iy = (k >> 13) & 0x1fffu, ix = k & 0x1fffu, xw = ix >> 6;
      if(SSD_CHK(9, static_cast<unsigned long long>(slot) * imgWords + iy * static_cast<unsigned int>(W64) + xw, static_cast<unsigned long long>(kMaxPlanes) * imgWords) && SSD_CHK(10, xw, W64))
        atomicOr(reinterpret_cast<unsigned int *>(planes + (slot * imgWords + iy * static_cast<unsigned int>(W64) + xw)) + ((ix >> 5) & 1u), bit);
      miss.y0 = min(miss.y0, static_cast<int>(iy)); miss.y1 = max(miss.y1, static_cast<int>(iy));
      miss.x0 = min(miss.x0, static_cast<int>(xw)); miss.x1 = max(miss.x1, static_cast<int>(xw));
      miss.planes |= 1u << slot;
    }
  }
}

} // namespace ssd

#endif /* SSD_K_WINDOWS_H_ */
