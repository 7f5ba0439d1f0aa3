/* ssd_k_point.h - shared per-point arithmetic, the streaming kernels' block shape and point loads (world_point_flat, load_points*, first_use).
 * Device code of the per-frame path, cut by stage: DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_POINT_H_
#define SSD_K_POINT_H_
#include "ssd_k_entry.h"

namespace ssd
{

/* ========================================================================= */
/* shared per-point arithmetic                                                */

struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };

/* CameraToWorld (transformation.h:59-64, 79-87): a*x + b, float promoted to double, row sums left to right, then the
 * translation; followed by the non-zero test (pointcloud.cpp:143-146) and the six strict range compares of
 * getPointsInRange (pointcloud.cpp:150-165).  Flat code: all three rows, then the seven tests combined without short
 * circuit.  Early exits only pay when all 64 lanes of a wave take them, which a camera image next to never offers; as nested
 * branches they cost the default values of everything the point contributes, re-materialised at every level (9 moves per
 * point in K1's ISA).  (The throughput of K1 / K2 on float3 input did not move with it — they sit on the memory roof
 * of the GPU's current clock state — but the instruction count did: what 16-bit depth input, VALU-bound, runs on.) */
__device__ __forceinline__ bool world_point_flat(const PointParams &P, const F3 &v, double &wx, double &wy, double &wz)
{
  const double x = v.x, y = v.y, z = v.z;
  wx = (P.a[0] * x + P.a[1] * y) + P.a[2] * z;
  wy = (P.a[3] * x + P.a[4] * y) + P.a[5] * z;
  wz = (P.a[6] * x + P.a[7] * y) + P.a[8] * z;
  wx = wx + P.b[0];
  wy = wy + P.b[1];
  wz = wz + P.b[2];
  return (v.z > 0.0f) & (wx > P.xMin) & (wx < P.xMax) & (wy > P.yMin) & (wy < P.yMax) & (wz > P.zMin) & (wz < P.zMax);
}

/* The same decisions taken height first, for the passes that drop most points on their height bin: the z row
 * and the z tests, then (only for points whose bin matters) the x and y rows and their tests.  The
 * conjunction of tests and every operation are those of world_point_flat. */
__device__ __forceinline__ bool world_z(const PointParams &P, const F3 &v, double &wz)
{
  if(!(v.z > 0.0f))
    return false;
  wz = (P.a[6] * static_cast<double>(v.x) + P.a[7] * static_cast<double>(v.y)) + P.a[8] * static_cast<double>(v.z);
  wz = wz + P.b[2];
  return wz > P.zMin && wz < P.zMax;
}
/* world_z without the early exit, for flat code (wz is meaningless when false is returned) */
__device__ __forceinline__ bool world_z_flat(const PointParams &P, const F3 &v, double &wz)
{
  wz = (P.a[6] * static_cast<double>(v.x) + P.a[7] * static_cast<double>(v.y)) + P.a[8] * static_cast<double>(v.z);
  wz = wz + P.b[2];
  return v.z > 0.0f && wz > P.zMin && wz < P.zMax;
}
__device__ __forceinline__ bool world_xy(const PointParams &P, const F3 &v, double &wx, double &wy)
{
  const double x = v.x, y = v.y, z = v.z;
  wx = (P.a[0] * x + P.a[1] * y) + P.a[2] * z;
  wy = (P.a[3] * x + P.a[4] * y) + P.a[5] * z;
  wx = wx + P.b[0];
  wy = wy + P.b[1];
  return wx > P.xMin && wx < P.xMax && wy > P.yMin && wy < P.yMax;
}

/* calcHeights (pointcloud.cpp:175): truncating conversion, value is in [0, nBins) */
__device__ __forceinline__ int height_bin(const PointParams &P, double wz)
{
  return static_cast<int>((wz - P.zMin) * P.recip);
}

/* ========================================================================= */
/* the streaming kernels' block shape, point sources and loads                */

/* k_raster is built for 6 waves per SIMD: 75 VGPRs, no scratch spills (round 2: 7 waves, 72 VGPRs, 3 spills).  Measured in
 * round 3, same box, alternating runs, XGA batch: 8 / 7 / 6 / 5 / 4 waves 0.848 / 0.823 / 0.800 / 0.801 / 0.799 ms; FHD stress:
 * 7 / 6 / 5 within 1 % — the walk is bound by instruction issue, not by latency: residency beyond four waves buys nothing */
/* k_inquad (round 6: every decision in single precision first, the doubles out of line): 5 waves per SIMD - 92 vector registers,
 * no spill of either kind in the XGA instantiation; 6 waves spill 3 vector registers and run a third slower (0.64 -> 0.84 ms), 4 waves
 * the same as 5 (profiles/r06_k4_edges.txt).  Until round 6: 8 waves at 48 scalar spills in the loop. */
#ifndef SSD_K4_WAVES
#define SSD_K4_WAVES 5
#endif
#ifndef SSD_K2_WAVES
#define SSD_K2_WAVES 6
#endif
constexpr int kThreads = 256;
constexpr int kPts = 4;                 /* points per thread per iteration: four CONSECUTIVE points (48 B) */
constexpr int kTile = kThreads * kPts;  /* 1024 points per block iteration */
#ifndef SSD_HIST_COPIES
#define SSD_HIST_COPIES 32
#endif
constexpr int kHistCopies = SSD_HIST_COPIES;         /* LDS histogram privatised by lane & 31: bank = copy, no conflicts */

/* Point sources of the streaming kernels */
constexpr int kSrcF3 = 0;          /* float xyz, 12-byte loads (unaligned frames, or a point count not divisible by 4) */
constexpr int kSrcF3Aligned = 1;   /* float xyz, 16-byte loads */
constexpr int kSrcDepth16 = 2;     /* 16-bit depth image + intrinsics: deprojected on the fly */

/* Four consecutive points of one lane.  kSrcF3Aligned: three 16-byte loads (lanes 48 B apart; the three
 * instructions of a wave together cover 3 KiB contiguously — measured 6.2-6.3 TB/s on MI355X, the same as
 * a plain float4 stream, tools/loadbench.hip).  kSrcF3 (frame base/stride not 16-byte aligned, or the
 * tail of a frame whose point count is not a multiple of 4): 12-byte loads.  kSrcDepth16: four 16-bit depth
 * values (one 8-byte load) turned into points exactly as librealsense's pointcloud block does in float:
 * d = raw * depth_units; point = (d * xmap[u], d * ymap[v], d); raw = 0 gives the invalid point (0,0,0). */
/* kSrcDepth16: the lane's four depth pixels and the maps' values for them -> four points, in float as librealsense does
 * (d = raw * depth_units; point = (d * xmap[u], d * ymap[v], d); raw = 0 gives the invalid point (0,0,0)) */
__device__ __forceinline__ void deproject4(const uint2 raw, const float4 xm, const float ym, const float units, F3 (&v)[kPts])
{
  const float d0 = static_cast<float>(raw.x & 0xffffu) * units, d1 = static_cast<float>(raw.x >> 16) * units;
  const float d2 = static_cast<float>(raw.y & 0xffffu) * units, d3 = static_cast<float>(raw.y >> 16) * units;
  v[0] = F3{ d0 * xm.x, d0 * ym, d0 };
  v[1] = F3{ d1 * xm.y, d1 * ym, d1 };
  v[2] = F3{ d2 * xm.z, d2 * ym, d2 };
  v[3] = F3{ d3 * xm.w, d3 * ym, d3 };
}
/* image row of point index idx (DepthSrc::rowMagic) */
__device__ __forceinline__ int depth_row(const DepthSrc &D, int idx)
{
  return D.rowMagic ? static_cast<int>(__umulhi(static_cast<unsigned int>(idx), D.rowMagic) >> 7) : idx / D.W;
}

template<int SRC>
__device__ __forceinline__ void load_points(const float *__restrict__ base, int idx0, int end, F3 (&v)[kPts], const DepthSrc &D)
{
  if(SRC == kSrcDepth16)
  {
    /* width % 4 == 0 and idx0 % 4 == 0 (ssd_enqueue_depth checks the first, every caller provides the second): the four
     * pixels share the image row, lie wholly inside or wholly outside the frame, and their x-map entries are one aligned
     * 16-byte load (round 3: four dependent 4-byte loads and a division per call) */
    const unsigned short *depth = reinterpret_cast<const unsigned short *>(base);
    const bool inside = idx0 + kPts <= end;
    const uint2 raw = inside ? *reinterpret_cast<const uint2 *>(depth + idx0) : make_uint2(0u, 0u);
    const int row = depth_row(D, idx0), col = idx0 - row * D.W;
    const float ym = D.ymap[min(row, D.H - 1)];               /* lanes past the end of the frame (raw = 0) stay inside the map */
    const float4 xm = *reinterpret_cast<const float4 *>(D.xmap + col);
    deproject4(raw, xm, ym, D.depthUnits, v);
    return;
  }
  if(SRC == kSrcF3Aligned && idx0 + kPts <= end)
  {
    const float4 *q = reinterpret_cast<const float4 *>(base + 3 * static_cast<size_t>(idx0));
    const float4 a = q[0], b = q[1], c = q[2];
    v[0] = F3{ a.x, a.y, a.z };
    v[1] = F3{ a.w, b.x, b.y };
    v[2] = F3{ b.z, b.w, c.x };
    v[3] = F3{ c.y, c.z, c.w };
    return;
  }
#pragma unroll
  for(int j = 0; j < kPts; j++)
  {
    const int idx = idx0 + j;
    v[j] = F3{ 0.0f, 0.0f, 0.0f };
    if(idx < end)
      v[j] = *reinterpret_cast<const F3 *>(base + 3 * static_cast<size_t>(idx));
  }
}

/* The lane's four points of a tile that lies wholly inside the frame: no bounds, no branches, nothing between the loads and their
 * first use.  Round 5: load_points() has two paths (this one, and point by point at the frame's end); where they join the compiler
 * puts copies of the loaded registers INTO the fast path - an s_waitcnt vmcnt right behind the loads - and the "prefetch" of the
 * next tile waited for its data before the current tile was touched (found in the ISA of the single pass's K1, which a build fed
 * from the Infinity Cache had shown to be waiting for memory: 1.69 ms against 2.12 from HBM; tools/mkvariant.sh's SED_EXPR). */
template<int SRC>
__device__ __forceinline__ void load_points_full(const float *__restrict__ base, int idx0, F3 (&v)[kPts])
{
  if(SRC == kSrcDepth16)
    return;                                     /* vertex input only: the depth stream has a loop of its own */
  if(SRC == kSrcF3Aligned)
  {
    const float4 *q = reinterpret_cast<const float4 *>(base + 3 * static_cast<size_t>(idx0));
    /* (the frames read as a stream that is not to be kept in the caches, __builtin_nontemporal_load: 25 % slower,
     * profiles/r06_box_spread.txt; the code: commit ad9a851) */
    const float4 a = q[0], b = q[1], c = q[2];
    v[0] = F3{ a.x, a.y, a.z };
    v[1] = F3{ a.w, b.x, b.y };
    v[2] = F3{ b.z, b.w, c.x };
    v[3] = F3{ c.y, c.z, c.w };
    return;
  }
#pragma unroll
  for(int j = 0; j < kPts; j++)
    v[j] = *reinterpret_cast<const F3 *>(base + 3 * static_cast<size_t>(idx0 + j));
}

/* The same without knowing that the tile is whole: the loads go to addresses clamped into [0, end) - no bounds, no branches, and so
 * nothing that uses the data behind the loads - and zero_beyond(), called where the points are first used, blanks the points at or
 * beyond `end` (z = 0: "no measurement", dropped by every consumer first).  end >= 4; vertex input only.  kSrcF3Aligned: idx0 and end
 * are multiples of 4 (points_aligned()), so a lane's four points lie wholly inside or wholly beyond. */
template<int SRC>
__device__ __forceinline__ void load_points_clamped(const float *__restrict__ base, int idx0, int end, F3 (&v)[kPts])
{
  if(SRC == kSrcDepth16)
    return;
  if(SRC == kSrcF3Aligned)
  {
    load_points_full<SRC>(base, min(idx0, end - kPts), v);
    return;
  }
#pragma unroll
  for(int j = 0; j < kPts; j++)
    v[j] = *reinterpret_cast<const F3 *>(base + 3 * static_cast<size_t>(min(idx0 + j, end - 1)));
}
__device__ __forceinline__ void zero_beyond(F3 (&v)[kPts], int idx0, int end)
{
#pragma unroll
  for(int j = 0; j < kPts; j++)
    if(idx0 + j >= end)
      v[j] = F3{ 0.0f, 0.0f, 0.0f };
}

/* "The loaded registers are first looked at HERE": an empty asm that takes and returns the twelve registers of a lane's four points.
 * Placed behind the tile the loads were issued in front of: without it the compiler builds the (x, y) register pairs of the next
 * tile's points (v_pk_fma_f32 and the fp64 conversions want them aligned) right behind the loads - and waits for the data there. */
__device__ __forceinline__ void first_use(F3 (&v)[kPts])
{
  asm volatile("" : "+v"(v[0].x), "+v"(v[0].y), "+v"(v[0].z), "+v"(v[1].x), "+v"(v[1].y), "+v"(v[1].z),
                    "+v"(v[2].x), "+v"(v[2].y), "+v"(v[2].z), "+v"(v[3].x), "+v"(v[3].y), "+v"(v[3].z));
}

/* A block of a streaming kernel (K1, K2, K4) owns a contiguous chunk of a frame.  K1 walks all of it in tiles of 1024 points: the
 * loads of the next tile are issued before the current tile is processed (register double buffer: hist_block's "one copy of the
 * body"), so that HBM requests stay in flight while the SIMDs do the fp64 work.  K2 and K4 walk the chunk's list of wanted cells
 * instead (ssd_k_cells.h). */

} // namespace ssd

#endif /* SSD_K_POINT_H_ */
