/*
 * ssd_treadgrid.h — the tread grid rule (include/ssd_hip.h), stated once for the device (k_tread_grid and
 * k_tread_grid_cams, ssd_kernels_treadgrid.hip) and the host (ssd_tread_grid_host, ssd_tread_grid_solve: ssd_host.cpp), and the kernels'
 * launcher.  Built on ssd_clearance.h, whose functions decide which points stand on which surface and stay as they are; this text adds
 * the tread points of a surface and the cell of a point in the surface's own frame.  Both sides are compiled without FMA contraction;
 * sqrt and / are correctly rounded on both (ssd_math.h relies on the same); everything counted or maximised is an integer: they agree
 * bit for bit.
 */
#ifndef SSD_TREADGRID_H_
#define SSD_TREADGRID_H_

#include "ssd_clearance.h"
#include "ssd_moments.h"

namespace ssd
{

constexpr int kTgCells = SSD_TG_ROWS * SSD_TG_COLS;

/* the ranges a rule must lie in: the clearance rule's, and cell in [0.005, 1]; a NaN fails */
inline bool tread_grid_rule_ok(const ssd_tread_grid_rule &r)
{
  return clearance_rule_ok(r.clearance) && r.cell >= 0.005 && r.cell <= 1.0;
}

/* A surface's own frame: the front edge FL -> FR (side 0 of the ring), its length, the ring's orientation, and the least u of the four
 * corners.  live: the grid takes points (o != 0 and the front edge has a length; a NaN: not live). */
struct TreadGridAxes
{
  double x0, y0, dx, dy, o, len, u0;
  bool live;
};

__host__ __device__ inline void tread_grid_axes(const ClearanceSurface &S, TreadGridAxes &G)
{
  const ClearanceSide &e = S.side[0];
  G.x0 = e.x;
  G.y0 = e.y;
  G.dx = e.dx;
  G.dy = e.dy;
  G.o = S.o;
  G.len = sqrt(e.dx * e.dx + e.dy * e.dy);
  G.live = S.o != 0.0 && G.len > 0.0;
  double u0 = 0.0;                               /* FL; then FR, BR, BL in ring order */
#pragma unroll
  for(int i = 1; i < 4; i++)
  {
    const double ax = S.side[i].x - e.x, ay = S.side[i].y - e.y;
    const double ui = (e.dx * ax + e.dy * ay) / G.len;
    if(ui < u0)
      u0 = ui;
  }
  G.u0 = u0;
}

/* The cell of (ex, ey) on the surface: along the front edge from the leftmost corner (column), behind the edge (row).  false: outside
 * the grid, or the grid is not live - compared as doubles before any conversion, so a NaN is out. */
__host__ __device__ inline bool tread_grid_cell(const TreadGridAxes &G, double cell, double ex, double ey, int &row, int &col)
{
  if(!G.live)
    return false;
  const double ax = ex - G.x0, ay = ey - G.y0;
  const double u = (G.dx * ax + G.dy * ay) / G.len;
  const double v = (G.o * (G.dx * ay - G.dy * ax)) / G.len;
  const double c = floor((u - G.u0) / cell), r = floor(v / cell);
  if(!(c >= 0.0 && c < static_cast<double>(SSD_TG_COLS) && r >= 0.0 && r < static_cast<double>(SSD_TG_ROWS)))
    return false;
  row = static_cast<int>(r);
  col = static_cast<int>(c);
  return true;
}

/* The surface a point that is no occupant is a tread point of: the lowest k among `candidates` (bit k; a superset of the surfaces whose
 * slab holds ez gives the same answer as all of them) whose slab holds ez and whose shrunk quadrilateral holds (ex, ey); -1: none */
__host__ __device__ inline int tread_grid_lowest(const ClearanceSurface *S, unsigned int candidates, double ex, double ey, double ez, double lo)
{
  while(candidates != 0u)
  {
    const int k = __builtin_ctz(candidates);
    candidates &= candidates - 1u;
    if(!(__builtin_fabs(ez - S[k].height) > lo) && clearance_inside(S[k], ex, ey))
      return k;
  }
  return -1;
}

/* an occupant's height above its surface in units of 2^-16 m (positive: it lies more than lo above; below 2^19: hi <= 8) */
__host__ __device__ inline int tread_grid_top(double ez, double height)
{
  return static_cast<int>(moment_round(ez - height));
}

/* grid coordinates (in cells: a cell's centre is row + .5, col + .5) mapped back to the external world:
 * FL + ((u0 + col cell) / L) e + ((row cell) / L) o (-dy, dx) */
inline void tread_grid_world(const TreadGridAxes &G, double cell, double row, double col, double &x, double &y)
{
  const double a = (G.u0 + col * cell) / G.len, b = (row * cell) / G.len;
  x = (G.x0 + a * G.dx) + b * (G.o * -G.dy);
  y = (G.y0 + a * G.dy) + b * (G.o * G.dx);
}

/* k_tread_grid behind a whole run of the chain on the same workspace (k_tread_grid_cams behind a whole cameras batch): launch_clearance's
 * arguments with the grid's rule and record.  out: frame i's record at out + i, zeroed by the caller on the stream in front of the
 * launch, which only adds to it and raises its maxima */
struct Batch;                                 /* ssd_launch.h */
void launch_tread_grid(const Batch &B, int chunkPoints, const ssd_frame_result *results, const ssd_tread_grid_rule &rule, ssd_frame_tread_grid *out);

/* k_stair_map / k_stair_map_cams (ssd_kernels_stairmap.hip) in the same place: the same walk against the caller's
 * staircases.  maps: nmaps records, device; mapOf: the batch's index frame -> map, device, an int per frame (anything not below nmaps: the
 * frame adds nothing); out: nmaps records, which the launch only adds to and raises, and whose headers it writes */
void launch_stair_map(const Batch &B, int chunkPoints, const ssd_stair_map *maps, const int *mapOf, int nmaps, const ssd_tread_grid_rule &rule,
                      ssd_frame_tread_grid *out);

/* The fold's step over two records (ssd_tread_grid_add): false, and acc as it was, if a count would pass 2^32 - 1 */
inline bool tread_grid_add(const ssd_frame_tread_grid &in, ssd_frame_tread_grid &acc)
{
  for(int k = 0; k < SSD_MAX_STEPS; k++)
  {
    const ssd_tread_grid &a = in.s[k], &b = acc.s[k];
    bool over = a.n_seen_out > 0xffffffffu - b.n_seen_out || a.n_occ_out > 0xffffffffu - b.n_occ_out;
    for(int i = 0; i < kTgCells && !over; i++)
      over = (&a.seen[0][0])[i] > 0xffffffffu - (&b.seen[0][0])[i] || (&a.occ[0][0])[i] > 0xffffffffu - (&b.occ[0][0])[i];
    if(over)
      return false;
  }
  acc.n_surfaces = in.n_surfaces;
  acc.ground = in.ground;
  for(int k = 0; k < SSD_MAX_STEPS; k++)
  {
    const ssd_tread_grid &a = in.s[k];
    ssd_tread_grid &b = acc.s[k];
    b.n_seen_out += a.n_seen_out;
    b.n_occ_out += a.n_occ_out;
    if(a.top_out > b.top_out)
      b.top_out = a.top_out;
    for(int i = 0; i < kTgCells; i++)
    {
      (&b.seen[0][0])[i] += (&a.seen[0][0])[i];
      (&b.occ[0][0])[i] += (&a.occ[0][0])[i];
      if((&a.top[0][0])[i] > (&b.top[0][0])[i])
        (&b.top[0][0])[i] = (&a.top[0][0])[i];
    }
  }
  return true;
}

} // namespace ssd

#endif /* SSD_TREADGRID_H_ */
