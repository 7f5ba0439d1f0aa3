/*
 * ssd_host.cpp — the handle-free half of the C ABI of libssd_hip.so (include/ssd_hip.h): the configuration and the calibrations, the
 * host statements of the passes (the rule headers' text over one frame on the CPU), the solvers and folds over their records, the
 * label split and the serializer - and the refusals they share with the entry points that run on a handle (ssd_host.h).  Plain C++:
 * compiled without a device pass, no HIP call, no ssd_handle, no stream, no launcher; a function that needs one of those belongs in
 * ssd_capi.hip.  -ffp-contract=off as everywhere: the reference arithmetic has no FMA, and the statements' records are compared with
 * the kernels' byte for byte.
 */
#include "ssd_host.h"
#include "ssd_pose.h"
#include "ssd_fuse.h"
#include "ssd_edges.h"
#include "ssd_fill.h"
#include "ssd_warp.h"
#include "ssd_refit.h"
#include "ssd_clearance.h"
#include "ssd_treadgrid.h"
#include "ssd_solve.h"
#include "ssd_fold.h"

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

using namespace ssd;

static thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
  g_err = msg;
  return code;
}

const char *ssd_last_error(void)
{
  return g_err.c_str();
}

int ssd_default_config(ssd_config *cfg, int width, int height)
{
  if(!cfg || width <= 0 || height <= 0)
    return fail(SSD_E_ARG, "ssd_default_config: bad argument");
  /* configuration.h:27-52 */
  cfg->width = width;
  cfg->height = height;
  cfg->x_min = -0.6; cfg->x_max = 0.6;
  cfg->y_min = 0.1; cfg->y_max = 1.3;
  cfg->z_min = -0.1; cfg->z_max = 1.1;
  cfg->height_interval = 0.01;
  cfg->min_height_above_ground = 0.05;
  cfg->min_step_depth = 0.1;
  cfg->max_frames_per_batch = 64;
  cfg->max_step_plateaus = SSD_MAX_STEP_IMAGES;
  cfg->batches_in_flight = 0;                 /* automatic: see ssd_config */
  return SSD_OK;
}

int ssd_calibration_identity(ssd_calibration *out)
{
  if(!out)
    return fail(SSD_E_ARG, "ssd_calibration_identity: null");
  std::memset(out, 0, sizeof(*out));
  out->a[0] = out->a[4] = out->a[8] = 1.0;
  out->r2[0] = out->r2[3] = 1.0;
  return SSD_OK;
}

/* camera_to_world_from_plane - CameraToWorld from the floor's plane in camera coordinates, shared by ssd_calibration_from_points,
 * ssd_calibration_from_plane and the ground fit - is ssd_solve.h's: the device asks it too (k_camera_ground_gates) */

int ssd_calibration_from_plane(const double n0[3], double dist, const ssd_calibration *prior, ssd_calibration *out)
{
  if(!n0 || !prior || !out)
    return fail(SSD_E_ARG, "ssd_calibration_from_plane: null");
  ssd_calibration r = *prior;                   /* r2, t2, world_z carried over */
  if(!camera_to_world_from_plane(n0[0], n0[1], n0[2], dist, r.a, r.b))
    return fail(SSD_E_ARG, "ssd_calibration_from_plane: degenerate plane (reference assert, transformation.cpp:153)");
  *out = r;
  return SSD_OK;
}

/* GeometricTransformation(worldPoints, cameraPoints), transformation.cpp:196-215.
 * Vector algebra as Boost.QVM evaluates it: products summed left to right,
 * normalized(v) = v * (1 / sqrt(dot(v, v))). */
int ssd_calibration_from_points(const double w[9], const double c[9], ssd_calibration *out)
{
  if(!w || !c || !out)
    return fail(SSD_E_ARG, "ssd_calibration_from_points: null");
  struct V3 { double x, y, z; };
  auto sub = [](V3 a, V3 b) { return V3{ a.x - b.x, a.y - b.y, a.z - b.z }; };
  auto cross = [](V3 a, V3 b) { return V3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; };
  auto dot = [](V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; };
  auto norm = [](V3 a)
  {
    const double m2 = a.x * a.x + a.y * a.y + a.z * a.z;
    const double rm = 1.0 / std::sqrt(m2);
    return V3{ a.x * rm, a.y * rm, a.z * rm };
  };
  const V3 c0{ c[0], c[1], c[2] }, c1{ c[3], c[4], c[5] }, c2{ c[6], c[7], c[8] };

  /* Transformation_<3>(triangleInPlane), transformation.cpp:108-157 */
  const V3 n0 = norm(cross(sub(c1, c0), sub(c2, c0)));
  const double dist = dot(c0, n0);
  if(!camera_to_world_from_plane(n0.x, n0.y, n0.z, dist, out->a, out->b))
    return fail(SSD_E_ARG, "ssd_calibration_from_points: degenerate triangle (reference assert, transformation.cpp:153)");

  /* Transformation_<2>({w0, w1}, {cameraToWorld(c0), cameraToWorld(c1)}), transformation.cpp:65-106 */
  auto c2w = [&](V3 p)
  {
    V3 r;
    r.x = out->a[0] * p.x + out->a[1] * p.y + out->a[2] * p.z;
    r.y = out->a[3] * p.x + out->a[4] * p.y + out->a[5] * p.z;
    r.z = out->a[6] * p.x + out->a[7] * p.y + out->a[8] * p.z;
    r.x = r.x + out->b[0]; r.y = r.y + out->b[1]; r.z = r.z + out->b[2];
    return r;
  };
  const V3 m0 = c2w(c0), m1 = c2w(c1);
  auto norm2 = [](double x, double y, double &ox, double &oy)
  {
    const double m2 = x * x + y * y;
    const double rm = 1.0 / std::sqrt(m2);
    ox = x * rm; oy = y * rm;
  };
  double dx, dy, dxm, dym;
  norm2(w[3] - w[0], w[4] - w[1], dx, dy);
  norm2(m1.x - m0.x, m1.y - m0.y, dxm, dym);
  const double xBaseX = dx * dxm + dy * dym;
  const double xBaseY = dy * dxm - dx * dym;
  out->r2[0] = xBaseX; out->r2[1] = -xBaseY;
  out->r2[2] = xBaseY; out->r2[3] = xBaseX;
  out->t2[0] = w[0] - (out->r2[0] * m0.x + out->r2[1] * m0.y);
  out->t2[1] = w[1] - (out->r2[2] * m0.x + out->r2[3] * m0.y);
  out->world_z = w[2];
  if(!std::isfinite(xBaseX) || !std::isfinite(xBaseY))
    return fail(SSD_E_ARG, "ssd_calibration_from_points: coincident reference points");
  return SSD_OK;
}

/* ---- calibration files -------------------------------------------- */
namespace
{

/* What the reference's readValue (calibrationTriangle.cpp:48-68) accepts, stated on the token stream: the file from the
 * current position on is a sequence of whitespace-separated tokens; the first occurrence of the token `name` that is directly
 * followed by the token "=" selects the value, which is then extracted from the SAME stream with operator>> for T (so
 * "x1 = 0.5," yields 0.5 and leaves the comma, a string value takes the next token).  An occurrence of `name` not followed by
 * "=" consumes both tokens and the search goes on behind them.  False when the stream ends first or the extraction fails. */
template<typename T>
bool read_named_value(std::ifstream &file, const std::string &name, T &value)
{
  for(std::string token; file >> token; )
  {
    if(token != name)
      continue;
    std::string next;
    if(!(file >> next))
      break;
    if(next != "=")
      continue;
    return static_cast<bool>(file >> value);
  }
  return false;
}

/* CalibrationTriangle::load + isValid, calibrationTriangle.cpp:97-125, 148-172 */
bool load_triangle(const char *path, double w[9])
{
  std::ifstream file(path);
  std::string id;
  std::getline(file, id);
  if(id != "calibration triangle")
    return false;
  bool r = true;
  for(int n = 1; n <= 3; n++)
  {
    const std::string ns = std::to_string(n);
    r = r && read_named_value(file, "x" + ns, w[3 * (n - 1)]);
    r = r && read_named_value(file, "y" + ns, w[3 * (n - 1) + 1]);
    r = r && read_named_value(file, "z" + ns, w[3 * (n - 1) + 2]);
  }
  std::string side;
  r = r && read_named_value(file, "lowerQuadrant", side);
  if(!r)
    return false;
  const double minDistQu = 0.01 * 0.01;
  auto distQu = [&](int a, int b)
  {
    const double dx = w[3 * b] - w[3 * a], dy = w[3 * b + 1] - w[3 * a + 1], dz = w[3 * b + 2] - w[3 * a + 2];
    return dx * dx + dy * dy + dz * dz;
  };
  if(distQu(0, 1) < minDistQu || distQu(1, 2) < minDistQu || distQu(2, 0) < minDistQu)
    return false;
  return side == "left" || side == "right";
}

/* loadPoints + calcAverageRefPointSet, geometricCalibration.cpp:73-98, 127-141: ten rows of three float
 * points, summed in double in file order, divided by the count */
bool load_points(const char *path, double c[9])
{
  std::ifstream file(path);
  std::string id;
  std::getline(file, id);
  if(id != "calibration points")
    return false;
  const int numIterations = 10;
  double sum[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
  int n = 0;
  while(true)
  {
    float p[9];
    char ch;
    for(int k = 0; k < 3; k++)
    {
      file >> p[3 * k] >> ch >> p[3 * k + 1] >> ch >> p[3 * k + 2];
      if(k < 2)
        file >> ch;
    }
    if(!file)
      break;
    for(int k = 0; k < 9; k++)
      sum[k] += static_cast<double>(p[k]);
    if(++n == numIterations)
    {
      for(int k = 0; k < 9; k++)
        c[k] = sum[k] / static_cast<double>(static_cast<size_t>(n));
      return true;
    }
  }
  return false;
}

} // namespace

int ssd_calibration_load(const char *triangle_path, const char *points_path, ssd_calibration *out, int *loaded,
                         double *world_points, double *camera_points)
{
  if(!triangle_path || !points_path || !out)
    return fail(SSD_E_ARG, "ssd_calibration_load: null argument");
  double w[9], c[9];
  if(loaded)
    *loaded = 0;
  if(load_triangle(triangle_path, w) && load_points(points_path, c))
  {
    if(world_points) std::memcpy(world_points, w, sizeof(w));
    if(camera_points) std::memcpy(camera_points, c, sizeof(c));
    const int rc = ssd_calibration_from_points(w, c, out);
    if(rc == SSD_OK && loaded)
      *loaded = 1;
    return rc;
  }
  return ssd_calibration_identity(out);      /* geometricCalibration.cpp:199-202: log an error, return {} */
}

/* rs2::pointcloud's maps (librealsense2 src/proc/pointcloud.cpp, pre_compute_x_y_map), float arithmetic */
void depth_maps(const ssd_intrinsics &in, int W, int H, std::vector<float> &maps)
{
  maps.resize(static_cast<size_t>(W) + H);
  for(int u = 0; u < W; u++)
    maps[u] = (static_cast<float>(u) - in.ppx) / in.fx;
  for(int v = 0; v < H; v++)
    maps[W + v] = (static_cast<float>(v) - in.ppy) / in.fy;
}

int ssd_deproject_host(const ssd_intrinsics *intr, int width, int height, const uint16_t *depth, float *xyz)
{
  if(!intr || !depth || !xyz || width <= 0 || height <= 0)
    return fail(SSD_E_ARG, "ssd_deproject_host: bad argument");
  std::vector<float> maps;
  depth_maps(*intr, width, height, maps);
  for(int v = 0; v < height; v++)
    for(int u = 0; u < width; u++)
    {
      const size_t i = static_cast<size_t>(v) * width + u;
      const float d = static_cast<float>(depth[i]) * intr->depth_units;
      xyz[3 * i] = d * maps[u];
      xyz[3 * i + 1] = d * maps[width + v];
      xyz[3 * i + 2] = d;
    }
  return SSD_OK;
}

/* ---- ground fit: a calibration refined from the floor in the frames (include/ssd_hip.h) ----------- */

bool good_intrinsics(const ssd_intrinsics &in)
{
  return in.fx != 0.0f && in.fy != 0.0f && in.depth_units > 0.0f;
}

void ground_prior_fill(GroundPrior &g, const ssd_calibration &cal, const ssd_intrinsics *in)
{
  std::memset(&g, 0, sizeof(g));
  for(int i = 0; i < 9; i++) g.a[i] = cal.a[i];
  for(int i = 0; i < 3; i++) g.b[i] = cal.b[i];
  if(in)
  {
    g.ppx = in->ppx; g.ppy = in->ppy; g.fx = in->fx; g.fy = in->fy; g.depthUnits = in->depth_units;
  }
}

int ssd_ground_moments_host(const ssd_config *cfg, const ssd_camera *prior, int input, const void *frame, double tol, ssd_ground_moments *out)
{
  if(!cfg || !prior || !frame || !out || cfg->width <= 0 || cfg->height <= 0)
    return fail(SSD_E_ARG, "ssd_ground_moments_host: bad argument");
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, "ssd_ground_moments_host: input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  if(!(tol > 0.0) || !(tol <= 1.0))
    return fail(SSD_E_ARG, "ssd_ground_moments_host: tol must lie in (0, 1]");
  const bool depth = input == SSD_INPUT_DEPTH16;
  if(depth && (!prior->has_intrinsics || !good_intrinsics(prior->intr)))
    return fail(SSD_E_ARG, "ssd_ground_moments_host: depth input needs the prior's intrinsics");
  GroundPrior C;
  ground_prior_fill(C, prior->cal, depth ? &prior->intr : nullptr);
  const GroundRange R{ cfg->x_min, cfg->x_max, cfg->y_min, cfg->y_max, tol };
  const int W = cfg->width, H = cfg->height;
  long long acc[kGroundSums] = {};
  if(depth)
  {
    const uint16_t *d16 = static_cast<const uint16_t *>(frame);
    std::vector<float> xm(static_cast<size_t>(W));
    for(int u = 0; u < W; u++)
      xm[u] = ground_map_x(C, u);
    for(int v = 0; v < H; v++)
    {
      const float ym = ground_map_y(C, v);
      for(int u = 0; u < W; u++)
      {
        const float d = static_cast<float>(d16[static_cast<size_t>(v) * W + u]) * C.depthUnits;
        ground_point(C, R, d * xm[u], d * ym, d, acc);
      }
    }
  }
  else
  {
    const float *xyz = static_cast<const float *>(frame);
    for(size_t i = 0, n = static_cast<size_t>(W) * H; i < n; i++)
      ground_point(C, R, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], acc);
  }
  static_assert(sizeof(ssd_ground_moments) == sizeof(long long) * kGroundSums, "ssd_ground_moments is the kernel's record");
  std::memcpy(out, acc, sizeof(*out));
  return SSD_OK;
}

/* jacobi3, PlaneOfMoments and plane_of_moments - the core of the solve, shared by the ground fit, the surface fit, the riser fit and
 * the gates - are ssd_solve.h's: the device runs the same text (k_surface_gates) */

int ssd_ground_fit_solve(const ssd_ground_moments *m, const ssd_calibration *prior, int min_points, ssd_ground_fit *out)
{
  if(!m || !prior || !out)
    return fail(SSD_E_ARG, "ssd_ground_fit_solve: null");
  std::memset(out, 0, sizeof(*out));
  out->m = *m;
  out->cal = *prior;
  PlaneOfMoments pl;
  out->status = plane_of_moments(m, min_points, pl);
  if(out->status != SSD_GF_OK)
    return SSD_OK;
  out->status = SSD_GF_DEGENERATE;
  const double (&n0)[3] = pl.n0;
  const double dist = pl.dist;
  ssd_calibration cal = *prior;
  if(!camera_to_world_from_plane(n0[0], n0[1], n0[2], dist, cal.a, cal.b))
    return SSD_OK;
  out->status = SSD_GF_OK;
  out->cal = cal;
  for(int i = 0; i < 3; i++)
    out->normal[i] = n0[i];
  out->dist = dist;
  out->rms = std::sqrt(pl.lambda[0] > 0.0 ? pl.lambda[0] : 0.0);
  const double p[3] = { -prior->a[6], -prior->a[7], -prior->a[8] };
  const double cx = n0[1] * p[2] - n0[2] * p[1], cy = n0[2] * p[0] - n0[0] * p[2], cz = n0[0] * p[1] - n0[1] * p[0];
  out->tilt = std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), n0[0] * p[0] + n0[1] * p[1] + n0[2] * p[2]);
  out->height_delta = dist - prior->b[2];
  return SSD_OK;
}

/* ---- surface fit (include/ssd_hip.h): host side ---------------------------------------------------------- */

/* A frame's points as the host statements of the passes see them.  First the refusals the statements share: `pointers` = the caller's
 * own pointers are there, count = the frame's surfaces (`noun`: what the caller calls them), refused before the intrinsics where
 * countFirst (the two moment walks) and behind them otherwise (the clearance pass, the tread grid) */
static int host_frame_check(const std::string &who, bool pointers, const ssd_config *cfg, int input, const ssd_intrinsics *intr, const void *frame,
                            int count, const char *noun, bool countFirst)
{
  if(!pointers || !cfg || !frame || cfg->width <= 0 || cfg->height <= 0)
    return fail(SSD_E_ARG, who + ": bad argument");
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, who + ": input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  const bool countBad = count < 0 || count > SSD_MAX_STEPS;
  if(countFirst && countBad)
    return fail(SSD_E_ARG, who + ": " + noun + " must lie in 0 .. SSD_MAX_STEPS");
  if(input == SSD_INPUT_DEPTH16 && (!intr || !good_intrinsics(*intr)))
    return fail(SSD_E_ARG, who + ": depth input needs intrinsics");
  if(countBad)
    return fail(SSD_E_ARG, who + ": " + noun + " must lie in 0 .. SSD_MAX_STEPS");
  return SSD_OK;
}

/* ... then the frame as vertices: the caller's, or depth deprojected into `scratch` */
static int host_frame_xyz(const ssd_config *cfg, int input, const ssd_intrinsics *intr, const void *frame, std::vector<float> &scratch, const float *&xyz)
{
  xyz = static_cast<const float *>(frame);
  if(input != SSD_INPUT_DEPTH16)
    return SSD_OK;
  scratch.resize(3 * static_cast<size_t>(cfg->width) * cfg->height);
  xyz = scratch.data();
  return ssd_deproject_host(intr, cfg->width, cfg->height, static_cast<const uint16_t *>(frame), scratch.data());
}

/* ... and every point with z > 0 inside the configured range, in pixel order: f(pixel, x, y, z, wx, wy, wz), camera frame then world.
 * The transform is ((a0 x + a1 y) + a2 z) + b in double, as the kernels' (their records are compared byte for byte) */
template<class F>
static void host_frame_walk(const ssd_config *cfg, const ssd_calibration *cal, const float *xyz, F f)
{
  const size_t nPoints = static_cast<size_t>(cfg->width) * cfg->height;
  const double *a = cal->a, *b = cal->b;
  for(size_t i = 0; i < nPoints; i++)
  {
    const float fx = xyz[3 * i], fy = xyz[3 * i + 1], fz = xyz[3 * i + 2];
    if(!(fz > 0.0f))
      continue;
    const double x = fx, y = fy, z = fz;
    const double wx = ((a[0] * x + a[1] * y) + a[2] * z) + b[0];
    const double wy = ((a[3] * x + a[4] * y) + a[5] * z) + b[1];
    const double wz = ((a[6] * x + a[7] * y) + a[8] * z) + b[2];
    if(wx > cfg->x_min && wx < cfg->x_max && wy > cfg->y_min && wy < cfg->y_max && wz > cfg->z_min && wz < cfg->z_max)
      f(i, x, y, z, wx, wy, wz);
  }
}

/* What the clearance pass and the tread grid make of a frame's result before they walk it: the surfaces that can hold something (none
 * for a frame that threw), each with the rule's margin, and the calibration's external frame */
struct HostSurfaces
{
  int n;
  ClearanceSurface S[SSD_MAX_STEPS];
  ClearanceWorld X;
  HostSurfaces(const ssd_frame_result *result, const ssd_calibration *cal, double margin)
    : n((result->status & SSD_ST_THROW) ? 0 : result->n_steps),
      X{ { cal->r2[0], cal->r2[1], cal->r2[2], cal->r2[3] }, { cal->t2[0], cal->t2[1] }, cal->world_z }
  {
    for(int k = 0; k < n; k++)
      clearance_surface(result->steps[k], margin, S[k]);
  }
  /* their walk: f(pixel, x, y, z, ex, ey, ez), camera frame then external world */
  template<class F>
  void walk(const ssd_config *cfg, const ssd_calibration *cal, const float *xyz, F f) const
  {
    host_frame_walk(cfg, cal, xyz, [&](size_t i, double x, double y, double z, double wx, double wy, double wz)
    {
      double ex, ey;
      clearance_external(X, wx, wy, ex, ey);
      f(i, x, y, z, ex, ey, wz + X.worldZ);
    });
  }
};


/* The walk of ssd_surface_moments_host (gates == nullptr: every labelled point) and of ssd_surface_refit_moments_host (a labelled point
 * outside its surface's gate is skipped whole: ssd_refit.h) */
static int surface_moments_walk(const std::string &who, const ssd_config *cfg, int input, const ssd_intrinsics *intr, const void *frame,
                                const uint8_t *labels, const ssd_frame_gates *gates, int n_surfaces, int ground, ssd_frame_moments *out)
{
  int rc = host_frame_check(who, labels && out, cfg, input, intr, frame, n_surfaces, "n_surfaces", true);
  if(rc) return rc;
  const size_t nPoints = static_cast<size_t>(cfg->width) * cfg->height;
  for(size_t i = 0; i < nPoints; i++)
    if(labels[i] > n_surfaces)
      return fail(SSD_E_ARG, who + ": a label above n_surfaces");
  std::vector<float> deprojected;
  const float *xyz;
  rc = host_frame_xyz(cfg, input, intr, frame, deprojected, xyz);
  if(rc) return rc;
  static_assert(sizeof(ssd_surface_moments) == sizeof(long long) * (kGroundSums + 1), "ssd_surface_moments is the ten sums and n_far");
  long long acc[SSD_MAX_STEPS][kGroundSums + 1] = {};
  for(size_t i = 0; i < nPoints; i++)
  {
    if(labels[i] == SSD_LABEL_NONE)
      continue;
    if(gates && !refit_keeps(*gates, labels[i] - 1, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]))
      continue;
    long long (&a)[kGroundSums + 1] = acc[labels[i] - 1];
    const double rx = moment_round(xyz[3 * i]), ry = moment_round(xyz[3 * i + 1]), rz = moment_round(xyz[3 * i + 2]);
    if(moment_near(rx) && moment_near(ry) && moment_near(rz))
      moment_add(rx, ry, rz, a);
    else
      a[kGroundSums] += 1;
  }
  std::memset(out, 0, sizeof(*out));
  out->n_surfaces = n_surfaces;
  out->ground = ground ? 1 : 0;
  std::memcpy(out->s, acc, sizeof(acc));
  return SSD_OK;
}

/* a label mask with riser labels (ssd_set_riser_labels) into the two forms the host walks above accept; no GPU, no handle */
int ssd_labels_split(const uint8_t *labels, size_t n, uint8_t *surfaces, uint8_t *risers)
{
  if(!labels && n > 0)
    return fail(SSD_E_ARG, "ssd_labels_split: null labels");
  /* decided before anything is written: an output may be the input */
  for(size_t k = 0; k < n; k++)
    if(labels[k] > SSD_MAX_STEPS && (labels[k] < SSD_LABEL_RISER_BASE || labels[k] >= SSD_LABEL_RISER_BASE + SSD_MAX_RISERS))
      return fail(SSD_E_ARG, "ssd_labels_split: a label that is neither a surface's nor a riser's");
  for(size_t k = 0; k < n; k++)
  {
    const uint8_t l = labels[k];                 /* read once: either store below may overwrite it */
    const bool surface = l <= SSD_MAX_STEPS;
    if(surfaces)
      surfaces[k] = surface ? l : static_cast<uint8_t>(0);
    if(risers)
      risers[k] = surface ? static_cast<uint8_t>(0) : static_cast<uint8_t>(l - SSD_LABEL_RISER_BASE + 1);
  }
  return SSD_OK;
}

int ssd_surface_moments_host(const ssd_config *cfg, int input, const ssd_intrinsics *intr, const void *frame, const uint8_t *labels,
                             int n_surfaces, int ground, ssd_frame_moments *out)
{
  return surface_moments_walk("ssd_surface_moments_host", cfg, input, intr, frame, labels, nullptr, n_surfaces, ground, out);
}

int ssd_surface_fit_solve(const ssd_frame_moments *moments, const ssd_calibration *cal, int min_points, ssd_frame_surfaces *out)
{
  if(!moments || !cal || !out)
    return fail(SSD_E_ARG, "ssd_surface_fit_solve: null");
  if(moments->n_surfaces < 0 || moments->n_surfaces > SSD_MAX_STEPS)
    return fail(SSD_E_ARG, "ssd_surface_fit_solve: n_surfaces must lie in 0 .. SSD_MAX_STEPS");
  std::memset(out, 0, sizeof(*out));
  out->n_surfaces = moments->n_surfaces;
  out->ground = moments->ground;
  for(int k = 0; k < moments->n_surfaces; k++)
  {
    const ssd_surface_moments &sm = moments->s[k];
    ssd_surface_fit &f = out->s[k];
    f.n = sm.m.n;
    f.n_far = sm.n_far;
    PlaneOfMoments pl;
    f.status = plane_of_moments(&sm.m, min_points, pl);
    if(f.status != SSD_GF_OK)
      continue;
    /* the plane's normal towards the camera, in camera-dependent world coordinates (the rotation alone), then ToExternalWorld's
     * rotation of x and y; the centroid as a point: CameraToWorld, then ToExternalWorld (transformation.cpp:209-211) */
    double up[3], w[3];
    for(int i = 0; i < 3; i++)
    {
      up[i] = -((cal->a[3 * i] * pl.n0[0] + cal->a[3 * i + 1] * pl.n0[1]) + cal->a[3 * i + 2] * pl.n0[2]);
      w[i] = ((cal->a[3 * i] * pl.centroid[0] + cal->a[3 * i + 1] * pl.centroid[1]) + cal->a[3 * i + 2] * pl.centroid[2]) + cal->b[i];
    }
    f.normal[0] = cal->r2[0] * up[0] + cal->r2[1] * up[1];
    f.normal[1] = cal->r2[2] * up[0] + cal->r2[3] * up[1];
    f.normal[2] = up[2];
    f.centroid[0] = (cal->r2[0] * w[0] + cal->r2[1] * w[1]) + cal->t2[0];
    f.centroid[1] = (cal->r2[2] * w[0] + cal->r2[3] * w[1]) + cal->t2[1];
    f.centroid[2] = w[2] + cal->world_z;
    f.tilt = std::atan2(std::sqrt(f.normal[0] * f.normal[0] + f.normal[1] * f.normal[1]), f.normal[2]);
    f.rms = std::sqrt(pl.lambda[0] > 0.0 ? pl.lambda[0] : 0.0);
    f.extent[0] = std::sqrt(pl.lambda[2]);
    f.extent[1] = std::sqrt(pl.lambda[1]);
  }
  return SSD_OK;
}

int check_gate_rule(const char *who, double k_sigma, double gate_min)
{
  if(!(k_sigma > 0.0) || !(k_sigma <= 16.0))
    return fail(SSD_E_ARG, std::string(who) + ": k_sigma must lie in (0, 16]");
  if(!(gate_min >= 0.0) || !(gate_min <= 1.0))
    return fail(SSD_E_ARG, std::string(who) + ": gate_min must lie in [0, 1]");
  return SSD_OK;
}

int ssd_surface_gates_from_moments(const ssd_frame_moments *m, int min_points, double k_sigma, double gate_min, ssd_frame_gates *out)
{
  if(!m || !out)
    return fail(SSD_E_ARG, "ssd_surface_gates_from_moments: null");
  if(m->n_surfaces < 0 || m->n_surfaces > SSD_MAX_STEPS)
    return fail(SSD_E_ARG, "ssd_surface_gates_from_moments: n_surfaces must lie in 0 .. SSD_MAX_STEPS");
  const int rc = check_gate_rule("ssd_surface_gates_from_moments", k_sigma, gate_min);
  if(rc) return rc;
  std::memset(out, 0, sizeof(*out));
  out->n_surfaces = m->n_surfaces;
  for(int k = 0; k < m->n_surfaces; k++)
    out->g[k] = gate_of_moments(&m->s[k].m, min_points, k_sigma, gate_min);      /* ssd_solve.h; all zero unless the fit is OK */
  return SSD_OK;
}

int ssd_surface_refit_moments_host(const ssd_config *cfg, int input, const ssd_intrinsics *intr, const void *frame, const uint8_t *labels,
                                   const ssd_frame_gates *gates, int n_surfaces, int ground, ssd_frame_moments *out)
{
  if(!gates)
    return fail(SSD_E_ARG, "ssd_surface_refit_moments_host: null gates");
  return surface_moments_walk("ssd_surface_refit_moments_host", cfg, input, intr, frame, labels, gates, n_surfaces, ground, out);
}

/* host only: no handle, no device */
int ssd_camera_ground_gates(const ssd_frame_moments *moments, const uint16_t *camera_of_frame, int nframes, const ssd_camera_drift *drift,
                            int ncams, double k_sigma, double gate_min, ssd_frame_gates *gates)
{
  if(!moments || !camera_of_frame || !drift || !gates || nframes < 0)
    return fail(SSD_E_ARG, "ssd_camera_ground_gates: bad argument");
  if(ncams < 1 || ncams > SSD_MAX_CAMERAS)
    return fail(SSD_E_ARG, "ssd_camera_ground_gates: ncams must be 1.." + std::to_string(SSD_MAX_CAMERAS));
  for(int i = 0; i < nframes; i++)
    if(camera_of_frame[i] >= ncams)
      return fail(SSD_E_ARG, "ssd_camera_ground_gates: frame " + std::to_string(i) + " names camera " + std::to_string(camera_of_frame[i]) + " of " + std::to_string(ncams));
  const int rc = check_gate_rule("ssd_camera_ground_gates", k_sigma, gate_min);
  if(rc) return rc;
  for(int i = 0; i < nframes; i++)
  {
    const ssd_ground_fit &fit = drift[camera_of_frame[i]].fit;
    if(moments[i].ground != 1 || moments[i].n_surfaces < 1 || fit.status != SSD_GF_OK)
      continue;
    ssd_plane_gate &g = gates[i].g[0];
    for(int k = 0; k < 3; k++)
      g.n[k] = fit.normal[k];
    g.dist = fit.dist;
    const double wide = k_sigma * fit.rms;
    g.gate = wide > gate_min ? wide : gate_min;
    if(gates[i].n_surfaces < 1)
      gates[i].n_surfaces = 1;
  }
  return SSD_OK;
}

/* ---- tread clearance (include/ssd_hip.h) ------------------------------------------------------------------ */

int check_clearance_rule(const std::string &who, const ssd_clearance_rule *rule)
{
  if(!rule)
    return fail(SSD_E_ARG, who + ": null rule");
  if(!clearance_rule_ok(*rule))
    return fail(SSD_E_ARG, who + ": the rule must have margin in [0, 1], lo in (0, 1] and hi in (lo, 8]");
  return SSD_OK;
}

/* host only: the rule of ssd_clearance.h over one frame, point by point in the order of the text */
int ssd_clearance_host(const ssd_config *cfg, const ssd_calibration *cal, int input, const ssd_intrinsics *intr, const void *frame,
                       const ssd_frame_result *result, int ground, const ssd_clearance_rule *rule, ssd_frame_moments *out, uint8_t *mask)
{
  const std::string who("ssd_clearance_host");
  int rc = host_frame_check(who, cal && result, cfg, input, intr, frame, result ? result->n_steps : 0, "n_steps", false);
  if(!rc) rc = check_clearance_rule(who, rule);
  if(rc) return rc;
  std::vector<float> deprojected;
  const float *xyz;
  rc = host_frame_xyz(cfg, input, intr, frame, deprojected, xyz);
  if(rc) return rc;
  if(out)
    std::memset(out, 0, sizeof(*out));
  if(mask)
    std::memset(mask, 0, static_cast<size_t>(cfg->width) * cfg->height);
  const HostSurfaces T(result, cal, rule->margin);
  const int n = T.n;
  if(n == 0)
    return SSD_OK;                               /* no occupant: an all-zero record, as the surface moments' */
  long long acc[SSD_MAX_STEPS][kGroundSums + 1] = {};
  T.walk(cfg, cal, xyz, [&](size_t i, double x, double y, double z, double ex, double ey, double ez)
  {
    if(clearance_in_slab(T.S, n, ez, rule->lo))
      return;
    const int k = clearance_lowest(T.S, (1u << n) - 1u, ex, ey, ez, rule->lo, rule->hi);      /* every surface is a candidate; n <= 17 */
    if(k < 0)
      return;
    if(mask)
      mask[i] = static_cast<uint8_t>(k + 1);
    const double rx = moment_round(x), ry = moment_round(y), rz = moment_round(z);
    if(moment_near(rx) && moment_near(ry) && moment_near(rz))
      moment_add(rx, ry, rz, acc[k]);
    else
      acc[k][kGroundSums] += 1;
  });
  if(out)
  {
    out->n_surfaces = n;
    out->ground = ground ? 1 : 0;
    std::memcpy(out->s, acc, sizeof(acc));
  }
  return SSD_OK;
}

int ssd_clearance_solve(const ssd_frame_moments *moments, const ssd_frame_result *result, const ssd_calibration *cal, int min_support,
                        ssd_frame_clearance *out)
{
  if(!moments || !result || !cal || !out)
    return fail(SSD_E_ARG, "ssd_clearance_solve: null");
  if(moments->n_surfaces < 0 || moments->n_surfaces > SSD_MAX_STEPS)
    return fail(SSD_E_ARG, "ssd_clearance_solve: n_surfaces must lie in 0 .. SSD_MAX_STEPS");
  std::memset(out, 0, sizeof(*out));
  out->n_surfaces = moments->n_surfaces;
  out->ground = moments->ground;
  for(int k = 0; k < moments->n_surfaces; k++)
  {
    const ssd_ground_moments &m = moments->s[k].m;
    ssd_clearance &f = out->s[k];
    f.n = m.n;
    f.n_far = moments->s[k].n_far;
    f.status = f.n + f.n_far >= (min_support > 1 ? min_support : 1) ? SSD_CL_OCCUPIED : SSD_CL_FREE;
    if(f.status != SSD_CL_OCCUPIED || m.n < 1)
      continue;
    /* the centroid as ssd_surface_fit_solve forms it: camera coordinates, CameraToWorld, ToExternalWorld */
    const double nd = static_cast<double>(m.n);
    double c[3], w[3];
    for(int i = 0; i < 3; i++)
      c[i] = static_cast<double>(m.s[i]) / (nd * kGroundScale);
    for(int i = 0; i < 3; i++)
      w[i] = ((cal->a[3 * i] * c[0] + cal->a[3 * i + 1] * c[1]) + cal->a[3 * i + 2] * c[2]) + cal->b[i];
    f.centroid[0] = (cal->r2[0] * w[0] + cal->r2[1] * w[1]) + cal->t2[0];
    f.centroid[1] = (cal->r2[2] * w[0] + cal->r2[3] * w[1]) + cal->t2[1];
    f.centroid[2] = w[2] + cal->world_z;
    const ssd_step &st = result->steps[k];
    f.height_mean = f.centroid[2] - st.height;
    /* the centred scatter N SS - S (x) S, exact in 128-bit integers, in m^2 (plane_of_moments' statement: ssd_solve.h) */
    typedef __int128 i128;
    const double scale = 1.0 / (nd * nd * kGroundScale * kGroundScale);
    const int64_t ss[3][3] = { { m.ss[0], m.ss[1], m.ss[2] }, { m.ss[1], m.ss[3], m.ss[4] }, { m.ss[2], m.ss[4], m.ss[5] } };
    double sc[3][3], lambda[3], v[3][3];
    for(int i = 0; i < 3; i++)
      for(int j = 0; j < 3; j++)
        sc[i][j] = static_cast<double>(static_cast<i128>(m.n) * ss[i][j] - static_cast<i128>(m.s[i]) * m.s[j]) * scale;
    /* the variance along the world's up axis: row 3 of a */
    const double *up = cal->a + 6;
    double var = 0.0;
    for(int i = 0; i < 3; i++)
      var += up[i] * ((sc[i][0] * up[0] + sc[i][1] * up[1]) + sc[i][2] * up[2]);
    f.height_rms = std::sqrt(var > 0.0 ? var : 0.0);
    /* against the front edge FL -> FR: along it from FL, and behind it (towards the ring's inside) */
    const double dx = st.quad[2] - st.quad[0], dy = st.quad[3] - st.quad[1], len = std::sqrt(dx * dx + dy * dy);
    ClearanceSurface S;
    clearance_surface(st, 0.0, S);
    if(len > 0.0)
    {
      const double px = f.centroid[0] - st.quad[0], py = f.centroid[1] - st.quad[1];
      f.along_front = (px * dx + py * dy) / len;
      f.from_front = S.o * (dx * py - dy * px) / len;
    }
    jacobi3(sc, lambda, v);
    for(int i = 0; i < 3; i++)
      f.extent[i] = std::sqrt(lambda[2 - i] > 0.0 ? lambda[2 - i] : 0.0);
  }
  return SSD_OK;
}

/* ---- tread grid (include/ssd_hip.h) ----------------------------------------------------------------------- */

int check_tread_grid_rule(const std::string &who, const ssd_tread_grid_rule *rule)
{
  if(!rule)
    return fail(SSD_E_ARG, who + ": null rule");
  const int rc = check_clearance_rule(who, &rule->clearance);
  if(rc) return rc;
  if(!tread_grid_rule_ok(*rule))
    return fail(SSD_E_ARG, who + ": the rule must have cell in [0.005, 1]");
  return SSD_OK;
}

/* host only: the rule of ssd_treadgrid.h over one frame, point by point in the order of the text */
int ssd_tread_grid_host(const ssd_config *cfg, const ssd_calibration *cal, int input, const ssd_intrinsics *intr, const void *frame,
                        const ssd_frame_result *result, int ground, const ssd_tread_grid_rule *rule, ssd_frame_tread_grid *out)
{
  const std::string who("ssd_tread_grid_host");
  int rc = host_frame_check(who, cal && result && out, cfg, input, intr, frame, result ? result->n_steps : 0, "n_steps", false);
  if(!rc) rc = check_tread_grid_rule(who, rule);
  if(rc) return rc;
  std::vector<float> deprojected;
  const float *xyz;
  rc = host_frame_xyz(cfg, input, intr, frame, deprojected, xyz);
  if(rc) return rc;
  std::memset(out, 0, sizeof(*out));
  const HostSurfaces T(result, cal, rule->clearance.margin);
  const int n = T.n;
  if(n == 0)
    return SSD_OK;                               /* nothing counted: an all-zero record, as the clearance moments' */
  out->n_surfaces = n;
  out->ground = ground ? 1 : 0;
  const double lo = rule->clearance.lo, hi = rule->clearance.hi;
  TreadGridAxes G[SSD_MAX_STEPS];
  for(int k = 0; k < n; k++)
    tread_grid_axes(T.S[k], G[k]);
  const unsigned int all = (1u << n) - 1u;       /* every surface is a candidate; n <= 17 */
  T.walk(cfg, cal, xyz, [&](size_t, double, double, double, double ex, double ey, double ez)
  {
    const bool tread = clearance_in_slab(T.S, n, ez, lo);
    const int k = tread ? tread_grid_lowest(T.S, all, ex, ey, ez, lo) : clearance_lowest(T.S, all, ex, ey, ez, lo, hi);
    if(k < 0)
      return;
    ssd_tread_grid &g = out->s[k];
    int row, col;
    const bool in = tread_grid_cell(G[k], rule->cell, ex, ey, row, col);
    if(tread)
      (in ? g.seen[row][col] : g.n_seen_out) += 1u;
    else
    {
      (in ? g.occ[row][col] : g.n_occ_out) += 1u;
      const int32_t t = tread_grid_top(ez, T.S[k].height);
      int32_t &top = in ? g.top[row][col] : g.top_out;
      if(t > top)
        top = t;
    }
  });
  return SSD_OK;
}

int ssd_tread_grid_solve(const ssd_frame_tread_grid *grid, const ssd_frame_result *result, const ssd_tread_grid_rule *rule, int min_seen,
                         int min_occ, double foot_along, double foot_deep, ssd_frame_footholds *out)
{
  const std::string who("ssd_tread_grid_solve");
  if(!grid || !result || !out)
    return fail(SSD_E_ARG, who + ": null");
  if(grid->n_surfaces < 0 || grid->n_surfaces > SSD_MAX_STEPS)
    return fail(SSD_E_ARG, who + ": n_surfaces must lie in 0 .. SSD_MAX_STEPS");
  const int rc = check_tread_grid_rule(who, rule);
  if(rc) return rc;
  if(!(foot_along >= 0.0) || !(foot_deep >= 0.0))
    return fail(SSD_E_ARG, who + ": a foot size must be 0 or more");
  std::memset(out, 0, sizeof(*out));
  out->n_surfaces = grid->n_surfaces;
  out->ground = grid->ground;
  const double cell = rule->cell;
  /* the least rectangle that holds the foot, in cells (as doubles: a foot no grid holds finds nothing) */
  const double needCols = std::fmax(std::ceil(foot_along / cell), 1.0), needRows = std::fmax(std::ceil(foot_deep / cell), 1.0);
  const uint32_t minSeen = min_seen > 1 ? static_cast<uint32_t>(min_seen) : 1u, minOcc = min_occ > 1 ? static_cast<uint32_t>(min_occ) : 1u;
  for(int k = 0; k < grid->n_surfaces; k++)
  {
    const ssd_tread_grid &g = grid->s[k];
    ssd_foothold &f = out->s[k];
    ClearanceSurface S;
    TreadGridAxes G;
    clearance_surface(result->steps[k], rule->clearance.margin, S);
    tread_grid_axes(S, G);
    int32_t top = g.top_out;
    for(int r = 0; r < SSD_TG_ROWS; r++)
      for(int c = 0; c < SSD_TG_COLS; c++)
      {
        double x, y;
        tread_grid_world(G, cell, r + 0.5, c + 0.5, x, y);
        uint8_t s = SSD_TG_UNSEEN;
        if(!G.live || !clearance_inside(S, x, y))
          s = SSD_TG_OUT;
        else if(g.occ[r][c] >= minOcc)
          s = SSD_TG_OCCUPIED;
        else if(g.seen[r][c] >= minSeen)
          s = SSD_TG_FREE;
        f.state[r][c] = s;
        f.n_free += s == SSD_TG_FREE;
        f.n_occupied += s == SSD_TG_OCCUPIED;
        f.n_unseen += s == SSD_TG_UNSEEN;
        if(g.top[r][c] > top)
          top = g.top[r][c];
      }
    f.tallest = static_cast<double>(top) / 65536.0;
    /* the largest all-FREE rectangle: for every first row and height the columns free in all its rows, and their maximal runs - the
     * best rectangle is a maximal run of its rows (a shorter one has less area).  Ties: the smallest row0 (the outer loop's order
     * with a strict comparison), then the smallest col0, then the most cols */
    int bestArea = 0;
    for(int r0 = 0; r0 < SSD_TG_ROWS; r0++)
    {
      bool freeCol[SSD_TG_COLS];
      for(int c = 0; c < SSD_TG_COLS; c++)
        freeCol[c] = true;
      for(int rows = 1; r0 + rows <= SSD_TG_ROWS; rows++)
      {
        for(int c = 0; c < SSD_TG_COLS; c++)
          freeCol[c] = freeCol[c] && f.state[r0 + rows - 1][c] == SSD_TG_FREE;
        if(static_cast<double>(rows) < needRows)
          continue;
        for(int c = 0; c < SSD_TG_COLS;)
        {
          if(!freeCol[c])
          {
            c++;
            continue;
          }
          int end = c;
          while(end < SSD_TG_COLS && freeCol[end])
            end++;
          const int cols = end - c, area = cols * rows;
          if(static_cast<double>(cols) >= needCols)
          {
            const bool better = area > bestArea
              || (area == bestArea && r0 == f.row0 && (c < f.col0 || (c == f.col0 && cols > f.cols)));
            if(better)
            {
              bestArea = area;
              f.row0 = r0; f.col0 = c; f.rows = rows; f.cols = cols;
            }
          }
          c = end;
        }
      }
    }
    if(bestArea > 0)
    {
      f.foothold = 1;
      tread_grid_world(G, cell, f.row0 + 0.5 * f.rows, f.col0 + 0.5 * f.cols, f.centre[0], f.centre[1]);
      f.size[0] = f.cols * cell;
      f.size[1] = f.rows * cell;
    }
  }
  return SSD_OK;
}

/* ---- stair map (include/ssd_hip.h) ------------------------------------------------------------------------ */

int ssd_tread_grid_add(const ssd_frame_tread_grid *in, ssd_frame_tread_grid *acc)
{
  if(!in || !acc)
    return fail(SSD_E_ARG, "ssd_tread_grid_add: null");
  if(!tread_grid_add(*in, *acc))
    return fail(SSD_E_CAP, "ssd_tread_grid_add: a count would pass 2^32 - 1; the record is as it was");
  return SSD_OK;
}

int ssd_stair_map_from_results(const ssd_frame_result *results, int nframes, int ground, ssd_stair_map *out, int *n_used)
{
  if(!results || !out || nframes < 0)
    return fail(SSD_E_ARG, "ssd_stair_map_from_results: null, or nframes below 0");
  std::memset(out, 0, sizeof(*out));
  out->ground = ground;
  if(n_used)
    *n_used = 0;
  /* the usable frames, and how often each n_steps occurs among them */
  std::vector<int> usable;
  int votes[SSD_MAX_STEPS + 1] = {};
  for(int i = 0; i < nframes; i++)
  {
    const ssd_frame_result &r = results[i];
    if((r.status & (SSD_ST_THROW | SSD_ST_OVERFLOW)) != 0 || r.n_steps <= 0 || r.n_steps > SSD_MAX_STEPS)
      continue;
    bool finite = true;
    for(int k = 0; k < r.n_steps && finite; k++)
    {
      finite = std::isfinite(r.steps[k].height);
      for(int j = 0; j < 8 && finite; j++)
        finite = std::isfinite(r.steps[k].quad[j]);
    }
    if(!finite)
      continue;
    usable.push_back(i);
    votes[r.n_steps]++;
  }
  int mode = 0;
  for(int n = 1; n <= SSD_MAX_STEPS; n++)
    if(votes[n] > 0 && votes[n] >= votes[mode])       /* ties go to the larger */
      mode = n;
  if(mode == 0)
    return SSD_OK;
  std::vector<double> v;
  /* the lower median of one field over the kept frames: the values only, sorted - finite, so the order is total */
  auto median = [&](auto field)
  {
    v.clear();
    for(int i : usable)
      if(results[i].n_steps == mode)
        v.push_back(field(results[i]));
    std::sort(v.begin(), v.end());
    return v[(v.size() - 1) / 2];
  };
  out->stairs.n_steps = mode;
  for(int k = 0; k < mode; k++)
  {
    out->stairs.steps[k].height = median([k](const ssd_frame_result &r) { return r.steps[k].height; });
    for(int j = 0; j < 8; j++)
      out->stairs.steps[k].quad[j] = median([k, j](const ssd_frame_result &r) { return r.steps[k].quad[j]; });
  }
  if(n_used)
    *n_used = votes[mode];
  return SSD_OK;
}

/* ---- riser fit (include/ssd_hip.h): host side ------------------------------------------------------------ */

int ssd_riser_fit_solve(const ssd_frame_moments *moments, const ssd_frame_risers *risers, const ssd_calibration *cal, int min_points,
                        ssd_frame_riser_fits *out)
{
  if(!moments || !risers || !cal || !out)
    return fail(SSD_E_ARG, "ssd_riser_fit_solve: null");
  if(moments->n_surfaces < 0 || moments->n_surfaces > SSD_MAX_RISERS || moments->n_surfaces != risers->n_risers)
    return fail(SSD_E_ARG, "ssd_riser_fit_solve: n_surfaces must lie in 0 .. SSD_MAX_RISERS and be the risers' n_risers");
  std::memset(out, 0, sizeof(*out));
  const int nR = moments->n_surfaces;
  out->n_risers = nR;
  double hdir[SSD_MAX_RISERS][2] = {};      /* the unit horizontal projection of each OK normal (0, 0: horizontal normal) */
  for(int i = 0; i < nR; i++)
  {
    const ssd_surface_moments &sm = moments->s[i];
    const ssd_riser &q = risers->risers[i];
    ssd_riser_fit &f = out->r[i];
    f.n = sm.m.n;
    f.n_far = sm.n_far;
    f.rise = q.height_top - q.height_bottom;
    PlaneOfMoments pl;
    f.status = plane_of_moments(&sm.m, min_points, pl);
    if(f.status != SSD_GF_OK)
      continue;
    /* normal and centroid exactly as ssd_surface_fit_solve takes them: n0 points away from the camera, so -(A n0) looks at it */
    double nw[3], w[3];
    for(int k = 0; k < 3; k++)
    {
      nw[k] = -((cal->a[3 * k] * pl.n0[0] + cal->a[3 * k + 1] * pl.n0[1]) + cal->a[3 * k + 2] * pl.n0[2]);
      w[k] = ((cal->a[3 * k] * pl.centroid[0] + cal->a[3 * k + 1] * pl.centroid[1]) + cal->a[3 * k + 2] * pl.centroid[2]) + cal->b[k];
    }
    f.normal[0] = cal->r2[0] * nw[0] + cal->r2[1] * nw[1];
    f.normal[1] = cal->r2[2] * nw[0] + cal->r2[3] * nw[1];
    f.normal[2] = nw[2];
    f.centroid[0] = (cal->r2[0] * w[0] + cal->r2[1] * w[1]) + cal->t2[0];
    f.centroid[1] = (cal->r2[2] * w[0] + cal->r2[3] * w[1]) + cal->t2[1];
    f.centroid[2] = w[2] + cal->world_z;
    const double nz = f.normal[2] > 1.0 ? 1.0 : f.normal[2] < -1.0 ? -1.0 : f.normal[2];
    f.lean = std::asin(nz);
    const double hl = std::sqrt(f.normal[0] * f.normal[0] + f.normal[1] * f.normal[1]);
    const double ex = q.right[0] - q.left[0], ey = q.right[1] - q.left[1];
    const double el = std::sqrt(ex * ex + ey * ey);
    if(hl > 0.0)
    {
      hdir[i][0] = f.normal[0] / hl;
      hdir[i][1] = f.normal[1] / hl;
    }
    if(hl > 0.0 && el > 0.0)
    {
      const double d = std::fabs(hdir[i][0] * (ex / el) + hdir[i][1] * (ey / el));
      f.skew = std::asin(d > 1.0 ? 1.0 : d);
    }
    f.rms = std::sqrt(pl.lambda[0] > 0.0 ? pl.lambda[0] : 0.0);
    f.extent[0] = std::sqrt(pl.lambda[2]);
    f.extent[1] = std::sqrt(pl.lambda[1]);
  }
  for(int i = 0; i + 1 < nR; i++)
  {
    const ssd_riser_fit &a = out->r[i], &b = out->r[i + 1];
    if(a.status == SSD_GF_OK && b.status == SSD_GF_OK)
      out->r[i].going = std::fabs((b.centroid[0] - a.centroid[0]) * hdir[i][0] + (b.centroid[1] - a.centroid[1]) * hdir[i][1]);
  }
  return SSD_OK;
}

/* host only: no handle, no device */
int ssd_camera_drift_fold(const ssd_frame_moments *moments, const uint16_t *camera_of_frame, int nframes, const ssd_camera *cams, int ncams,
                          int min_points, ssd_camera_drift *out)
{
  if(!moments || !camera_of_frame || !cams || !out || nframes < 0)
    return fail(SSD_E_ARG, "ssd_camera_drift_fold: bad argument");
  if(ncams < 1 || ncams > SSD_MAX_CAMERAS)
    return fail(SSD_E_ARG, "ssd_camera_drift_fold: ncams must be 1.." + std::to_string(SSD_MAX_CAMERAS));
  for(int i = 0; i < nframes; i++)
    if(camera_of_frame[i] >= ncams)
      return fail(SSD_E_ARG, "ssd_camera_drift_fold: frame " + std::to_string(i) + " names camera " + std::to_string(camera_of_frame[i]) + " of " + std::to_string(ncams));
  static_assert(kFoldSums == kGroundSums + 1, "the fold's sums are the ground fit's ten and n_far");
  std::memset(out, 0, sizeof(ssd_camera_drift) * static_cast<size_t>(ncams));
  for(int c = 0; c < ncams; c++)
    out[c].camera = c;
  /* in index order; a frame whole or not at all: ssd_fold.h's step, which k_camera_fold runs too */
  for(int i = 0; i < nframes; i++)
    fold_step(out[camera_of_frame[i]], moments[i]);
  for(int c = 0; c < ncams; c++)
  {
    const int rc = ssd_ground_fit_solve(&out[c].m, &cams[c].cal, min_points, &out[c].fit);
    if(rc) return rc;
  }
  return SSD_OK;
}

/* host only: no handle, no device */
int ssd_camera_drift_from_fold(const ssd_camera_fold *fold, const ssd_camera *cams, int ncams, int min_points, ssd_camera_drift *out)
{
  if(!fold || !cams || !out)
    return fail(SSD_E_ARG, "ssd_camera_drift_from_fold: null");
  if(ncams < 1 || ncams > SSD_MAX_CAMERAS)
    return fail(SSD_E_ARG, "ssd_camera_drift_from_fold: ncams must be 1.." + std::to_string(SSD_MAX_CAMERAS));
  for(int c = 0; c < ncams; c++)
    if(fold[c].camera != c)
      return fail(SSD_E_ARG, "ssd_camera_drift_from_fold: record " + std::to_string(c) + " names camera " + std::to_string(fold[c].camera));
  static_assert(offsetof(ssd_camera_drift, fit) == sizeof(ssd_camera_fold), "ssd_camera_fold is the head of ssd_camera_drift");
  std::memset(out, 0, sizeof(ssd_camera_drift) * static_cast<size_t>(ncams));
  for(int c = 0; c < ncams; c++)
  {
    ssd_camera_drift &d = out[c];
    d.camera = fold[c].camera; d.frames = fold[c].frames; d.frames_ground = fold[c].frames_ground; d.frames_left = fold[c].frames_left;
    d.m = fold[c].m;
    d.n_far = fold[c].n_far;
    const int rc = ssd_ground_fit_solve(&d.m, &cams[c].cal, min_points, &d.fit);
    if(rc) return rc;
  }
  return SSD_OK;
}

/* ---- stair pose: a camera located against a stair map (include/ssd_hip.h) ------------------------------------ */

/* the refusals about the rule, the targets and the index that the host statement, the enqueue and the host form share */
int check_pose_rule(const std::string &me, const ssd_stair_pose_rule *rule)
{
  if(!rule)
    return fail(SSD_E_ARG, me + ": null rule");
  if(!pose_rule_ok(*rule))
    return fail(SSD_E_ARG, me + ": margin must lie in [0, 1], band, clear and reach in (0, 1]");
  return SSD_OK;
}

int check_pose_targets(const std::string &me, const ssd_stair_pose_target *targets, int ntargets, const uint16_t *target_of_frame, int nframes, int input)
{
  if(!targets)
    return fail(SSD_E_ARG, me + ": null targets");
  if(ntargets < 1 || ntargets > SSD_MAX_STAIR_MAPS)
    return fail(SSD_E_ARG, me + ": ntargets must lie in 1 .. SSD_MAX_STAIR_MAPS");
  for(int t = 0; t < ntargets; t++)
  {
    if(targets[t].map.stairs.n_steps < 0 || targets[t].map.stairs.n_steps > SSD_MAX_STEPS)
      return fail(SSD_E_ARG, me + ": a map's n_steps must lie in 0 .. SSD_MAX_STEPS");
    if(input == SSD_INPUT_DEPTH16 && (!targets[t].prior.has_intrinsics || !good_intrinsics(targets[t].prior.intr)))
      return fail(SSD_E_ARG, me + ": depth input, and target " + std::to_string(t) + " has no (valid) intrinsics");
  }
  for(int i = 0; i < nframes && target_of_frame; i++)
    if(target_of_frame[i] != SSD_STAIR_MAP_NONE && target_of_frame[i] >= ntargets)
      return fail(SSD_E_ARG, me + ": target_of_frame holds an index that is neither below ntargets nor SSD_STAIR_MAP_NONE");
  return SSD_OK;
}

int ssd_stair_pose_host(const ssd_config *cfg, const ssd_stair_pose_target *target, int input, const void *frame, const ssd_stair_pose_rule *rule,
                        ssd_stair_pose_moments *out)
{
  const std::string me("ssd_stair_pose_host");
  if(!cfg || !target || !frame || !out || cfg->width <= 0 || cfg->height <= 0)
    return fail(SSD_E_ARG, me + ": bad argument");
  if(input != SSD_INPUT_VERTICES && input != SSD_INPUT_DEPTH16)
    return fail(SSD_E_ARG, me + ": input must be SSD_INPUT_VERTICES or SSD_INPUT_DEPTH16");
  int rc = check_pose_rule(me, rule);
  if(!rc) rc = check_pose_targets(me, target, 1, nullptr, 0, input);
  if(rc) return rc;
  const bool depth = input == SSD_INPUT_DEPTH16;
  PoseTarget T;
  pose_target_fill(T, *target, depth, *rule);
  std::memset(out, 0, sizeof(*out));
  if(T.nSteps == 0)
    return SSD_OK;
  const PoseRange R{ cfg->x_min, cfg->x_max, cfg->y_min, cfg->y_max };
  const int W = cfg->width, H = cfg->height;
  long long acc[kPoseClasses][kPoseSums] = {};
  auto take = [&](float x, float y, float z)
  {
    const int c = pose_class(T.cam, T.world, T, R, x, y, z);
    if(c >= 0)
      pose_add(x, y, z, acc[c]);
  };
  if(depth)
  {
    const uint16_t *d16 = static_cast<const uint16_t *>(frame);
    std::vector<float> xm(static_cast<size_t>(W));
    for(int u = 0; u < W; u++)
      xm[u] = ground_map_x(T.cam, u);
    for(int v = 0; v < H; v++)
    {
      const float ym = ground_map_y(T.cam, v);
      for(int u = 0; u < W; u++)
      {
        const float d = static_cast<float>(d16[static_cast<size_t>(v) * W + u]) * T.cam.depthUnits;
        take(d * xm[u], d * ym, d);
      }
    }
  }
  else
  {
    const float *xyz = static_cast<const float *>(frame);
    for(size_t i = 0, n = static_cast<size_t>(W) * H; i < n; i++)
      take(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  }
  int64_t *rec = reinterpret_cast<int64_t *>(out);
  for(int c = 0; c < kPoseClasses; c++)
    for(int j = 0; j < kPoseSums; j++)
      rec[pose_word(c) + j] = acc[c][j];
  int32_t head[4];
  pose_headers(T.nSteps, T.ground, head);
  out->treads.n_surfaces = head[0]; out->treads.ground = head[1];
  out->risers.n_surfaces = head[2]; out->risers.ground = head[3];
  return SSD_OK;
}

int ssd_stair_pose_add(const ssd_stair_pose_moments *in, ssd_stair_pose_moments *acc)
{
  if(!in || !acc)
    return fail(SSD_E_ARG, "ssd_stair_pose_add: null");
  if(!pose_fold(*in, *acc))
    return fail(SSD_E_CAP, "ssd_stair_pose_add: a sum would leave int64; acc is untouched");
  return SSD_OK;
}

/* eigenvalues (ascending) and eigenvectors (columns of v) of a symmetric 6 x 6 matrix: cyclic Jacobi with jacobi3's rotation, host only
 * (ssd_solve.h is the device's too and stays as it is).  An off-diagonal entry that no longer changes either of its diagonal
 * neighbours when added to them is set to zero. */
static void jacobi6(double a[6][6], double lambda[6], double v[6][6])
{
  for(int i = 0; i < 6; i++)
    for(int j = 0; j < 6; j++)
      v[i][j] = i == j ? 1.0 : 0.0;
  for(int sweep = 0; sweep < 64; sweep++)
  {
    double off = 0.0;
    for(int p = 0; p < 5; p++)
      for(int q = p + 1; q < 6; q++)
        off += std::fabs(a[p][q]);
    if(off == 0.0)
      break;
    for(int p = 0; p < 5; p++)
      for(int q = p + 1; q < 6; q++)
      {
        const double apq = a[p][q], app = a[p][p], aqq = a[q][q];
        if(apq == 0.0)
          continue;
        if(std::fabs(app) + std::fabs(apq) == std::fabs(app) && std::fabs(aqq) + std::fabs(apq) == std::fabs(aqq))
        {
          a[p][q] = a[q][p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        a[p][p] = app - t * apq;
        a[q][q] = aqq + t * apq;
        a[p][q] = a[q][p] = 0.0;
        for(int r = 0; r < 6; r++)
        {
          if(r != p && r != q)
          {
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][q] = a[q][r] = s * arp + c * arq;
          }
          const double vrp = v[r][p], vrq = v[r][q];
          v[r][p] = c * vrp - s * vrq;
          v[r][q] = s * vrp + c * vrq;
        }
      }
  }
  int order[6] = { 0, 1, 2, 3, 4, 5 };
  for(int i = 1; i < 6; i++)                       /* a stable insertion sort of the diagonal by < */
    for(int j = i; j > 0 && a[order[j]][order[j]] < a[order[j - 1]][order[j - 1]]; j--)
      std::swap(order[j], order[j - 1]);
  double vv[6][6];
  for(int k = 0; k < 6; k++)
  {
    lambda[k] = a[order[k]][order[k]];
    for(int i = 0; i < 6; i++)
      vv[i][k] = v[i][order[k]];
  }
  std::memcpy(v, vv, sizeof(vv));
}

/* one class of the solve: its points' count, centroid and centred covariance in the external world, and its plane */
struct PoseClassFit
{
  double n, e[3], S[3][3], nrm[3], d;
};

/* a class's moments under the prior's affine map e = T p + c: the centroid and the centred scatter exact in 128-bit integers
 * (plane_of_moments' statement: ssd_solve.h), doubles from there on */
static void pose_class_fit(const ssd_ground_moments &m, const double T[3][3], const double c[3], PoseClassFit &f)
{
  typedef __int128 i128;
  const double nd = static_cast<double>(m.n);
  const double scale = 1.0 / (nd * nd * kGroundScale * kGroundScale);
  const int64_t s[3] = { m.s[0], m.s[1], m.s[2] };
  const int64_t ss[3][3] = { { m.ss[0], m.ss[1], m.ss[2] }, { m.ss[1], m.ss[3], m.ss[4] }, { m.ss[2], m.ss[4], m.ss[5] } };
  double pc[3], cc[3][3], tc[3][3];
  for(int i = 0; i < 3; i++)
  {
    pc[i] = static_cast<double>(s[i]) / (nd * kGroundScale);
    for(int j = 0; j < 3; j++)
      cc[i][j] = static_cast<double>(static_cast<i128>(m.n) * ss[i][j] - static_cast<i128>(s[i]) * s[j]) * scale;
  }
  f.n = nd;
  for(int i = 0; i < 3; i++)
  {
    f.e[i] = ((T[i][0] * pc[0] + T[i][1] * pc[1]) + T[i][2] * pc[2]) + c[i];
    for(int j = 0; j < 3; j++)
      tc[i][j] = (T[i][0] * cc[0][j] + T[i][1] * cc[1][j]) + T[i][2] * cc[2][j];
  }
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
      f.S[i][j] = (tc[i][0] * T[j][0] + tc[i][1] * T[j][1]) + tc[i][2] * T[j][2];
}

/* Rot(w) by Rodrigues' formula: I + A [w]x + B [w]x^2, A = sin(th) / th, B = (1 - cos(th)) / th^2 (their limits 1 and 1/2 below 1e-8 rad) */
static void rodrigues(const double w[3], double R[3][3])
{
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(t2);
  const double A = th < 1e-8 ? 1.0 : std::sin(th) / th, B = th < 1e-8 ? 0.5 : (1.0 - std::cos(th)) / t2;
  const double K[3][3] = { { 0.0, -w[2], w[1] }, { w[2], 0.0, -w[0] }, { -w[1], w[0], 0.0 } };
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
    {
      const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
      R[i][j] = (i == j ? 1.0 : 0.0) + A * K[i][j] + B * k2;
    }
}

/* e = T p + c: ToExternalWorld behind CameraToWorld, a calibration as the affine map camera -> external world (ssd_stair_pose_solve,
 * ssd_depth_warp_view_between) */
static void camera_to_external(const ssd_calibration &cal, double (&T)[3][3], double (&c)[3])
{
  for(int j = 0; j < 3; j++)
  {
    T[0][j] = cal.r2[0] * cal.a[j] + cal.r2[1] * cal.a[3 + j];
    T[1][j] = cal.r2[2] * cal.a[j] + cal.r2[3] * cal.a[3 + j];
    T[2][j] = cal.a[6 + j];
  }
  c[0] = (cal.r2[0] * cal.b[0] + cal.r2[1] * cal.b[1]) + cal.t2[0];
  c[1] = (cal.r2[2] * cal.b[0] + cal.r2[3] * cal.b[1]) + cal.t2[1];
  c[2] = cal.b[2] + cal.world_z;
}

int ssd_stair_pose_solve(const ssd_stair_pose_moments *moments, const ssd_stair_pose_target *target, int min_points, double observable,
                         ssd_stair_pose *out)
{
  if(!moments || !target || !out)
    return fail(SSD_E_ARG, "ssd_stair_pose_solve: null");
  const ssd_frame_result &st = target->map.stairs;
  if(st.n_steps < 0 || st.n_steps > SSD_MAX_STEPS)
    return fail(SSD_E_ARG, "ssd_stair_pose_solve: the map's n_steps must lie in 0 .. SSD_MAX_STEPS");
  if(!(observable >= 0.0) || !(observable <= 1.0))
    return fail(SSD_E_ARG, "ssd_stair_pose_solve: observable must lie in [0, 1]");
  const ssd_calibration &prior = target->prior.cal;
  std::memset(out, 0, sizeof(*out));
  out->cal = prior;
  out->status = SSD_GF_FEW;
  const int64_t need = min_points > 1 ? min_points : 1;
  const int nSteps = (st.status & SSD_ST_THROW) ? 0 : st.n_steps;
  double T[3][3], c[3];
  camera_to_external(prior, T, c);
  std::vector<PoseClassFit> used;
  for(int k = 0; k < nSteps; k++)
  {
    const ssd_surface_moments &sm = moments->treads.s[k];
    ClearanceSurface ring;
    clearance_surface(st.steps[k], 0.0, ring);
    if(sm.m.n < need || ring.o == 0.0)
      continue;
    PoseClassFit f;
    pose_class_fit(sm.m, T, c, f);
    f.nrm[0] = 0.0; f.nrm[1] = 0.0; f.nrm[2] = 1.0;
    f.d = st.steps[k].height;
    used.push_back(f);
    out->treads_used |= 1u << k;
    out->n += sm.m.n;
    out->n_far += sm.n_far;
  }
  for(int i = 0; i + 1 < nSteps; i++)
  {
    const ssd_surface_moments &sm = moments->risers.s[i];
    const ssd_step &up = st.steps[i + 1];
    const double dx = up.quad[2] - up.quad[0], dy = up.quad[3] - up.quad[1], l2 = dx * dx + dy * dy;
    if(sm.m.n < need || !(l2 > 0.0))
      continue;
    PoseClassFit f;
    pose_class_fit(sm.m, T, c, f);
    const double len = std::sqrt(l2);
    f.nrm[0] = -dy / len; f.nrm[1] = dx / len; f.nrm[2] = 0.0;
    f.d = f.nrm[0] * up.quad[0] + f.nrm[1] * up.quad[1];
    used.push_back(f);
    out->risers_used |= 1u << i;
    out->n += sm.m.n;
    out->n_far += sm.n_far;
  }
  if(used.empty())
    return SSD_OK;
  out->status = SSD_GF_DEGENERATE;
  /* the centroid of all used points, and their mean squared distance from it */
  double N = 0.0, E[3] = { 0.0, 0.0, 0.0 };
  for(const PoseClassFit &f : used)
  {
    N += f.n;
    for(int i = 0; i < 3; i++)
      E[i] += f.n * f.e[i];
  }
  for(int i = 0; i < 3; i++)
    E[i] /= N;
  double rho2 = 0.0;
  for(const PoseClassFit &f : used)
  {
    const double m[3] = { f.e[0] - E[0], f.e[1] - E[1], f.e[2] - E[2] };
    rho2 += f.n * (((f.S[0][0] + f.S[1][1]) + f.S[2][2]) + ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]));
  }
  rho2 /= N;
  const double rho = std::sqrt(rho2);
  if(!(rho > 0.0) || !std::isfinite(rho))
    return SSD_OK;
  /* per class, with q = e - e_c (mean 0, covariance S) and m = e_c - E: the row J = M q + j0, M = [K; 0], K q = q x n, j0 = [m x n; n], and
   * r = n . q + r_c - so sum J J^T = n (M S M^T + j0 j0^T), sum J r = n (M S n + j0 r_c), sum r r = n (n . S n + r_c r_c) */
  double Hm[6][6] = {}, g[6] = {}, rr = 0.0;
  for(const PoseClassFit &f : used)
  {
    const double *n = f.nrm;
    const double m[3] = { f.e[0] - E[0], f.e[1] - E[1], f.e[2] - E[2] };
    const double K[3][3] = { { 0.0, n[2], -n[1] }, { -n[2], 0.0, n[0] }, { n[1], -n[0], 0.0 } };
    const double j0[6] = { m[1] * n[2] - m[2] * n[1], m[2] * n[0] - m[0] * n[2], m[0] * n[1] - m[1] * n[0], n[0], n[1], n[2] };
    const double rc = ((n[0] * f.e[0] + n[1] * f.e[1]) + n[2] * f.e[2]) - f.d;
    double KS[3][3], KSK[3][3], Sn[3], KSn[3];
    for(int i = 0; i < 3; i++)
    {
      Sn[i] = (f.S[i][0] * n[0] + f.S[i][1] * n[1]) + f.S[i][2] * n[2];
      for(int j = 0; j < 3; j++)
        KS[i][j] = (K[i][0] * f.S[0][j] + K[i][1] * f.S[1][j]) + K[i][2] * f.S[2][j];
    }
    for(int i = 0; i < 3; i++)
    {
      KSn[i] = (KS[i][0] * n[0] + KS[i][1] * n[1]) + KS[i][2] * n[2];
      for(int j = 0; j < 3; j++)
        KSK[i][j] = (KS[i][0] * K[j][0] + KS[i][1] * K[j][1]) + KS[i][2] * K[j][2];
    }
    for(int i = 0; i < 6; i++)
    {
      for(int j = 0; j < 6; j++)
        Hm[i][j] += f.n * ((i < 3 && j < 3 ? KSK[i][j] : 0.0) + j0[i] * j0[j]);
      g[i] += f.n * ((i < 3 ? KSn[i] : 0.0) + j0[i] * rc);
    }
    rr += f.n * (((n[0] * Sn[0] + n[1] * Sn[1]) + n[2] * Sn[2]) + rc * rc);
  }
  /* the rotation columns over rho, everything over the point count: six comparable eigenvalues */
  double Hs[6][6], gs[6], lambda[6], V[6][6];
  for(int i = 0; i < 6; i++)
  {
    const double di = i < 3 ? 1.0 / rho : 1.0;
    gs[i] = g[i] * di / N;
    for(int j = 0; j < 6; j++)
      Hs[i][j] = Hm[i][j] * di * (j < 3 ? 1.0 / rho : 1.0) / N;
  }
  for(int i = 0; i < 6; i++)                      /* exactly symmetric for the rotations */
    for(int j = i + 1; j < 6; j++)
      Hs[i][j] = Hs[j][i] = 0.5 * (Hs[i][j] + Hs[j][i]);
  jacobi6(Hs, lambda, V);
  const double lmax = lambda[5], zero = 64.0 * 2.220446049250313e-16 * lmax;
  double y[6] = {}, gain = 0.0;
  int dof = 0;
  for(int k = 0; k < 6; k++)
  {
    if(!(lmax > 0.0) || !(lambda[k] >= observable * lmax) || !(lambda[k] > zero))
      continue;
    double p = 0.0;
    for(int i = 0; i < 6; i++)
      p += V[i][k] * gs[i];
    for(int i = 0; i < 6; i++)
      y[i] -= V[i][k] * (p / lambda[k]);
    gain += p * p / lambda[k];
    dof++;
  }
  if(dof == 0)
    return SSD_OK;
  const double w[3] = { y[0] / rho, y[1] / rho, y[2] / rho }, tau[3] = { y[3], y[4], y[5] };
  double Rw[3][3], Rp[3][3], cp[3];
  rodrigues(w, Rw);
  for(int i = 0; i < 3; i++)
  {
    for(int j = 0; j < 3; j++)
      Rp[i][j] = (Rw[i][0] * T[0][j] + Rw[i][1] * T[1][j]) + Rw[i][2] * T[2][j];
    cp[i] = (((Rw[i][0] * (c[0] - E[0]) + Rw[i][1] * (c[1] - E[1])) + Rw[i][2] * (c[2] - E[2])) + E[i]) + tau[i];
  }
  ssd_calibration cal = prior;
  if(!camera_to_world_from_plane(-Rp[2][0], -Rp[2][1], -Rp[2][2], cp[2] - prior.world_z, cal.a, cal.b))
    return SSD_OK;
  for(int i = 0; i < 2; i++)
    for(int j = 0; j < 2; j++)
      cal.r2[2 * i + j] = (Rp[i][0] * cal.a[3 * j] + Rp[i][1] * cal.a[3 * j + 1]) + Rp[i][2] * cal.a[3 * j + 2];
  cal.t2[0] = cp[0];
  cal.t2[1] = cp[1];
  bool finite = std::isfinite(cal.t2[0]) && std::isfinite(cal.t2[1]);
  for(int i = 0; i < 4; i++)
    finite = finite && std::isfinite(cal.r2[i]);
  if(!finite)
    return SSD_OK;
  out->status = SSD_GF_OK;
  out->dof = dof;
  out->cal = cal;
  for(int i = 0; i < 3; i++)
  {
    out->rotation[i] = w[i];
    out->translation[i] = tau[i];
    out->centre[i] = E[i];
  }
  for(int k = 0; k < 6; k++)
    out->eig[k] = lambda[k];
  const double before = rr / N, after = before - gain;
  out->rms_before = std::sqrt(before > 0.0 ? before : 0.0);
  out->rms_after = std::sqrt(after > 0.0 ? after : 0.0);
  return SSD_OK;
}

/* frames' records onto their targets' folds, in frame order (index: an int per frame; anything not below ntargets names none) */
int pose_fold_frames(const char *who, const ssd_stair_pose_moments *records, const int *index, int nframes, std::vector<ssd_stair_pose_moments> &folds)
{
  for(int i = 0; i < nframes; i++)
  {
    if(index[i] < 0 || index[i] >= static_cast<int>(folds.size()))
      continue;
    if(!pose_fold(records[i], folds[static_cast<size_t>(index[i])]))
      return fail(SSD_E_CAP, std::string(who) + ": the fold of target " + std::to_string(index[i]) + " would leave int64 at frame " + std::to_string(i));
  }
  return SSD_OK;
}

/* ---- depth fusion: one trimmed-median frame from n frames of a still camera (include/ssd_hip.h) ---------------- */

int ssd_depth_fuse_default_rule(int n, ssd_depth_fuse_rule *rule)
{
  if(!rule || n < 1 || n > SSD_FUSE_MAX_FRAMES)
    return fail(SSD_E_ARG, "ssd_depth_fuse_default_rule: null rule, or n outside 1 .. SSD_FUSE_MAX_FRAMES");
  rule->min_valid = rule->min_agree = (n + 1) / 2;
  rule->tol = SSD_FUSE_TOL;
  rule->reserved = 0;
  return SSD_OK;
}

/* the refusals about n and the rule that the host statement, the enqueue and the host-fed form share; *use: the rule to go by (the
 * defaults for n where the caller gave none) */
int check_fuse_rule(const std::string &me, int n, const ssd_depth_fuse_rule *rule, ssd_depth_fuse_rule *use)
{
  if(n < 1 || n > SSD_FUSE_MAX_FRAMES)
    return fail(SSD_E_ARG, me + ": n must lie in 1 .. SSD_FUSE_MAX_FRAMES");
  if(rule)
    *use = *rule;
  else
    ssd_depth_fuse_default_rule(n, use);
  if(!fuse_rule_ok(n, *use))
    return fail(SSD_E_ARG, me + ": the rule must hold 1 <= min_valid <= n, 1 <= min_agree <= n, 0 <= tol <= 65535");
  return SSD_OK;
}

int ssd_depth_fuse_host(int width, int height, const uint16_t *frames, size_t frame_stride_bytes, int n, const ssd_depth_fuse_rule *rule,
                        uint16_t *out, uint8_t *support, ssd_depth_fuse_stats *stats)
{
  const std::string me("ssd_depth_fuse_host");
  if(!frames || !out || !stats || width <= 0 || height <= 0)
    return fail(SSD_E_ARG, me + ": bad argument");
  ssd_depth_fuse_rule R;
  const int rc = check_fuse_rule(me, n, rule, &R);
  if(rc) return rc;
  const size_t nPoints = static_cast<size_t>(width) * height;
  if(frame_stride_bytes % 2 != 0 || (n > 1 && frame_stride_bytes < nPoints * 2))
    return fail(SSD_E_ARG, me + ": frames must be aligned to their element and the stride must hold a frame");
  int64_t rec[kFuseWords] = {};
  const unsigned char *base = reinterpret_cast<const unsigned char *>(frames);
  for(size_t p = 0; p < nPoints; p++)
  {
    uint32_t d[SSD_FUSE_MAX_FRAMES], sorted[SSD_FUSE_MAX_FRAMES];
    uint32_t m = 0;
    for(int j = 0; j < n; j++)
    {
      uint16_t v;
      std::memcpy(&v, base + static_cast<size_t>(j) * frame_stride_bytes + 2 * p, sizeof(v));
      d[j] = v;
      if(v != 0)
        sorted[m++] = v;
    }
    uint32_t c = 0, s = 0, med = 0;
    if(m > 0)
    {
      std::sort(sorted, sorted + m);
      med = sorted[fuse_median_index(static_cast<int>(m))];
      for(int j = 0; j < n; j++)
        if(fuse_agrees(d[j], med, static_cast<uint32_t>(R.tol)))
        {
          c++;
          s += d[j];
        }
    }
    int cls;
    const uint32_t o = fuse_output(m, c, s, R, cls);
    out[p] = static_cast<uint16_t>(o);
    if(support)
      support[p] = cls == kFuseNFused ? static_cast<uint8_t>(c) : 0;
    rec[cls]++;
    rec[kFuseSumValid] += m;
    if(cls == kFuseNFused)
    {
      rec[kFuseSumAgree] += c;
      for(int j = 0; j < n; j++)
        if(fuse_agrees(d[j], med, static_cast<uint32_t>(R.tol)))
          rec[kFuseSumAbsDev] += fuse_dev(d[j], o);
    }
  }
  std::memcpy(stats, rec, sizeof(*stats));
  return SSD_OK;
}

/* ---- depth edge filter: mixed and lone pixels out of one frame (include/ssd_hip.h) -------------------------------- */

int ssd_depth_edge_default_rule(ssd_depth_edge_rule *rule)
{
  if(!rule)
    return fail(SSD_E_ARG, "ssd_depth_edge_default_rule: null rule");
  rule->min_support = 2;
  rule->bridge = 1;
  rule->tol = SSD_FUSE_TOL;
  rule->slope = SSD_EDGE_SLOPE;
  return SSD_OK;
}

/* the refusals about the rule that the host statement, the enqueue and the host-fed form share; *use: the rule to go by (the defaults
 * where the caller gave none) */
int check_edge_rule(const std::string &me, const ssd_depth_edge_rule *rule, ssd_depth_edge_rule *use)
{
  if(rule)
    *use = *rule;
  else
    ssd_depth_edge_default_rule(use);
  if(!edge_rule_ok(*use))
    return fail(SSD_E_ARG, me + ": the rule must hold 0 <= min_support <= 8, 0 <= tol <= 65535, 0 <= slope <= 4096");
  return SSD_OK;
}

int ssd_depth_edges_host(int width, int height, const uint16_t *frame, const ssd_depth_edge_rule *rule, uint16_t *out, uint8_t *cls,
                         ssd_depth_edge_stats *stats)
{
  const std::string me("ssd_depth_edges_host");
  if(!frame || !out || !stats || width <= 0 || height <= 0)
    return fail(SSD_E_ARG, me + ": bad argument");
  ssd_depth_edge_rule R;
  const int rc = check_edge_rule(me, rule, &R);
  if(rc) return rc;
  int64_t rec[kEdgeWords] = {};
  /* the sample at (x, y), 0 where the frame has no such pixel */
  auto at = [&](int x, int y) -> uint32_t
  {
    return x >= 0 && x < width && y >= 0 && y < height ? frame[static_cast<size_t>(y) * width + x] : 0u;
  };
  for(int y = 0; y < height; y++)
    for(int x = 0; x < width; x++)
    {
      const uint32_t q[8] = { at(x - 1, y - 1), at(x, y - 1), at(x + 1, y - 1), at(x - 1, y), at(x + 1, y), at(x - 1, y + 1), at(x, y + 1), at(x + 1, y + 1) };
      const uint32_t d = at(x, y);
      uint32_t c;
      const int k = edge_pixel(d, q, R, &c);
      const size_t p = static_cast<size_t>(y) * width + x;
      out[p] = k == SSD_EDGE_KEPT ? static_cast<uint16_t>(d) : 0;
      if(cls)
        cls[p] = static_cast<uint8_t>(k);
      rec[k]++;
      if(k == SSD_EDGE_KEPT)
        rec[kEdgeSumSupport] += c;
    }
  std::memcpy(stats, rec, sizeof(*stats));
  return SSD_OK;
}

/* ---- depth warp: the frame another pose would have seen (include/ssd_hip.h) ---------------------------------- */

/* the refusals about the views and the target that the host statement, the enqueue and the host-fed form share */
int check_warp_views(const std::string &me, const ssd_depth_warp_view *views, int nviews, const ssd_intrinsics *dst)
{
  if(!views || !dst)
    return fail(SSD_E_ARG, me + ": null views or dst");
  if(!good_intrinsics(*dst))
    return fail(SSD_E_ARG, me + ": dst holds no valid intrinsics");
  for(int i = 0; i < nviews; i++)
  {
    bool finite = true;
    for(int k = 0; k < 9; k++) finite = finite && std::isfinite(views[i].r[k]);
    for(int k = 0; k < 3; k++) finite = finite && std::isfinite(views[i].t[k]);
    if(!finite || !good_intrinsics(views[i].src))
      return fail(SSD_E_ARG, me + ": view " + std::to_string(i) + " has a non-finite entry or no valid intrinsics");
  }
  return SSD_OK;
}

int ssd_depth_warp_host(int width, int height, const uint16_t *frame, const ssd_depth_warp_view *view, const ssd_intrinsics *dst, uint16_t *out,
                        ssd_depth_warp_stats *stats)
{
  const std::string me("ssd_depth_warp_host");
  if(!frame || !out || !stats || width <= 0 || height <= 0)
    return fail(SSD_E_ARG, me + ": bad argument");
  const int rc = check_warp_views(me, view, 1, dst);
  if(rc) return rc;
  const WarpTarget T = warp_target(*dst);
  const size_t n = static_cast<size_t>(width) * height;
  std::memset(out, 0, n * sizeof(uint16_t));
  std::vector<float> xm(static_cast<size_t>(width));
  for(int u = 0; u < width; u++)
    xm[u] = warp_map_x(view->src, u);
  int64_t rec[kWarpWords] = {};
  for(int v = 0; v < height; v++)
  {
    const float ym = warp_map_y(view->src, v);
    for(int u = 0; u < width; u++)
    {
      int a, b;
      uint32_t q;
      const int cls = warp_sample(*view, T, width, height, frame[static_cast<size_t>(v) * width + u], xm[u], ym, a, b, q);
      rec[cls]++;
      if(cls != kWarpNLanded)
        continue;
      uint16_t &o = out[static_cast<size_t>(b) * width + a];
      if(o == 0)
        rec[kWarpNFilled]++;
      o = static_cast<uint16_t>(warp_min(o, q));
    }
  }
  std::memcpy(stats, rec, sizeof(*stats));
  return SSD_OK;
}

int ssd_depth_warp_view_between(const ssd_camera *src, const ssd_camera *dst, ssd_depth_warp_view *out)
{
  const std::string me("ssd_depth_warp_view_between");
  if(!src || !dst || !out)
    return fail(SSD_E_ARG, me + ": null");
  if(!src->has_intrinsics || !good_intrinsics(src->intr))
    return fail(SSD_E_ARG, me + ": src has no (valid) intrinsics");
  double Ts[3][3], cs[3], Td[3][3], cd[3];
  camera_to_external(src->cal, Ts, cs);
  camera_to_external(dst->cal, Td, cd);
  bool finite = true;
  for(int i = 0; i < 3; i++)
  {
    finite = finite && std::isfinite(cs[i]) && std::isfinite(cd[i]);
    for(int j = 0; j < 3; j++)
      finite = finite && std::isfinite(Ts[i][j]) && std::isfinite(Td[i][j]);
  }
  if(!finite)
    return fail(SSD_E_ARG, me + ": a calibration has a non-finite entry");
  /* T_dst^-1 by cofactors */
  double co[3][3];
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
    {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      co[i][j] = Td[i1][j1] * Td[i2][j2] - Td[i1][j2] * Td[i2][j1];
    }
  const double det = (Td[0][0] * co[0][0] + Td[0][1] * co[0][1]) + Td[0][2] * co[0][2];
  if(!(std::fabs(det) >= 1e-9) || !std::isfinite(det))
    return fail(SSD_E_ARG, me + ": dst's calibration is singular (|det| < 1e-9)");
  double inv[3][3];
  for(int i = 0; i < 3; i++)
    for(int j = 0; j < 3; j++)
      inv[i][j] = co[j][i] / det;
  std::memset(out, 0, sizeof(*out));
  const double dc[3] = { cs[0] - cd[0], cs[1] - cd[1], cs[2] - cd[2] };
  for(int i = 0; i < 3; i++)
  {
    for(int j = 0; j < 3; j++)
      out->r[3 * i + j] = (inv[i][0] * Ts[0][j] + inv[i][1] * Ts[1][j]) + inv[i][2] * Ts[2][j];
    out->t[i] = (inv[i][0] * dc[0] + inv[i][1] * dc[1]) + inv[i][2] * dc[2];
  }
  out->src = src->intr;
  return SSD_OK;
}

/* ---- depth fill: holes and one-pixel see-through closed between agreeing samples (include/ssd_hip.h) ----------------- */

int ssd_depth_fill_default_rule(ssd_depth_fill_rule *rule)
{
  if(!rule)
    return fail(SSD_E_ARG, "ssd_depth_fill_default_rule: null rule");
  rule->min_pairs = 1;
  rule->cover = 1;
  rule->tol = SSD_FUSE_TOL;
  rule->slope = 0;
  return SSD_OK;
}

/* the refusals about the rule that the host statement, the enqueue and the host-fed forms share; *use: the rule to go by (the defaults
 * where the caller gave none) */
int check_fill_rule(const std::string &me, const ssd_depth_fill_rule *rule, ssd_depth_fill_rule *use)
{
  if(rule)
    *use = *rule;
  else
    ssd_depth_fill_default_rule(use);
  if(!fill_rule_ok(*use))
    return fail(SSD_E_ARG, me + ": the rule must hold 1 <= min_pairs <= 4, 0 <= cover <= 4, 0 <= tol <= 65535, 0 <= slope <= 4096");
  return SSD_OK;
}

int ssd_depth_fill_host(int width, int height, const uint16_t *frame, const ssd_depth_fill_rule *rule, uint16_t *out, uint8_t *cls,
                        ssd_depth_fill_stats *stats)
{
  const std::string me("ssd_depth_fill_host");
  if(!frame || !out || !stats || width <= 0 || height <= 0)
    return fail(SSD_E_ARG, me + ": bad argument");
  ssd_depth_fill_rule R;
  const int rc = check_fill_rule(me, rule, &R);
  if(rc) return rc;
  int64_t rec[kFillWords] = {};
  /* the sample at (x, y), 0 where the frame has no such pixel */
  auto at = [&](int x, int y) -> uint32_t
  {
    return x >= 0 && x < width && y >= 0 && y < height ? frame[static_cast<size_t>(y) * width + x] : 0u;
  };
  for(int y = 0; y < height; y++)
    for(int x = 0; x < width; x++)
    {
      const uint32_t q[8] = { at(x - 1, y - 1), at(x, y - 1), at(x + 1, y - 1), at(x - 1, y), at(x + 1, y), at(x - 1, y + 1), at(x, y + 1), at(x + 1, y + 1) };
      uint32_t o, pairs, spread;
      const int k = fill_pixel(at(x, y), q, R, &o, &pairs, &spread);
      const size_t p = static_cast<size_t>(y) * width + x;
      out[p] = static_cast<uint16_t>(o);
      if(cls)
        cls[p] = static_cast<uint8_t>(k);
      rec[k]++;
      rec[kFillSumPairs] += pairs;
      rec[kFillSumSpread] += spread;
    }
  std::memcpy(stats, rec, sizeof(*stats));
  return SSD_OK;
}

/* Stairs::serialize(), stairs.cpp:34-70: ["stairs",["stairSteps",N],[[["height",h],["quadrilateral",[x,y] x4]],...]]
 * fixed notation, 3 decimals; the third element is omitted when N = 0. */
int ssd_serialize(const ssd_frame_result *r, char *buf, size_t cap)
{
  if(!r || !buf || cap == 0)
    return fail(SSD_E_ARG, "ssd_serialize: bad argument");
  if(r->status & SSD_ST_THROW)
  {
    buf[0] = 0;
    return 0;
  }
  std::string s;
  s.reserve(128 + 160 * static_cast<size_t>(r->n_steps > 0 ? r->n_steps : 0));
  /* fixed notation, 3 decimals, as `os << fixed << setprecision(3)` prints in the classic locale: std::to_chars is
   * locale-independent (a host that called setlocale(LC_NUMERIC, "de_DE") must not get "0,170") and writes every
   * digit of any magnitude (DBL_MAX has 309 integral digits) */
  char tmp[384];
  auto num = [&](double v)
  {
    const std::to_chars_result r = std::to_chars(tmp, tmp + sizeof(tmp), v, std::chars_format::fixed, 3);
    s.append(tmp, r.ptr);
  };
  s += "[\"stairs\",[\"stairSteps\",";
  s += std::to_string(r->n_steps);
  s += ']';
  if(r->n_steps > 0)
  {
    s += ",[";
    for(int i = 0; i < r->n_steps; i++)
    {
      const ssd_step &st = r->steps[i];
      if(i) s += ',';
      s += "[[\"height\",";
      num(st.height);
      s += "],[\"quadrilateral\",";
      for(int k = 0; k < 4; k++)
      {
        if(k) s += ',';
        s += '[';
        num(st.quad[2 * k]);
        s += ',';
        num(st.quad[2 * k + 1]);
        s += ']';
      }
      s += "]]";
    }
    s += ']';
  }
  s += ']';
  if(s.size() + 1 > cap)
    return fail(SSD_E_CAP, "ssd_serialize: buffer too small");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return static_cast<int>(s.size());
}
