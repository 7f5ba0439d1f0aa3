/*
 * tools/stair_pose_sanitize.cpp - the stair pose's host rule, fold and solve (ssd_stair_pose_host, ssd_stair_pose_add,
 * ssd_stair_pose_solve) once through a stand-alone program, for a build of the library's HOST code under
 * AddressSanitizer and UBSan on a machine without a GPU (tools/stair_pose_sanitize.sh builds and runs it).  No device is touched: the
 * three functions need no handle.  A 3-step staircase on exact planes seen by a camera 1 m up and pitched 50 degrees, as vertices and as
 * 16-bit depth; a prior moved by 2 cm; every map the rule treats specially; the fold up to the edge of int64.  Exit status 0 and one
 * line per step when everything is as expected.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/ssd_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do                                                                                  \
  {                                                                                   \
    if(!(cond))                                                                       \
    {                                                                                 \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                           \
      failures++;                                                                     \
    }                                                                                 \
  } while(0)

int main()
{
  const int W = 96, H = 72;
  ssd_config cfg;
  EXPECT(ssd_default_config(&cfg, W, H) == SSD_OK);
  /* the camera: 1 m above the floor, pitched 50 degrees down; the external world is the camera-dependent one */
  const double pitch = 50.0 * M_PI / 180.0, n0[3] = { 0.0, std::sin(pitch), std::cos(pitch) };
  ssd_calibration ident, truth;
  EXPECT(ssd_calibration_identity(&ident) == SSD_OK);
  EXPECT(ssd_calibration_from_plane(n0, 1.0, &ident, &truth) == SSD_OK);
  /* the staircase: treads 0.3 m deep over x -0.4 .. 0.4 from y = 0.2 on, rising 0.16 m each */
  ssd_stair_pose_target target;
  std::memset(&target, 0, sizeof(target));
  target.prior.cal = truth;
  target.prior.intr = ssd_intrinsics{ 60.0f, 60.0f, (W - 1) / 2.0f, (H - 1) / 2.0f, 0.00025f };
  target.prior.has_intrinsics = 1;
  target.map.ground = 1;
  target.map.stairs.n_steps = 3;
  for(int k = 0; k < 3; k++)
  {
    ssd_step &s = target.map.stairs.steps[k];
    const double y0 = 0.2 + 0.3 * k, q[8] = { -0.4, y0, 0.4, y0, -0.4, y0 + 0.3, 0.4, y0 + 0.3 };
    s.height = 0.16 * k;
    std::memcpy(s.quad, q, sizeof(q));
  }
  /* the frame: every pixel a point of the staircase, pixel (u, v) at the world's x = -0.38 + 0.76 u / (W - 1) and the v-th of H stations
   * up the profile (tread, face, tread, face, tread); camera p = A^T (w - b) */
  std::vector<float> xyz(3 * static_cast<size_t>(W) * H, 0.0f);
  for(int v = 0; v < H; v++)
    for(int u = 0; u < W; u++)
    {
      const double s = (v + 0.5) / H * 5.0;
      const int part = static_cast<int>(s);
      const double f = s - part, wx = -0.38 + 0.76 * u / (W - 1);
      double wy, wz;
      if(part % 2 == 0)
      {
        wy = 0.2 + 0.3 * (part / 2) + 0.04 + 0.22 * f;
        wz = 0.16 * (part / 2);
      }
      else
      {
        wy = 0.2 + 0.3 * ((part + 1) / 2);
        wz = 0.16 * (part / 2) + 0.05 + 0.06 * f;
      }
      const double w[3] = { wx - truth.b[0], wy - truth.b[1], wz - truth.b[2] };
      float *p = &xyz[3 * (static_cast<size_t>(v) * W + u)];
      for(int j = 0; j < 3; j++)
        p[j] = static_cast<float>(truth.a[j] * w[0] + truth.a[3 + j] * w[1] + truth.a[6 + j] * w[2]);
    }
  ssd_stair_pose_rule rule{ SSD_SP_MARGIN, SSD_SP_BAND, SSD_SP_CLEAR, SSD_SP_REACH };
  ssd_stair_pose_moments rec, acc;
  EXPECT(ssd_stair_pose_host(&cfg, &target, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_OK);
  EXPECT(rec.treads.n_surfaces == 3 && rec.risers.n_surfaces == 2 && rec.treads.ground == 1);
  for(int k = 0; k < 3; k++)
    EXPECT(rec.treads.s[k].m.n > 500);
  for(int i = 0; i < 2; i++)
    EXPECT(rec.risers.s[i].m.n > 500);
  std::printf("host, vertices: treads %lld %lld %lld, risers %lld %lld\n", (long long)rec.treads.s[0].m.n, (long long)rec.treads.s[1].m.n,
              (long long)rec.treads.s[2].m.n, (long long)rec.risers.s[0].m.n, (long long)rec.risers.s[1].m.n);
  /* the fold: three frames, then the edge of int64 */
  std::memset(&acc, 0, sizeof(acc));
  for(int i = 0; i < 3; i++)
    EXPECT(ssd_stair_pose_add(&rec, &acc) == SSD_OK);
  EXPECT(acc.treads.s[1].m.n == 3 * rec.treads.s[1].m.n && acc.risers.s[1].m.ss[5] == 3 * rec.risers.s[1].m.ss[5]);
  ssd_stair_pose_moments full = acc, kept;
  full.risers.s[15].n_far = INT64_MAX;
  kept = full;
  ssd_stair_pose_moments one;
  std::memset(&one, 0, sizeof(one));
  one.risers.s[15].n_far = 1;
  EXPECT(ssd_stair_pose_add(&one, &full) == SSD_E_CAP && std::memcmp(&full, &kept, sizeof(full)) == 0);
  EXPECT(ssd_stair_pose_add(nullptr, &full) == SSD_E_ARG && ssd_stair_pose_add(&one, nullptr) == SSD_E_ARG);
  /* the solve: from the truth, and from a prior 2 cm off along the going and 1.5 cm in height (one pass recovers a translation) */
  ssd_stair_pose pose;
  EXPECT(ssd_stair_pose_solve(&acc, &target, 200, SSD_SP_OBSERVABLE, &pose) == SSD_OK);
  EXPECT(pose.status == SSD_GF_OK && pose.dof == 5 && pose.treads_used == 7u && pose.risers_used == 3u && pose.rms_before < 1e-4);
  std::printf("solve from the truth: status %d, dof %d, rms %.3e -> %.3e m\n", pose.status, pose.dof, pose.rms_before, pose.rms_after);
  ssd_stair_pose_target moved = target;
  moved.prior.cal.t2[1] += 0.02;
  moved.prior.cal.world_z += 0.015;
  EXPECT(ssd_stair_pose_host(&cfg, &moved, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_OK);
  EXPECT(ssd_stair_pose_solve(&rec, &moved, 200, SSD_SP_OBSERVABLE, &pose) == SSD_OK);
  EXPECT(pose.status == SSD_GF_OK && pose.dof == 5);
  EXPECT(std::fabs(pose.translation[1] + 0.02) < 1e-4 && std::fabs(pose.translation[2] + 0.015) < 1e-4 && pose.rms_after < 1e-4);
  std::printf("solve from a moved prior: translation %.6f %.6f %.6f, rms %.3e -> %.3e m\n", pose.translation[0], pose.translation[1],
              pose.translation[2], pose.rms_before, pose.rms_after);
  EXPECT(ssd_stair_pose_solve(&rec, &moved, 1 << 30, SSD_SP_OBSERVABLE, &pose) == SSD_OK && pose.status == SSD_GF_FEW);
  EXPECT(std::memcmp(&pose.cal, &moved.prior.cal, sizeof(ssd_calibration)) == 0);
  /* 16-bit depth: the same frame's z through the intrinsics (the points move, the classes are still all seen) */
  std::vector<uint16_t> depth(static_cast<size_t>(W) * H);
  for(size_t i = 0; i < depth.size(); i++)
    depth[i] = static_cast<uint16_t>(std::lrint(xyz[3 * i + 2] / 0.00025f));
  depth[0] = 0;
  depth[1] = 65535;
  EXPECT(ssd_stair_pose_host(&cfg, &target, SSD_INPUT_DEPTH16, depth.data(), &rule, &rec) == SSD_OK);
  std::printf("host, depth: treads %lld %lld %lld, risers %lld %lld\n", (long long)rec.treads.s[0].m.n, (long long)rec.treads.s[1].m.n,
              (long long)rec.treads.s[2].m.n, (long long)rec.risers.s[0].m.n, (long long)rec.risers.s[1].m.n);
  EXPECT(ssd_stair_pose_solve(&rec, &target, 1, SSD_SP_OBSERVABLE, &pose) == SSD_OK);
  /* the maps the rule treats specially: thrown, empty, one step, the full 17, a NaN corner, and the refusals */
  ssd_stair_pose_target odd = target;
  odd.map.stairs.status = SSD_ST_THROW;
  EXPECT(ssd_stair_pose_host(&cfg, &odd, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_OK && rec.treads.n_surfaces == 0 && rec.treads.s[0].m.n == 0);
  EXPECT(ssd_stair_pose_solve(&rec, &odd, 1, SSD_SP_OBSERVABLE, &pose) == SSD_OK && pose.status == SSD_GF_FEW);
  odd = target;
  odd.map.stairs.n_steps = 0;
  EXPECT(ssd_stair_pose_host(&cfg, &odd, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_OK && rec.treads.n_surfaces == 0);
  odd.map.stairs.n_steps = 1;
  EXPECT(ssd_stair_pose_host(&cfg, &odd, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_OK && rec.risers.n_surfaces == 0 && rec.treads.s[0].m.n > 500);
  EXPECT(ssd_stair_pose_solve(&rec, &odd, 200, SSD_SP_OBSERVABLE, &pose) == SSD_OK && pose.status == SSD_GF_OK && pose.dof == 3);
  odd.map.stairs.n_steps = SSD_MAX_STEPS;
  for(int k = 3; k < SSD_MAX_STEPS; k++)
  {
    odd.map.stairs.steps[k] = odd.map.stairs.steps[2];
    odd.map.stairs.steps[k].height = 0.16 * k;
  }
  EXPECT(ssd_stair_pose_host(&cfg, &odd, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_OK && rec.risers.n_surfaces == SSD_MAX_STEPS - 1);
  EXPECT(ssd_stair_pose_solve(&rec, &odd, 200, SSD_SP_OBSERVABLE, &pose) == SSD_OK);
  odd.map.stairs.steps[1].quad[0] = std::nan("");
  EXPECT(ssd_stair_pose_host(&cfg, &odd, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_OK && rec.risers.s[0].m.n == 0);
  EXPECT(ssd_stair_pose_solve(&rec, &odd, 1, SSD_SP_OBSERVABLE, &pose) == SSD_OK);
  odd.map.stairs.n_steps = SSD_MAX_STEPS + 1;
  EXPECT(ssd_stair_pose_host(&cfg, &odd, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_E_ARG);
  EXPECT(ssd_stair_pose_solve(&rec, &odd, 1, SSD_SP_OBSERVABLE, &pose) == SSD_E_ARG);
  rule.reach = std::nan("");
  EXPECT(ssd_stair_pose_host(&cfg, &target, SSD_INPUT_VERTICES, xyz.data(), &rule, &rec) == SSD_E_ARG);
  std::printf("stair pose host functions: %s\n", failures ? "FAILED" : "clean");
  return failures ? 1 : 0;
}
