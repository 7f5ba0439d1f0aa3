/*
 * tools/depth_warp_sanitize.cpp - the depth warp's host functions (ssd_depth_warp_host, ssd_depth_warp_view_between; DESIGN.md section
 * 7v) once through a stand-alone program, for a build of the library's HOST code under AddressSanitizer and UBSan on a machine without a
 * GPU (tools/host_sanitize.sh builds and runs it).  No device is touched: the functions need no handle.  Frames in buffers exactly as
 * large as the call may touch (so a sample scattered a pixel too far is seen), under views that send samples to every side of the frame,
 * behind the camera and out of the 16-bit range; 1 x 2 and 2 x 1 frames; the identity; the view between two cameras; and the refusals.
 * Exit status 0 when everything is as expected.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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

static ssd_depth_warp_view identity(const ssd_intrinsics &in)
{
  ssd_depth_warp_view v;
  std::memset(&v, 0, sizeof(v));
  v.r[0] = v.r[4] = v.r[8] = 1.0;
  v.src = in;
  return v;
}

/* the frame under the view in buffers of exactly w * h values; the counts must add up and n_filled must be the output's */
static ssd_depth_warp_stats run(int w, int h, const std::vector<uint16_t> &frame, const ssd_depth_warp_view &v, const ssd_intrinsics &dst,
                                std::vector<uint16_t> &out)
{
  const size_t n = static_cast<size_t>(w) * h;
  out.assign(n, 7);
  ssd_depth_warp_stats st;
  EXPECT(ssd_depth_warp_host(w, h, frame.data(), &v, &dst, out.data(), &st) == SSD_OK);
  EXPECT(st.n_empty + st.n_behind + st.n_range + st.n_outside + st.n_landed == static_cast<long long>(n));
  long long filled = 0;
  for(size_t p = 0; p < n; p++)
    filled += out[p] != 0;
  EXPECT(filled == st.n_filled && st.n_filled <= st.n_landed && st.reserved[0] == 0 && st.reserved[1] == 0);
  return st;
}

int main()
{
  EXPECT(sizeof(ssd_depth_warp_view) == 120 && sizeof(ssd_depth_warp_stats) == 64);
  const ssd_intrinsics in = { 20.0f, 18.0f, 6.0f, 4.0f, 0.00025f };
  const int w = 13, h = 9;
  const size_t n = static_cast<size_t>(w) * h;
  std::vector<uint16_t> frame(n), out;
  const uint16_t kinds[] = { 4000, 4010, 0, 65535, 6000, 1, 8000, 3990, 12000 };
  for(size_t p = 0; p < n; p++)
    frame[p] = kinds[(p * 7 + p / 5) % 9];
  /* the identity gives the frame back */
  ssd_depth_warp_view v = identity(in);
  ssd_depth_warp_stats st = run(w, h, frame, v, in, out);
  EXPECT(out == frame && st.n_landed == st.n_filled && st.n_behind == 0 && st.n_range == 0 && st.n_outside == 0);
  /* shifts that push samples over each side, rotations, a half turn (everything BEHIND), t[2] out of the range both ways */
  const double shifts[][3] = { { 5.0, 0, 0 }, { -5.0, 0, 0 }, { 0, 5.0, 0 }, { 0, -5.0, 0 }, { 0.3, -0.2, 0.5 }, { 0, 0, 20.0 }, { 0, 0, -0.9 }, { 0, 0, -1.0005 } };
  for(const double (&t)[3] : shifts)
  {
    v = identity(in);
    v.t[0] = t[0]; v.t[1] = t[1]; v.t[2] = t[2];
    st = run(w, h, frame, v, in, out);
  }
  v = identity(in);
  v.t[2] = 20.0;
  st = run(w, h, frame, v, in, out);
  EXPECT(st.n_range > 0);                                              /* 65535 * units + 20 m is beyond 16 bits */
  v = identity(in);
  v.r[0] = -1.0; v.r[8] = -1.0;                                        /* a half turn about y */
  st = run(w, h, frame, v, in, out);
  EXPECT(st.n_behind == static_cast<long long>(n) - st.n_empty && st.n_filled == 0);
  for(int k = 0; k < 6; k++)
  {
    const double a = 0.02 * (k + 1), c = std::cos(a), s = std::sin(a);
    v = identity(in);
    if(k % 3 == 0) { v.r[4] = c; v.r[5] = -s; v.r[7] = s; v.r[8] = c; }
    else if(k % 3 == 1) { v.r[0] = c; v.r[2] = s; v.r[6] = -s; v.r[8] = c; }
    else { v.r[0] = c; v.r[1] = -s; v.r[3] = s; v.r[4] = c; }
    v.t[0] = 0.01 * k; v.t[2] = -0.05 * k;
    st = run(w, h, frame, v, in, out);
  }
  /* everything onto one pixel: a target with no focal spread to speak of */
  {
    const ssd_intrinsics flat = { 1e-6f, 1e-6f, 3.0f, 2.0f, 0.00025f };
    v = identity(in);
    st = run(w, h, frame, v, flat, out);
    EXPECT(st.n_filled == 1 && out[2 * w + 3] == 1);
  }
  /* the smallest frames */
  for(int shape = 0; shape < 2; shape++)
  {
    const int sw = shape ? 2 : 1, sh = shape ? 1 : 2;
    const ssd_intrinsics small = { 2.0f, 2.0f, 0.0f, 0.0f, 0.001f };
    std::vector<uint16_t> f = { 1000, 65535 };
    v = identity(small);
    st = run(sw, sh, f, v, small, out);
    EXPECT(out == f);
    v.t[shape ? 0 : 1] = -200.0;
    st = run(sw, sh, f, v, small, out);
    EXPECT(st.n_outside == 2);
  }
  /* the view between two cameras: equal cameras give the identity, and the refusals */
  {
    ssd_camera a, b;
    std::memset(&a, 0, sizeof(a));
    const double c = std::cos(0.7), s = std::sin(0.7);
    const double rot[9] = { 1, 0, 0, 0, -s, c, 0, -c, -s };
    for(int i = 0; i < 9; i++) a.cal.a[i] = rot[i];
    a.cal.b[2] = 1.0;
    a.cal.r2[0] = a.cal.r2[3] = 1.0;
    a.cal.world_z = 0.004;
    a.intr = in;
    a.has_intrinsics = 1;
    b = a;
    ssd_depth_warp_view between;
    EXPECT(ssd_depth_warp_view_between(&a, &b, &between) == SSD_OK);
    const ssd_depth_warp_view id = identity(in);
    double worst = 0.0;
    for(int i = 0; i < 9; i++) worst = std::fmax(worst, std::fabs(between.r[i] - id.r[i]));
    for(int i = 0; i < 3; i++) worst = std::fmax(worst, std::fabs(between.t[i]));
    EXPECT(worst < 1e-12 && std::memcmp(&between.src, &in, sizeof(in)) == 0 && between.reserved[0] == 0);
    b.cal.b[2] = 1.02;
    b.has_intrinsics = 0;                                              /* dst needs none */
    EXPECT(ssd_depth_warp_view_between(&a, &b, &between) == SSD_OK);
    st = run(w, h, frame, between, in, out);
    EXPECT(ssd_depth_warp_view_between(nullptr, &b, &between) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_view_between(&a, nullptr, &between) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_view_between(&a, &b, nullptr) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_view_between(&b, &a, &between) == SSD_E_ARG);        /* src without intrinsics */
    ssd_camera bad = a;
    bad.cal.a[4] = std::numeric_limits<double>::quiet_NaN();
    EXPECT(ssd_depth_warp_view_between(&a, &bad, &between) == SSD_E_ARG && ssd_depth_warp_view_between(&bad, &a, &between) == SSD_E_ARG);
    bad = a;
    for(int i = 0; i < 9; i++) bad.cal.a[i] = 0.0;
    EXPECT(ssd_depth_warp_view_between(&a, &bad, &between) == SSD_E_ARG);      /* singular */
    bad = a;
    bad.intr.fx = 0.0f;
    EXPECT(ssd_depth_warp_view_between(&bad, &a, &between) == SSD_E_ARG);
  }
  /* the host statement's refusals */
  {
    std::vector<uint16_t> f(6, 100), o(6);
    v = identity(in);
    EXPECT(ssd_depth_warp_host(3, 2, nullptr, &v, &in, o.data(), &st) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), nullptr, &in, o.data(), &st) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &v, nullptr, o.data(), &st) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &v, &in, nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &v, &in, o.data(), nullptr) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(0, 2, f.data(), &v, &in, o.data(), &st) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(3, 0, f.data(), &v, &in, o.data(), &st) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(-3, 2, f.data(), &v, &in, o.data(), &st) == SSD_E_ARG);
    ssd_intrinsics badIn = in;
    badIn.depth_units = 0.0f;
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &v, &badIn, o.data(), &st) == SSD_E_ARG);
    ssd_depth_warp_view badV = v;
    badV.src.fy = 0.0f;
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &badV, &in, o.data(), &st) == SSD_E_ARG);
    badV = v;
    badV.t[1] = std::numeric_limits<double>::infinity();
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &badV, &in, o.data(), &st) == SSD_E_ARG);
    badV = v;
    badV.r[5] = std::numeric_limits<double>::quiet_NaN();
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &badV, &in, o.data(), &st) == SSD_E_ARG);
    EXPECT(ssd_depth_warp_host(3, 2, f.data(), &v, &in, o.data(), &st) == SSD_OK && st.n_landed == 6);
  }
  std::printf("depth warp host functions: %s\n", failures ? "FAILED" : "clean");
  return failures ? 1 : 0;
}
