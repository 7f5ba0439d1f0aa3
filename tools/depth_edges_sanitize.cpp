/*
 * tools/depth_edges_sanitize.cpp - the depth edge filter's host statement (ssd_depth_edge_default_rule, ssd_depth_edges_host; DESIGN.md
 * section 7t) once through a stand-alone program, for a build of the library's HOST code under AddressSanitizer and UBSan on a machine
 * without a GPU (tools/depth_edges_sanitize.sh builds and runs it).  No device is touched: the functions need no handle.  Small frames
 * stated by hand, one per edge of the rule, each in buffers exactly as large as the call may touch (so a byte too far - a neighbour
 * outside the frame read all the same - is seen); a 1 x 1 frame; and the refusals.  Exit status 0 when everything is as expected.
 */
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

/* one frame of up to 9 pixels, the rule, and what comes out of it: the outputs and the classes, pixel by pixel */
struct Case
{
  const char *name;
  int w, h;
  uint16_t d[9];
  ssd_depth_edge_rule rule;
  uint16_t out[9];
  uint8_t cls[9];
};

static const Case kCases[] = {
  { "flat 3 x 3, min_support 4: the corners go", 3, 3, { 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000 }, { 4, 0, 40, 0 },
    { 0, 1000, 0, 1000, 1000, 1000, 0, 1000, 0 }, { 2, 0, 2, 0, 0, 0, 2, 0, 2 } },
  { "flat 3 x 3, min_support 6: only the centre stays", 3, 3, { 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000 }, { 6, 0, 40, 0 },
    { 0, 0, 0, 0, 1000, 0, 0, 0, 0 }, { 2, 2, 2, 2, 0, 2, 2, 2, 2 } },
  { "a neighbour at exactly t", 2, 1, { 1000, 1040 }, { 1, 0, 40, 0 }, { 1000, 1040 }, { 0, 0 } },
  { "a neighbour at t + 1", 2, 1, { 1000, 1041 }, { 1, 0, 40, 0 }, { 0, 0 }, { 2, 2 } },
  { "3 beside 65500", 2, 1, { 3, 65500 }, { 1, 0, 40, 0 }, { 0, 0 }, { 2, 2 } },
  { "t saturates at 65535", 3, 1, { 65535, 1, 65535 }, { 1, 1, 40, 4096 }, { 65535, 0, 65535 }, { 0, 2, 0 } },
  { "a bridge at exactly t is none", 3, 1, { 960, 1000, 1041 }, { 0, 1, 40, 0 }, { 960, 1000, 1041 }, { 0, 0, 0 } },
  { "a bridge at t + 1, W/E", 3, 1, { 959, 1000, 1041 }, { 0, 1, 40, 0 }, { 959, 0, 1041 }, { 0, 3, 0 } },
  { "a bridge at t + 1, N/S, flipped", 1, 3, { 1041, 1000, 959 }, { 0, 1, 40, 0 }, { 1041, 0, 959 }, { 0, 3, 0 } },
  { "a bridge at t + 1, NW/SE", 3, 3, { 959, 0, 0, 0, 1000, 0, 0, 0, 1041 }, { 0, 1, 40, 0 }, { 959, 0, 0, 0, 0, 0, 0, 0, 1041 },
    { 0, 1, 1, 1, 3, 1, 1, 1, 0 } },
  { "a bridge at t + 1, NE/SW", 3, 3, { 0, 0, 959, 0, 1000, 0, 1041, 0, 0 }, { 0, 1, 40, 0 }, { 0, 0, 959, 0, 0, 0, 1041, 0, 0 },
    { 1, 1, 0, 1, 3, 1, 0, 1, 1 } },
  { "a pair with one pixel outside the frame", 2, 1, { 1000, 1100 }, { 0, 1, 40, 0 }, { 1000, 1100 }, { 0, 0 } },
  { "a pair with one pixel invalid", 3, 1, { 0, 1000, 1100 }, { 0, 1, 40, 0 }, { 0, 1000, 1100 }, { 1, 0, 0 } },
  { "lone and bridged: LONE", 3, 1, { 900, 1000, 1100 }, { 1, 1, 40, 0 }, { 0, 0, 0 }, { 2, 2, 2 } },
  { "bridge switched off", 3, 1, { 900, 1000, 1100 }, { 0, 0, 40, 0 }, { 900, 1000, 1100 }, { 0, 0, 0 } },
  { "1 x 1 valid", 1, 1, { 1234 }, { 0, 1, 40, 32 }, { 1234 }, { 0 } },
  { "1 x 1 valid, lone", 1, 1, { 1234 }, { 2, 1, 40, 0 }, { 0 }, { 2 } },
  { "1 x 1 empty", 1, 1, { 0 }, { 2, 1, 40, 0 }, { 0 }, { 1 } },
};

int main()
{
  ssd_depth_edge_rule rule;
  EXPECT(ssd_depth_edge_default_rule(&rule) == SSD_OK);
  EXPECT(rule.min_support == 2 && rule.bridge == 1 && rule.tol == SSD_FUSE_TOL && rule.slope == SSD_EDGE_SLOPE);
  EXPECT(ssd_depth_edge_default_rule(nullptr) == SSD_E_ARG);
  for(const Case &c : kCases)
  {
    const size_t n = static_cast<size_t>(c.w) * c.h;
    std::vector<uint16_t> frame(c.d, c.d + n), out(n, 7);             /* exactly the frame: the heap's red zones lie right behind */
    std::vector<uint8_t> cls(n, 7);
    ssd_depth_edge_stats st, st2;
    EXPECT(ssd_depth_edges_host(c.w, c.h, frame.data(), &c.rule, out.data(), cls.data(), &st) == SSD_OK);
    bool ok = true;
    long long count[4] = { 0, 0, 0, 0 };
    for(size_t p = 0; p < n; p++)
    {
      ok = ok && out[p] == c.out[p] && cls[p] == c.cls[p];
      count[c.cls[p]]++;
    }
    if(!ok)
      std::printf("case '%s' differs\n", c.name);
    EXPECT(ok);
    EXPECT(st.n_kept == count[0] && st.n_empty == count[1] && st.n_lone == count[2] && st.n_bridge == count[3]);
    EXPECT(st.reserved[0] == 0 && st.reserved[1] == 0 && st.reserved[2] == 0 && st.sum_support >= 0 && st.sum_support <= 8 * st.n_kept);
    std::vector<uint16_t> out2(n, 7);
    EXPECT(ssd_depth_edges_host(c.w, c.h, frame.data(), &c.rule, out2.data(), nullptr, &st2) == SSD_OK);
    EXPECT(out2 == out && std::memcmp(&st, &st2, sizeof(st)) == 0);
  }
  std::printf("%d hand-made frames\n", static_cast<int>(sizeof(kCases) / sizeof(kCases[0])));
  /* a frame with every kind of pixel at the sizes a row walk could trip over: 1 x N, N x 1, and 7 x 5 under the defaults */
  for(int shape = 0; shape < 3; shape++)
  {
    const int w = shape == 0 ? 37 : shape == 1 ? 1 : 7, h = shape == 0 ? 1 : shape == 1 ? 37 : 5;
    const size_t n = static_cast<size_t>(w) * h;
    std::vector<uint16_t> frame(n), out(n);
    std::vector<uint8_t> cls(n);
    const uint16_t kinds[] = { 1000, 1010, 0, 65535, 1500, 1020, 2000, 1, 1030 };
    for(size_t p = 0; p < n; p++)
      frame[p] = kinds[(p * 7 + p / 5) % 9];
    ssd_depth_edge_stats st;
    EXPECT(ssd_depth_edges_host(w, h, frame.data(), nullptr, out.data(), cls.data(), &st) == SSD_OK);
    EXPECT(st.n_kept + st.n_empty + st.n_lone + st.n_bridge == static_cast<long long>(n));
    for(size_t p = 0; p < n; p++)
      EXPECT((out[p] == 0 || out[p] == frame[p]) && (cls[p] == SSD_EDGE_KEPT) == (out[p] != 0) && cls[p] <= SSD_EDGE_BRIDGE);
  }
  /* the refusals */
  {
    std::vector<uint16_t> f(6, 100), o(6);
    ssd_depth_edge_stats st;
    const ssd_depth_edge_rule bad[] = { { -1, 1, 40, 0 }, { 9, 1, 40, 0 }, { 2, 1, -1, 0 }, { 2, 1, 65536, 0 }, { 2, 1, 40, -1 }, { 2, 1, 40, 4097 } };
    for(const ssd_depth_edge_rule &b : bad)
      EXPECT(ssd_depth_edges_host(3, 2, f.data(), &b, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_edges_host(3, 2, nullptr, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_edges_host(3, 2, f.data(), nullptr, nullptr, nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_edges_host(3, 2, f.data(), nullptr, o.data(), nullptr, nullptr) == SSD_E_ARG);
    EXPECT(ssd_depth_edges_host(0, 2, f.data(), nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_edges_host(3, 0, f.data(), nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_edges_host(-3, 2, f.data(), nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    const ssd_depth_edge_rule widest = { 8, 1, 65535, 4096 };
    EXPECT(ssd_depth_edges_host(3, 2, f.data(), &widest, o.data(), nullptr, &st) == SSD_OK && st.n_lone == 6);
    EXPECT(ssd_depth_edges_host(3, 2, f.data(), nullptr, o.data(), nullptr, &st) == SSD_OK && st.n_kept == 6 && st.sum_support == 22);
  }
  std::printf("depth edge filter host functions: %s\n", failures ? "FAILED" : "clean");
  return failures ? 1 : 0;
}
