/*
 * tools/depth_fill_sanitize.cpp - the depth fill's host statement (ssd_depth_fill_default_rule, ssd_depth_fill_host; DESIGN.md section
 * 7w) once through a stand-alone program, for a build of the library's HOST code under AddressSanitizer and UBSan on a machine without
 * a GPU (tools/host_sanitize.sh depth_fill builds and runs it).  No device is touched: the functions need no handle.  Small frames
 * stated by hand, one per edge of the rule, each in buffers exactly as large as the call may touch (so a byte too far - a neighbour
 * outside the frame read all the same - is seen); frames of one row, one column and one pixel; and the refusals.  Exit status 0 when
 * everything is as expected.
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

/* one frame of up to 9 pixels, the rule, and what comes out of it: the outputs and the classes, pixel by pixel, and the record's sums */
struct Case
{
  const char *name;
  int w, h;
  uint16_t d[9];
  ssd_depth_fill_rule rule;
  uint16_t out[9];
  uint8_t cls[9];
  long long pairs, spread;
};

static const Case kCases[] = {
  { "W/E at exactly t", 3, 1, { 1000, 0, 1040 }, { 1, 1, 40, 0 }, { 1000, 1020, 1040 }, { 0, 2, 0 }, 1, 40 },
  { "W/E at t + 1", 3, 1, { 1000, 0, 1041 }, { 1, 1, 40, 0 }, { 1000, 0, 1041 }, { 0, 1, 0 }, 0, 0 },
  { "N/S, m rounds up", 1, 3, { 1001, 0, 1000 }, { 1, 1, 40, 0 }, { 1001, 1001, 1000 }, { 0, 2, 0 }, 1, 1 },
  { "NW/SE", 3, 3, { 500, 0, 0, 0, 0, 0, 0, 0, 520 }, { 1, 1, 40, 0 }, { 500, 0, 0, 0, 510, 0, 0, 0, 520 }, { 0, 1, 1, 1, 2, 1, 1, 1, 0 }, 1, 20 },
  { "NE/SW", 3, 3, { 0, 0, 500, 0, 0, 0, 520, 0, 0 }, { 1, 1, 40, 0 }, { 0, 0, 500, 0, 510, 0, 520, 0, 0 }, { 1, 1, 0, 1, 2, 1, 0, 1, 1 }, 1, 20 },
  { "a tie: the first pair in the rule's order", 3, 3, { 0, 2000, 0, 1000, 0, 1010, 0, 2010, 0 }, { 1, 1, 40, 0 },
    { 0, 2000, 0, 1000, 1005, 1010, 0, 2010, 0 }, { 1, 0, 1, 0, 2, 0, 1, 0, 1 }, 2, 10 },
  { "the tighter pair, though later", 3, 3, { 0, 2000, 0, 1000, 0, 1010, 0, 2009, 0 }, { 1, 1, 40, 0 },
    { 0, 2000, 0, 1000, 2005, 1010, 0, 2009, 0 }, { 1, 0, 1, 0, 2, 0, 1, 0, 1 }, 2, 9 },
  { "min_pairs 2 missed by one", 3, 3, { 0, 2000, 0, 1000, 0, 1010, 0, 2041, 0 }, { 2, 1, 40, 0 },
    { 0, 2000, 0, 1000, 0, 1010, 0, 2041, 0 }, { 1, 0, 1, 0, 1, 0, 1, 0, 1 }, 0, 0 },
  { "65535 beside 65535", 3, 1, { 65535, 0, 65535 }, { 1, 1, 0, 0 }, { 65535, 65535, 65535 }, { 0, 2, 0 }, 1, 0 },
  { "t saturates at 65535", 3, 1, { 1, 0, 65535 }, { 1, 1, 65535, 4096 }, { 1, 32768, 65535 }, { 0, 2, 0 }, 1, 65534 },
  { "covered at hi + t + 1", 3, 1, { 1000, 1051, 1010 }, { 1, 1, 40, 0 }, { 1000, 1005, 1010 }, { 0, 3, 0 }, 1, 10 },
  { "not covered at hi + t", 3, 1, { 1000, 1050, 1010 }, { 1, 1, 40, 0 }, { 1000, 1050, 1010 }, { 0, 0, 0 }, 0, 0 },
  { "cover 0 keeps it", 3, 1, { 1000, 5000, 1010 }, { 1, 0, 40, 0 }, { 1000, 5000, 1010 }, { 0, 0, 0 }, 0, 0 },
  { "cover 2 missed by one", 3, 1, { 1000, 5000, 1010 }, { 1, 2, 40, 0 }, { 1000, 5000, 1010 }, { 0, 0, 0 }, 0, 0 },
  { "a pair end outside the frame", 2, 1, { 1000, 0 }, { 1, 1, 40, 0 }, { 1000, 0 }, { 0, 1 }, 0, 0 },
  { "1 x 1 valid", 1, 1, { 1234 }, { 1, 1, 40, 32 }, { 1234 }, { 0 }, 0, 0 },
  { "1 x 1 empty", 1, 1, { 0 }, { 1, 1, 40, 0 }, { 0 }, { 1 }, 0, 0 },
};

int main()
{
  ssd_depth_fill_rule rule;
  EXPECT(ssd_depth_fill_default_rule(&rule) == SSD_OK);
  EXPECT(rule.min_pairs == 1 && rule.cover == 1 && rule.tol == SSD_FUSE_TOL && rule.slope == 0);
  EXPECT(ssd_depth_fill_default_rule(nullptr) == SSD_E_ARG);
  for(const Case &c : kCases)
  {
    const size_t n = static_cast<size_t>(c.w) * c.h;
    std::vector<uint16_t> frame(c.d, c.d + n), out(n, 7);             /* exactly the frame: the heap's red zones lie right behind */
    std::vector<uint8_t> cls(n, 7);
    ssd_depth_fill_stats st, st2;
    EXPECT(ssd_depth_fill_host(c.w, c.h, frame.data(), &c.rule, out.data(), cls.data(), &st) == SSD_OK);
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
    EXPECT(st.n_kept == count[0] && st.n_empty == count[1] && st.n_filled == count[2] && st.n_covered == count[3]);
    EXPECT(st.reserved[0] == 0 && st.reserved[1] == 0 && st.sum_pairs == c.pairs && st.sum_spread == c.spread);
    std::vector<uint16_t> out2(n, 7);
    EXPECT(ssd_depth_fill_host(c.w, c.h, frame.data(), &c.rule, out2.data(), nullptr, &st2) == SSD_OK);
    EXPECT(out2 == out && std::memcmp(&st, &st2, sizeof(st)) == 0);
  }
  std::printf("%d hand-made frames\n", static_cast<int>(sizeof(kCases) / sizeof(kCases[0])));
  /* a frame with every kind of pixel at the sizes a row walk could trip over: 1 x N, N x 1, and 7 x 5, under the defaults and under
   * the widest rule: whatever is written lies between two samples of the input, whatever is kept is the input */
  for(int shape = 0; shape < 6; shape++)
  {
    const int w = shape % 3 == 0 ? 37 : shape % 3 == 1 ? 1 : 7, h = shape % 3 == 0 ? 1 : shape % 3 == 1 ? 37 : 5;
    const size_t n = static_cast<size_t>(w) * h;
    std::vector<uint16_t> frame(n), out(n);
    std::vector<uint8_t> cls(n);
    const uint16_t kinds[] = { 1000, 1010, 0, 65535, 1500, 1020, 0, 1, 1030 };
    for(size_t p = 0; p < n; p++)
      frame[p] = kinds[(p * 7 + p / 5) % 9];
    const ssd_depth_fill_rule widest = { 1, 1, 65535, 4096 };
    ssd_depth_fill_stats st;
    EXPECT(ssd_depth_fill_host(w, h, frame.data(), shape < 3 ? nullptr : &widest, out.data(), cls.data(), &st) == SSD_OK);
    EXPECT(st.n_kept + st.n_empty + st.n_filled + st.n_covered == static_cast<long long>(n));
    EXPECT(st.sum_pairs >= st.n_filled + st.n_covered && st.sum_pairs <= 4 * (st.n_filled + st.n_covered));
    for(size_t p = 0; p < n; p++)
    {
      EXPECT(cls[p] <= SSD_FILL_COVERED);
      EXPECT(cls[p] != SSD_FILL_KEPT || (out[p] == frame[p] && frame[p] != 0));
      EXPECT(cls[p] != SSD_FILL_EMPTY || (out[p] == 0 && frame[p] == 0));
      EXPECT(cls[p] != SSD_FILL_FILLED || (out[p] != 0 && frame[p] == 0));
      EXPECT(cls[p] != SSD_FILL_COVERED || (out[p] != 0 && out[p] < frame[p]));
    }
  }
  /* the refusals */
  {
    std::vector<uint16_t> f(6, 100), o(6);
    ssd_depth_fill_stats st;
    const ssd_depth_fill_rule bad[] = { { 0, 1, 40, 0 }, { 5, 1, 40, 0 }, { 1, -1, 40, 0 }, { 1, 5, 40, 0 }, { 1, 1, -1, 0 }, { 1, 1, 65536, 0 },
                                        { 1, 1, 40, -1 }, { 1, 1, 40, 4097 } };
    for(const ssd_depth_fill_rule &b : bad)
      EXPECT(ssd_depth_fill_host(3, 2, f.data(), &b, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fill_host(3, 2, nullptr, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fill_host(3, 2, f.data(), nullptr, nullptr, nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fill_host(3, 2, f.data(), nullptr, o.data(), nullptr, nullptr) == SSD_E_ARG);
    EXPECT(ssd_depth_fill_host(0, 2, f.data(), nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fill_host(3, 0, f.data(), nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fill_host(-3, 2, f.data(), nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    const ssd_depth_fill_rule widest = { 4, 4, 65535, 4096 };
    EXPECT(ssd_depth_fill_host(3, 2, f.data(), &widest, o.data(), nullptr, &st) == SSD_OK && st.n_kept == 6);
    EXPECT(ssd_depth_fill_host(3, 2, f.data(), nullptr, o.data(), nullptr, &st) == SSD_OK && st.n_kept == 6 && st.sum_pairs == 0);
  }
  std::printf("depth fill host functions: %s\n", failures ? "FAILED" : "clean");
  return failures ? 1 : 0;
}
