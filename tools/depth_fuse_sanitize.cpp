/*
 * tools/depth_fuse_sanitize.cpp - the depth fusion's host statement (ssd_depth_fuse_default_rule, ssd_depth_fuse_host; DESIGN.md section
 * 7s) once through a stand-alone program, for a build of the library's HOST code under AddressSanitizer and UBSan on a machine without
 * a GPU (tools/depth_fuse_sanitize.sh builds and runs it).  No device is touched: the functions need no handle.  A frame built for the
 * rule's edges, one pixel per case, in buffers that are exactly as large as the call may touch (so a byte too far is seen), at a packed
 * and at a padded stride, for every n; and the refusals.  Exit status 0 and one line per step when everything is as expected.
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

/* one pixel's case: up to 5 samples (the rest invalid) and what the default rule for n = 5 (3, 3, 40) makes of it */
struct Case
{
  const char *name;
  uint16_t d[5];
  uint16_t out;
  uint8_t support;
};

static const Case kCases[] = {
  { "all invalid", { 0, 0, 0, 0, 0 }, 0, 0 },
  { "m == min_valid - 1", { 20000, 0, 20000, 0, 0 }, 0, 0 },
  { "m == min_valid", { 20000, 0, 20000, 20000, 0 }, 20000, 3 },
  { "c == min_agree - 1", { 20000, 30000, 20000, 30000, 0 }, 0, 0 },
  { "a sample at med + tol", { 30000, 30040, 30000, 0, 0 }, 30013, 3 },
  { "a sample at med + tol + 1", { 30000, 30041, 30000, 0, 0 }, 0, 0 },
  { "a sample at med - tol", { 30000, 29960, 30000, 0, 0 }, 29987, 3 },
  { "a sample at med - tol - 1", { 30000, 29959, 30000, 0, 0 }, 0, 0 },
  { "far above a small median", { 3, 65500, 3, 3, 0 }, 3, 3 },
  { "far below a large median", { 65534, 1, 65534, 65534, 0 }, 65534, 3 },
  { "even m: the lower median", { 1000, 1000, 2000, 2000, 0 }, 0, 0 },
  { "even m: the lower median's camp wins", { 1000, 1000, 1001, 2000, 0 }, 1000, 3 },
  { "a mean ending in one half, even c", { 1000, 1001, 1000, 1001, 0 }, 1001, 4 },
  { "a mean ending in one half, odd c", { 1000, 1000, 1003, 1003, 1004 }, 1002, 5 },
  { "valid samples of 1", { 1, 1, 1, 0, 0 }, 1, 3 },
  { "valid samples of 65535", { 65535, 65535, 65535, 65535, 65535 }, 65535, 5 },
  { "a median near 65535 beside invalid samples", { 65530, 0, 65535, 0, 65530 }, 65532, 3 },
};

int main()
{
  const int nCases = static_cast<int>(sizeof(kCases) / sizeof(kCases[0])), W = nCases, H = 3;
  const size_t nPoints = static_cast<size_t>(W) * H;
  ssd_depth_fuse_rule rule;
  for(int n = 1; n <= SSD_FUSE_MAX_FRAMES; n++)
  {
    EXPECT(ssd_depth_fuse_default_rule(n, &rule) == SSD_OK);
    EXPECT(rule.min_valid == (n + 1) / 2 && rule.min_agree == (n + 1) / 2 && rule.tol == SSD_FUSE_TOL && rule.reserved == 0);
  }
  EXPECT(ssd_depth_fuse_default_rule(0, &rule) == SSD_E_ARG && ssd_depth_fuse_default_rule(17, &rule) == SSD_E_ARG);
  EXPECT(ssd_depth_fuse_default_rule(5, nullptr) == SSD_E_ARG);
  /* the edge frame at n = 5: row 0 the cases, row 1 the cases with their samples reversed, row 2 all invalid */
  for(int padded = 0; padded < 2; padded++)
  {
    const size_t stride = nPoints * 2 + (padded ? 6 : 0);
    std::vector<unsigned char> frames(stride * 4 + nPoints * 2, 0);           /* exactly what five frames at that stride span */
    for(int j = 0; j < 5; j++)
      for(int p = 0; p < W; p++)
      {
        std::memcpy(&frames[stride * j + 2 * p], &kCases[p].d[j], 2);
        std::memcpy(&frames[stride * j + 2 * (W + p)], &kCases[p].d[4 - j], 2);
      }
    std::vector<uint16_t> out(nPoints, 7);
    std::vector<uint8_t> sup(nPoints, 7);
    ssd_depth_fuse_stats st;
    EXPECT(ssd_depth_fuse_host(W, H, reinterpret_cast<const uint16_t *>(frames.data()), stride, 5, nullptr, out.data(), sup.data(), &st) == SSD_OK);
    long long fused = 0;
    for(int p = 0; p < W; p++)
    {
      const bool ok = out[p] == kCases[p].out && sup[p] == kCases[p].support && out[W + p] == kCases[p].out && sup[W + p] == kCases[p].support;
      if(!ok)
        std::printf("case '%s': %u / %u (reversed %u / %u), expected %u / %u\n", kCases[p].name, out[p], sup[p], out[W + p], sup[W + p],
                    kCases[p].out, kCases[p].support);
      EXPECT(ok);
      fused += kCases[p].out != 0 ? 2 : 0;
      EXPECT(out[2 * W + p] == 0 && sup[2 * W + p] == 0);
    }
    EXPECT(st.n_fused == fused && st.n_fused + st.n_empty + st.n_few + st.n_split == static_cast<long long>(nPoints) && st.n_empty == W + 2);
    EXPECT(st.reserved == 0 && st.sum_agree >= 3 * st.n_fused);
    std::printf("n = 5, stride %zu: fused %lld, empty %lld, few %lld, split %lld, valid %lld, agree %lld, abs dev %lld\n", stride, (long long)st.n_fused,
                (long long)st.n_empty, (long long)st.n_few, (long long)st.n_split, (long long)st.sum_valid, (long long)st.sum_agree, (long long)st.sum_abs_dev);
    /* without the support map, and tol = 0 with one sample enough */
    ssd_depth_fuse_stats st2;
    std::vector<uint16_t> out2(nPoints, 7);
    EXPECT(ssd_depth_fuse_host(W, H, reinterpret_cast<const uint16_t *>(frames.data()), stride, 5, nullptr, out2.data(), nullptr, &st2) == SSD_OK);
    EXPECT(out2 == out && std::memcmp(&st, &st2, sizeof(st)) == 0);
    const ssd_depth_fuse_rule exact = { 1, 1, 0, 0 };
    EXPECT(ssd_depth_fuse_host(W, H, reinterpret_cast<const uint16_t *>(frames.data()), stride, 5, &exact, out2.data(), sup.data(), &st2) == SSD_OK);
    EXPECT(out2[4] == 30000 && sup[4] == 2 && out2[0] == 0 && st2.n_few == 0 && st2.n_split == 0 && st2.sum_abs_dev == 0);
    /* n = 1 .. 5 over the first n frames, in a buffer that ends with the n-th */
    for(int n = 1; n <= 5; n++)
    {
      std::vector<unsigned char> part(frames.begin(), frames.begin() + static_cast<long>(stride * (n - 1) + nPoints * 2));
      EXPECT(ssd_depth_fuse_host(W, H, reinterpret_cast<const uint16_t *>(part.data()), stride, n, nullptr, out2.data(), sup.data(), &st2) == SSD_OK);
      EXPECT(st2.n_fused + st2.n_empty + st2.n_few + st2.n_split == static_cast<long long>(nPoints));
    }
  }
  /* sixteen frames of one pixel each: the sums' upper end */
  {
    std::vector<uint16_t> col(16, 65535);
    uint16_t o = 0;
    uint8_t s = 0;
    ssd_depth_fuse_stats st;
    EXPECT(ssd_depth_fuse_host(1, 1, col.data(), 2, 16, nullptr, &o, &s, &st) == SSD_OK && o == 65535 && s == 16 && st.sum_agree == 16 && st.sum_abs_dev == 0);
    col[3] = 65495;
    EXPECT(ssd_depth_fuse_host(1, 1, col.data(), 2, 16, nullptr, &o, &s, &st) == SSD_OK && o == 65533 && s == 16 && st.sum_abs_dev == 15 * 2 + 38);
  }
  /* the refusals */
  {
    std::vector<uint16_t> f(2 * 6, 100), o(6);
    ssd_depth_fuse_stats st;
    const ssd_depth_fuse_rule bad[] = { { 0, 1, 40, 0 }, { 3, 1, 40, 0 }, { 1, 0, 40, 0 }, { 1, 3, 40, 0 }, { 1, 1, -1, 0 }, { 1, 1, 65536, 0 } };
    for(const ssd_depth_fuse_rule &b : bad)
      EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 12, 2, &b, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, nullptr, 12, 2, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 12, 2, nullptr, nullptr, nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 12, 2, nullptr, o.data(), nullptr, nullptr) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(0, 2, f.data(), 12, 2, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 0, f.data(), 12, 2, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 12, 0, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 12, 17, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 10, 2, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 13, 2, nullptr, o.data(), nullptr, &st) == SSD_E_ARG);
    EXPECT(ssd_depth_fuse_host(3, 2, f.data(), 12, 2, nullptr, o.data(), nullptr, &st) == SSD_OK && st.n_fused == 6);
  }
  std::printf("depth fusion host functions: %s\n", failures ? "FAILED" : "clean");
  return failures ? 1 : 0;
}
