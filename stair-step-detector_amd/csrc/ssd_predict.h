/*
 * ssd_predict.h — the table the single pass's predictor makes of its sample histogram (k_predict's last step), stated as a
 * plain function for host and device.  k_predict computes the same table with one thread per bin (ballots and rank counting);
 * the test hook ssd_test_predict_table_host runs THIS statement, tests/test_predict.py checks its properties on the CPU and
 * tests/test_gpu_single_pass.py that the kernel's table equals it on every frame of a batch.
 *
 * sample[b]: points of height bin b among the sampled points: the points that lie wholly inside one 128-byte line of memory out of
 *            every kPredictGroupLines consecutive lines of the frame (predict_sample_run below: ten points of every 160, one in
 *            kSpecSample).
 * plane[b]:  the plane (bit image) K1 rasters bin b's points into, 0xff = none.  Returns the number of planes.
 *
 * Rules ("The single pass"):
 *  - candidate peak: minHeight <= b < nBins - 1 (a step plateau's peak, pointcloud.cpp:402-418), a local maximum of the
 *    sample (c > left, c >= right), >= 1200 points scaled up, the neighbours' sum below 1.5 c plus 8 samples (filterPeaks,
 *    pointcloud.cpp:243-256, on the sample);
 *  - at most kMaxPlanes / 3 candidates: the fullest (ties: the lower bin);
 *  - a chosen peak gets a plane for its bin, and for each neighbour unless the OTHER neighbour is more than twice as full (+ 8):
 *    the plateau is the peak's bin and the fuller neighbour (extractPlateauPoints, pointcloud.cpp:300-335);
 *  - the peak and a neighbour beyond doubt share ONE plane; otherwise every bin has its own;
 *  - more planes than kMaxPlanes: none at all (cannot happen with eight candidates of three bins; kept as a guard).
 * sabotage (tests): 1 = the table three bins above where it belongs, 2 = no planes.
 */
#ifndef SSD_PREDICT_H_
#define SSD_PREDICT_H_

#include "ssd_device.h"

namespace ssd
{

/* ---- the sample ----
 * k_predict reads whole 128-byte lines - what the memory system fetches anyway - and counts the points that lie wholly inside them.
 * Lines are counted on absolute byte addresses (a frame is only 4-byte aligned: a caller's odd base still gives whole lines); a
 * window of 128 bytes that starts a multiple of 4 bytes into a point holds ten whole 12-byte points, and a group of
 * kPredictGroupLines = 15 lines is 160 points: ten in 160 is one in kSpecSample = 16, so every threshold below stays as it is.
 * Group g of a frame is the lines 15 g .. 15 g + 14 counted from the line the frame's first byte lies in; the group's sampled line is
 * at predict_sample_offset(g) in it: floor(15 frac(g c)) with c = (golden ratio - 1) / 56.  The place creeps through the group by a
 * sixth of a line from one group to the next: sampled lines follow each other 15 lines apart, every sixth time 16 (and once in 90
 * groups one, where the place wraps) - an even spacing along the scan whose place in the camera's rows keeps moving.  A fixed place, or
 * one of a short period, samples some columns in every row and others never (an XGA row is 96 lines, 96 mod 15 = 6; a VGA row is 60).
 * The constant is chosen by what the table makes of the sample (tools/predict_sample_rules.py, profiles/predict_whole_lines.txt):
 * places that jump about - a hash of g, the golden ratio itself - cost the benchmark's frames half as many planes again as the round-4
 * sample, or twice as many and more, a creep of c about the same or fewer, this one the fewest of those tried on two batches of XGA frames and on FHD stress.
 * What it does NOT give is evenness over the columns at every width: like every rule of this family tried (the golden ratio itself
 * included) it leaves some band of 64 columns outside 0.75 .. 1.25 of its share at one or two widths in a hundred - those where a row is
 * close to a whole number of the 15.17-line strides, 324 and 647 points among them; the same file lists them.  Every geometry of
 * tests/test_gpu_single_pass.py is held to that bound in tests/test_predict_sample.py, and a frame whose sample misleads the table costs
 * planes or a pass of k_raster, never a result.
 * The frame's first and last line give the points of theirs that belong to the frame. */
constexpr int kPredictLineBytes = 128, kPredictPointBytes = 12;
constexpr int kPredictLinePoints = (kPredictLineBytes - 8) / kPredictPointBytes;                           /* 10 */
constexpr int kPredictGroupLines = kSpecSample * kPredictLinePoints * kPredictPointBytes / kPredictLineBytes;   /* 15 */
static_assert(kPredictGroupLines * kPredictLineBytes == kSpecSample * kPredictLinePoints * kPredictPointBytes,
              "a group of lines must hold kSpecSample times the points of one line");

struct PredictRun { int first, count; };            /* the sampled points of one group: first .. first + count - 1 (count 0 .. 10) */

__host__ __device__ inline unsigned int predict_sample_offset(unsigned int g)
{
  return (((g * 0x02D346BEu) >> 16) * static_cast<unsigned int>(kPredictGroupLines)) >> 16;          /* 2^32 (golden ratio - 1) / 56 */
}
/* groups of a frame of nPoints points (1 .. 2^26) whose first byte has the address `base` */
__host__ __device__ inline int predict_sample_groups(unsigned long long base, int nPoints)
{
  const unsigned int a7 = static_cast<unsigned int>(base) & static_cast<unsigned int>(kPredictLineBytes - 1);
  const unsigned int lines = (a7 + static_cast<unsigned int>(nPoints) * kPredictPointBytes + kPredictLineBytes - 1) / kPredictLineBytes;
  return static_cast<int>((lines + kPredictGroupLines - 1) / kPredictGroupLines);
}
/* THE rule: the points of group `group` that are sampled.  A group at or beyond predict_sample_groups() gives count 0 (k_predict
 * asks for up to a few hundred groups beyond the frame's end). */
__host__ __device__ inline PredictRun predict_sample_run(unsigned long long base, int nPoints, int group)
{
  const unsigned int a7 = static_cast<unsigned int>(base) & static_cast<unsigned int>(kPredictLineBytes - 1);
  const unsigned int g = static_cast<unsigned int>(group);
  const unsigned int line = g * kPredictGroupLines + predict_sample_offset(g);
  const unsigned int hi = (line + 1u) * kPredictLineBytes - a7;          /* the line's end, in bytes from the frame's first */
  const unsigned int lo = hi - kPredictLineBytes;                        /* its start (the frame's first line: at or before the frame's) */
  const unsigned int first = hi <= static_cast<unsigned int>(kPredictLineBytes) ? 0u : (lo + kPredictPointBytes - 1) / kPredictPointBytes;
  const unsigned int whole = hi / kPredictPointBytes;
  const unsigned int end = whole < static_cast<unsigned int>(nPoints) ? whole : static_cast<unsigned int>(nPoints);
  PredictRun r;
  r.first = static_cast<int>(first);
  r.count = end > first ? static_cast<int>(end - first) : 0;
  return r;
}

/* ---- the table ---- */

__host__ __device__ inline bool predict_candidate(const unsigned int *sample, int nBins, int minHeight, int b)
{
  if(b < (minHeight > 1 ? minHeight : 1) || b >= nBins - 1)
    return false;
  const unsigned int c = sample[b], l = sample[b - 1], r = sample[b + 1];
  return c > l && c >= r && c * static_cast<unsigned int>(kSpecSample) >= 1200u && (l + r) * 2u < 3u * c + 16u;
}

__host__ __device__ inline int predict_table(const unsigned int *sample, int nBins, int minHeight, int sabotage, unsigned char *plane)
{
  unsigned char code[kMaxBins];          /* 1 = chosen peak, 2 = its lower neighbour wanted, 4 = its upper neighbour wanted */
  for(int b = 0; b < kMaxBins; b++)
  {
    code[b] = 0;
    plane[b] = 0xff;
  }
  if(sabotage == 2)
    return 0;
  for(int b = 0; b < nBins && b < kMaxBins; b++)
  {
    if(!predict_candidate(sample, nBins, minHeight, b))
      continue;
    int fuller = 0;
    for(int o = 0; o < nBins && o < kMaxBins; o++)
      if(o != b && predict_candidate(sample, nBins, minHeight, o) && (sample[o] > sample[b] || (sample[o] == sample[b] && o < b)))
        fuller++;
    if(fuller >= kMaxPlanes / 3)
      continue;
    const unsigned int l = sample[b - 1], r = sample[b + 1];
    code[b] = static_cast<unsigned char>(1u | (r > 2u * l + 8u ? 0u : 2u) | (l > 2u * r + 8u ? 0u : 4u));
  }
  const int shift = sabotage == 1 ? 3 : 0;
  auto code_of = [&](int k) -> unsigned int
  {
    k -= shift;
    return k >= 0 && k < kMaxBins ? code[k] : 0u;
  };
  auto wanted = [&](int k) -> bool
  {
    return k >= 0 && k < nBins && ((code_of(k - 1) & 4u) | (code_of(k) & 1u) | (code_of(k + 1) & 2u)) != 0u;
  };
  int n = 0;
  for(int b = 0; b < nBins && b < kMaxBins; b++)
  {
    if(!wanted(b))
      continue;
    const bool withBelow = wanted(b - 1) && (code_of(b - 1) == 5u || code_of(b) == 3u);
    if(!withBelow)
      n++;
    plane[b] = static_cast<unsigned char>(n - 1);
  }
  if(n > kMaxPlanes)
  {
    for(int b = 0; b < kMaxBins; b++)
      plane[b] = 0xff;
    return 0;
  }
  return n;
}

} // namespace ssd

#endif /* SSD_PREDICT_H_ */
