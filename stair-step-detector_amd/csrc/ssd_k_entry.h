/* ssd_k_entry.h - what every stage header starts from: how a kernel whose body stands in its entry point is spelled (SSD_ENTRY,
 * SSD_BYVAL), the tools builds' macros (SSD_CHK, SSD_CNT, ssd_phase.h) and the constants that more than one stage and the launch
 * rules share.  DESIGN.md section 3b says who includes what. */
#ifndef SSD_K_ENTRY_H_
#define SSD_K_ENTRY_H_
/* The device code is compiled in more than one translation unit.  In ssd_kernels.hip it is the one-calibration path: every
 * kernel takes the handle's constants by value.  ssd_kernels_cams.hip, which includes that file for the stages' bodies, and
 * ssd_kernels_refit.hip, which includes only the stage headers it builds on, define SSD_CAMERAS_TU before their first include (this
 * is the one place that spells the macros by it): the kernels whose body stands in the entry point itself become device functions
 * there (SSD_ENTRY gives them their second name, SSD_BYVAL turns the by-value constants into references), and the cameras entry
 * points call them with the frame's camera record.
 * Without SSD_CAMERAS_TU both macros spell exactly the entry point, so ssd_kernels.hip's code does not change.
 * That rule - a kernel's code object stays byte for byte what it was - holds for the chain K0 - K5, which bench.py measures.  The
 * extension kernels K6 - K8 (labels, surface moments, the refit, the three riser passes) are written from shared pieces and held to
 * their results, their resources and their time instead: DESIGN.md section 7l. */
#ifndef SSD_CAMERAS_TU
#define SSD_ENTRY(bounds, kernel, block) __global__ bounds void kernel
#define SSD_BYVAL(T) T
#else
#define SSD_ENTRY(bounds, kernel, block) __device__ __forceinline__ void block
#define SSD_BYVAL(T) const T &
#undef SSD_PHASE_TIMING       /* the tools' clocks and counters are ssd_kernels.hip's translation unit's */
#undef SSD_COUNT
#endif
#include "ssd_device.h"
#include "ssd_moments.h"
#include "ssd_math.h"
#include "ssd_quadtest.h"
#include "ssd_closing.h"
#include "ssd_bestline.h"
#include "ssd_sort.h"
#include "ssd_predict.h"    /* k_predict's sample rule (predict_sample_run), shared with the tests */
#include "ssd_refit.h"      /* the refit's gate rule (refit_keeps), shared with the host */

namespace ssd
{

#include "ssd_phase.h"      /* tools builds: clocks at the marks below; product build: empty macros */

/* Bounds-checked tools build (-DSSD_CHECKED, tools/checked.sh; GPU sanitizers are not available on this pool): the index of every
 * store or atomic whose address comes from a point, a pixel, a window or a list is compared with the extent of what it writes
 * into FIRST; a violation is reported from the device (one line, "SSD_CHECK site ...") and the access is dropped.  In the
 * product build the macro is the constant `true`. */
#ifdef SSD_CHECKED
__device__ __noinline__ void ssd_chk_report(int site, unsigned long long idx, unsigned long long limit)
{
  printf("SSD_CHECK site %d index %llu limit %llu block (%u, %u) thread %u\n", site, idx, limit, blockIdx.x, blockIdx.y, threadIdx.x);
}
__device__ __forceinline__ bool ssd_chk(int site, unsigned long long idx, unsigned long long limit)
{
  if(idx < limit)
    return true;
  ssd_chk_report(site, idx, limit);
  return false;
}
#define SSD_CHK(site, idx, limit) ssd_chk((site), static_cast<unsigned long long>(idx), static_cast<unsigned long long>(limit))
#else
#define SSD_CHK(site, idx, limit) (true)
#endif

/* Tools build (-DSSD_COUNT, tools/k1count.py): what K1's windows do - tiles with candidate points, window moves, words flushed,
 * pixels that missed the window.  In the product build the macros are empty. */
#ifdef SSD_COUNT
__device__ unsigned long long ssd_k1_counters[8];
#define SSD_CNT(i, n) do { if(threadIdx.x % 64 == 0) atomicAdd(&ssd_k1_counters[i], static_cast<unsigned long long>(n)); } while(0)
#define SSD_CNT_LANES(i, pred) do { const unsigned long long cnt_m = __ballot(pred); if(threadIdx.x % 64 == 0 && cnt_m) atomicAdd(&ssd_k1_counters[i], static_cast<unsigned long long>(__popcll(cnt_m))); } while(0)
#else
#define SSD_CNT(i, n) do { } while(0)
#define SSD_CNT_LANES(i, pred) do { } while(0)
#endif

/* threads of the image kernels (K3, K5): one block per image, a chain of short phases.  More waves = fewer rows per
 * thread in the closing (latency), but the arithmetic phases (BestLine) run at the CU's rate whatever the count, and every
 * barrier and every per-wave preamble is paid per wave: measured on 1024 XGA frames, K3 takes 0.106 / 0.146 / 0.307 ms with
 * 256 / 512 / 1024 threads, on a single frame 30 / 26.5 / 28 us.  Hence two instantiations: 256 for batches, 512 for a few
 * frames. */
/* (round 4, FHD stress batch of 256 frames, same box, alternating: k_outline with 256 / 512 / 1024 threads per image 0.310 / 0.363 /
 * 0.438 ms — the batch is bound by the images' total work, which more threads do not shrink; tools/mkvariant.sh with
 * -DSSD_IMG_THREADS_BATCH=..) */
#ifndef SSD_IMG_THREADS_BATCH
#define SSD_IMG_THREADS_BATCH 256
#endif
constexpr int kImgThreadsBatch = SSD_IMG_THREADS_BATCH, kImgThreadsFew = 512;   /* chosen per launch (launch_outline / launch_final) */
constexpr int kMaxImgWaves = (kImgThreadsBatch > kImgThreadsFew ? kImgThreadsBatch : kImgThreadsFew) / 64;
constexpr int kImgFewFrames = 64;
constexpr int kMaxCols = SSD_MAX_SCANS;      /* scan columns per image (W/25 + 1 <= 128) */
constexpr int kMaxProbe = SSD_MAX_EDGE_PTS;  /* probe rows per vertical edge: (H - 1)/10 + 1 <= 256, make_params refuses H > 2560 */

} // namespace ssd

#endif /* SSD_K_ENTRY_H_ */
