/*
 * ssd_chunks.h — how many points a block of each streaming kernel takes: the chunk rules of an enqueue, pure functions of the handle's
 * launch-geometry constants (ssd_tuning), the frame's points and the batch's frames.  A plain header: no HIP, no handle, no stream, no
 * include - it defines the constants and the tuning record it reads, and ssd_launch.h and ssd_handle.h take them from here -, so any C++
 * compiler builds a program around chunk_plan (tests/test_chunk_plan.py does).
 */
#ifndef SSD_CHUNKS_H_
#define SSD_CHUNKS_H_

namespace ssd
{
constexpr int kTileHost = 1024;
/* kTileHost = kThreads * kPts of ssd_kernels.hip: chunk sizes are multiples of it; a block's chunk is at most
 * kMaxTilesPerBlockHost tiles (K1 keeps the chunk's cell masks, K2/K4/K6 the list of its wanted cells, in LDS) */
#ifndef SSD_MAX_TILES
#define SSD_MAX_TILES 32
#endif
constexpr int kMaxTilesPerBlockHost = SSD_MAX_TILES;
constexpr int kMaxTilesPerBlockRasterHost = 128;   /* K2 only */
constexpr int kMaxTilesPerBlockInquadHost = 128;   /* K4 only */
} // namespace ssd

/* Launch-geometry constants of a handle.  The product uses the compiled defaults below (each one measured: chunk_plan, below).
 * Only a tools build (make EXTRA=-DSSD_TUNING OUT=../lib_tuning, tools/exp*.sh) reads
 * overrides from the environment (SSD_CHUNK_POINTS, SSD_TARGET_BLOCKS, SSD_K1_BLOCKS_PER_FRAME, SSD_K24_MIN_BLOCKS,
 * SSD_K24_TALL_BLOCKS, SSD_K2_CHUNK_TILES, SSD_K4_CHUNK_TILES, SSD_WIN_SHIFT, SSD_WIN_SHIFT_G, SSD_FUSE_GROUP_FASTEST), and only once, in ssd_create:
 * no entry point of the product library calls getenv. */
struct ssd_tuning
{
  int chunkPoints = 0;            /* > 0: the general chunk, forced */
  int targetBlocks = 32768;       /* blocks a streaming launch aims at */
  int k1BlocksPerFrame = 256;     /* K1: at most this many blocks per frame (their final atomics share the frame's histogram) */
  int k24MinBlocks = 1536, k24TallBlocks = 6144;
  int k2ChunkTiles = 32, k4ChunkTiles = 16;
  int winShift = 0, winShiftGround = 0;     /* > 0: shape of the waves' LDS image windows, forced */
  int recordPad = 0;              /* cell records per frame added to the stride between the frames' record arrays */
  int fuseGroupFastest = 0;       /* k_depth_fuse's grid: 0 = neighbouring blocks take neighbouring chunks of one group, 1 = the same chunk of neighbouring groups */
};

#pragma GCC visibility push(hidden)            /* internal to libssd_hip.so, like ssd_host.h */

namespace ssd
{

/* points per block: `chunk` for every kernel that has no rule of its own (the extension passes, the labels), K1's, K2's, K4's */
struct ChunkPlan
{
  int chunk, hist, raster, inquad;
};

inline int choose_chunk(const ssd_tuning &tune, int nPoints, int nframes)
{
  const int forced = tune.chunkPoints;
  if(forced > 0)
  {
    const int c = ((forced + kTileHost - 1) / kTileHost) * kTileHost;
    return c > kMaxTilesPerBlockHost * kTileHost ? kMaxTilesPerBlockHost * kTileHost : c;
  }
  const int target = tune.targetBlocks;
  int cpf = (target + nframes - 1) / nframes;
  const int maxCpf = (nPoints + kTileHost - 1) / kTileHost;
  if(cpf > maxCpf) cpf = maxCpf;
  if(cpf < 1) cpf = 1;
  const int per = (nPoints + cpf - 1) / cpf;
  int chunk = ((per + kTileHost - 1) / kTileHost) * kTileHost;
  /* a block should stream at least 32 tiles (its prologue copies the frame's tables, its epilogue flushes the LDS
   * histogram / windows): measured +0.5 % on the XGA batch, +6.5 % on the FHD stress batch (tools/target_blocks.sh) —
   * as long as that leaves the machine at least 8192 blocks (small batches, single frames: latency first) */
  long long minChunk = static_cast<long long>(kMaxTilesPerBlockHost) * kTileHost;
  const long long total = static_cast<long long>(nPoints) * nframes;
  if(total / minChunk < 8192)
    minChunk = total / 8192 / kTileHost * kTileHost;
  if(chunk < minChunk)
    chunk = static_cast<int>(minChunk);
  if(chunk > kMaxTilesPerBlockHost * kTileHost)
    chunk = kMaxTilesPerBlockHost * kTileHost;
  return chunk;
}

inline ChunkPlan chunk_plan(const ssd_tuning &tune, int nPoints, int nframes)
{
  const int chunk = choose_chunk(tune, nPoints, nframes);
  /* K2 and K4 walk cell columns: the taller a block's chunk, the fewer window flushes and block starts per cell (below) */
  /* K1 ends every block with up to 121 global atomics into the frame's histogram: with one-tile chunks (single frames) 768
   * blocks queue up on the same addresses; at most ssd_tuning::k1BlocksPerFrame blocks per frame keeps that short */
  int chunkHist = chunk;
  {
    const int perFrame = tune.k1BlocksPerFrame;
    const int tilesPerFrame = (nPoints + kTileHost - 1) / kTileHost;
    int t = (tilesPerFrame + perFrame - 1) / perFrame;
    if(t > kMaxTilesPerBlockHost) t = kMaxTilesPerBlockHost;
    if(t * kTileHost > chunkHist) chunkHist = t * kTileHost;
  }
  int chunkRaster = chunk, chunkInquad = chunk;
  {
    /* Blocks of K2 / K4 by batch size (XGA, tools/exp_frames.sh, 1-128 frames swept): what a block pays per start (state,
     * LDS, cell list, window flush, final atomics) wants tall chunks, the 2048 block slots of the chip want >= ~1536 blocks,
     * and a grid of one to two rounds of slots wants more, smaller blocks for its tail.  Rule: chunks of more than 8 tiles
     * only while they leave >= 6144 blocks (three rounds); else as tall as leaves >= 1536 blocks, K2 never below 2 tiles.
     * Against the former ">= 600 blocks": 8 / 16 / 32 / 64 frames 46 -> 49 k, 73 -> 82 k, 113 -> 124 k, 159 -> 172 k frames/s. */
    const long long totalTiles = (static_cast<long long>(nPoints) + kTileHost - 1) / kTileHost * nframes;
    const int minBlocks = tune.k24MinBlocks, tallBlocks = tune.k24TallBlocks;
    int t2 = tune.k2ChunkTiles, t4 = tune.k4ChunkTiles;
    if(t2 > kMaxTilesPerBlockRasterHost) t2 = kMaxTilesPerBlockRasterHost;
    if(t4 > kMaxTilesPerBlockInquadHost) t4 = kMaxTilesPerBlockInquadHost;
    auto pick = [&](int t, int tMin)
    {
      while(t > 8 && totalTiles / t < tallBlocks) t /= 2;
      while(t > tMin && totalTiles / t < minBlocks) t /= 2;
      return t;
    };
    t2 = pick(t2, 2);
    t4 = pick(t4, 1);
    if(t2 * kTileHost > chunkRaster) chunkRaster = t2 * kTileHost;
    if(t4 * kTileHost > chunkInquad) chunkInquad = t4 * kTileHost;
  }
  return ChunkPlan{ chunk, chunkHist, chunkRaster, chunkInquad };
}

} // namespace ssd

#pragma GCC visibility pop

#endif
