// tests/test_chunk_plan.py builds and runs this: csrc/ssd_chunks.h by itself, no device.  One line of the bounds, then one line per
// (nPoints, nframes) pair given on the command line: the plan of the default tuning.
#include "ssd_chunks.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
  using namespace ssd;
  std::printf("%d %d %d %d\n", kTileHost, kMaxTilesPerBlockHost, kMaxTilesPerBlockRasterHost, kMaxTilesPerBlockInquadHost);
  const ssd_tuning tuning;
  for(int i = 1; i + 1 < argc; i += 2)
  {
    const int nPoints = std::atoi(argv[i]), nframes = std::atoi(argv[i + 1]);
    const ChunkPlan p = chunk_plan(tuning, nPoints, nframes);
    std::printf("%d %d %d %d %d %d\n", nPoints, nframes, p.chunk, p.hist, p.raster, p.inquad);
  }
  return 0;
}
