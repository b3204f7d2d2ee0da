// Host-clock timing of host_disjoint.h alone (no GPU): the batched region
// encode's disjointness test for the batches tools/regions_encode_bench.py
// times, and for its worst shapes.  Prints one line per case: the median and
// the range of `reps` runs in milliseconds.
//
//   g++ -O2 -std=c++17 -I zfp-par_amd/csrc/hip -o disjoint_time tools/disjoint_time.cpp
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <random>
#include <vector>
#include "host_disjoint.h"
using namespace zfp_amd;

static void run(const char* name, const std::vector<BlockBox>& b, int reps)
{
  std::vector<double> ms;
  bool any = false;
  for (int r = 0; r < reps + 3; r++) {
    size_t ia, ib;
    const auto t0 = std::chrono::steady_clock::now();
    any = first_shared_block(b.data(), b.size(), 2, &ia, &ib);
    const auto t1 = std::chrono::steady_clock::now();
    if (r >= 3)
      ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  printf("disjointness test, %-44s %6zu entries: median %.4f ms (min %.4f, max %.4f)%s\n", name, b.size(),
         ms[ms.size() / 2], ms.front(), ms.back(), any ? "  SHARED BLOCK" : "");
}

int main()
{
  // 64 crops of 8^3 blocks on a 4 x 4 x 4 lattice of pitch 64 blocks (the bench's case b)
  std::vector<BlockBox> crops;
  for (uint32_t z = 0; z < 4; z++)
    for (uint32_t y = 0; y < 4; y++)
      for (uint32_t x = 0; x < 4; x++)
        crops.push_back(BlockBox{{64 * x, 64 * y, 64 * z}, {8, 8, 8}});
  run("64 crops on a lattice", crops, 200);
  // 4,096 one-block entries in one plane of the sweep axis: the quadratic case
  std::vector<BlockBox> plane;
  for (uint32_t i = 0; i < 4096; i++)
    plane.push_back(BlockBox{{2 * (i % 64), 2 * (i / 64), 7}, {1, 1, 1}});
  run("4,096 coplanar one-block entries", plane, 20);
  // 65,536 one-block entries scattered over a 256^3 block grid, all distinct
  std::vector<BlockBox> scattered;
  std::mt19937 rng(1);
  for (uint32_t i = 0; i < 65536; i++) {
    // one entry per 4 x 4 x 4 cell of blocks, at a random block of the cell
    const uint32_t c = i * 4u + rng() % 4u;  // a cell number below 2^18
    const uint32_t cx = c & 63u, cy = (c >> 6) & 63u, cz = c >> 12;
    const uint32_t jx = rng() % 4u, jy = rng() % 4u, jz = rng() % 4u;
    scattered.push_back(BlockBox{{4 * cx + jx, 4 * cy + jy, 4 * cz + jz}, {1, 1, 1}});
  }
  std::shuffle(scattered.begin(), scattered.end(), rng);
  run("65,536 scattered one-block entries", scattered, 10);
  return 0;
}
