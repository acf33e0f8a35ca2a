// Stand-alone host check of the batch leaf kernels' tile mapping
// (celestia-app_amd/csrc/quad_tiles.hpp): no HIP, no device. Build it with a host compiler,
// optionally under sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I celestia-app_amd/csrc tools/quad_tiles_check.cpp -o quad_tiles_check && ./quad_tiles_check
// For k = 16 .. 512 it walks every lane of both launches as the kernels do (workgroup, lane ->
// tile, block) and checks that the two classes cover the tile grid exactly once, that each
// tile is of its class, that every block lies inside the square, and that a launch has fewer
// than one workgroup of surplus lanes.
// tests/test_quad_tiles.py builds and runs it, plain and under ASan + UBSan.
#include <cstdio>
#include <vector>

#include "quad_tiles.hpp"

using namespace cel::quad;

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAIL %s:%d: %s (k = %u)\n", __FILE__, __LINE__, #c, k); \
      fails++;                                                      \
    }                                                               \
  } while (0)

// Walks the launch of one class lane by lane; seen[tile row * side + tile column] counts
// the lanes that land in each tile of the grid.
static void walk(uint32_t k, bool q0_class, std::vector<uint32_t>& seen) {
  const uint32_t side = k / kTileSide, tiles = q0_class ? q0_tiles(k) : par_tiles(k);
  const uint32_t groups = groups_for(tiles);
  const uint64_t lanes = (uint64_t)groups * kGroupLanes, used = (uint64_t)tiles * kTileLanes;
  CHECK(lanes >= used && lanes - used < 256);
  uint64_t ran = 0;
  for (uint32_t wg = 0; wg < groups; wg++) {
    for (uint32_t th = 0; th < kGroupLanes; th++) {
      const uint32_t g = wg * kGroupLanes + th, tile = g / kTileLanes, l = g % kTileLanes;
      if (tile >= tiles) continue;  // the kernels return here
      ran++;
      const TilePos at = q0_class ? q0_tile(tile, k) : par_tile(tile, k);
      CHECK(at.row < side && at.col < side);
      if (at.row >= side || at.col >= side) continue;
      const uint32_t bi = at.row * kTileSide + l / kTileSide, bj = at.col * kTileSide + l % kTileSide;
      CHECK(bi < k && bj < k);
      // the block's cells are rows 2bi, 2bi + 1 and columns 2bj, 2bj + 1 of the 2k x 2k EDS
      CHECK(2 * bi + 1 < 2 * k && 2 * bj + 1 < 2 * k);
      const bool inside = bi < k / 2 && bj < k / 2;
      CHECK(inside == q0_class);
      // the tile as a whole: all of its blocks on one side of k/2 in each direction
      CHECK((at.row * kTileSide < k / 2) == ((at.row + 1) * kTileSide <= k / 2));
      CHECK((at.col * kTileSide < k / 2) == ((at.col + 1) * kTileSide <= k / 2));
      seen[(size_t)at.row * side + at.col]++;
    }
  }
  CHECK(ran == used);
}

int main() {
  for (uint32_t k : {16u, 32u, 64u, 128u, 256u, 512u}) {
    CHECK(split_width(k));
    const uint32_t side = k / kTileSide;
    CHECK(q0_tiles(k) + par_tiles(k) == side * side);
    std::vector<uint32_t> seen((size_t)side * side, 0);  // exactly the grid: a tile outside it is a write out of bounds
    walk(k, true, seen);
    for (uint32_t t = 0; t < side * side; t++)  // after the Q0 launch: its tiles once, whole; no other
      CHECK(seen[t] == ((t / side < side / 2 && t % side < side / 2) ? kTileLanes : 0u));
    walk(k, false, seen);
    for (uint32_t t = 0; t < side * side; t++) CHECK(seen[t] == kTileLanes);  // every tile once over both
    std::printf("k = %3u: %5u Q0 tiles in %4u workgroups, %5u parity tiles in %5u workgroups\n", k, q0_tiles(k),
                groups_for(q0_tiles(k)), par_tiles(k), groups_for(par_tiles(k)));
  }
  for (uint32_t k : {1u, 2u, 4u, 8u, 24u}) CHECK(!split_width(k));
  std::printf("quad tiles check: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
