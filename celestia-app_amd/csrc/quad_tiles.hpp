// The batch leaf kernels' tile mapping (nmt_kernels.hip: k_leaf_quad_q0, k_leaf_quad_par), for
// squares of width k >= 16, k a multiple of 16. A lane is one 2x2 block of EDS cells, the
// blocks of a square form a k x k grid, and a wave is one 8x8 tile of blocks: a grid of
// k/8 x k/8 tiles. A tile whose tile row and tile column are both below k/16 lies wholly
// inside Q0 (every cell's row and column below k), every other tile wholly outside it. Each
// class has a kernel of its own, and the functions here number a class's tiles 0, 1, ... and
// say where tile i lies. Together the two classes cover the tile grid exactly once
// (tools/quad_tiles_check.cpp, no HIP, checks that on the host).
// Header-only, no HIP needed: the device code and the launchers read the same functions.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CEL_TILE_HD __host__ __device__
#else
#define CEL_TILE_HD
#endif

namespace cel {
namespace quad {

constexpr uint32_t kTileSide = 8;                       // blocks along a tile's side
constexpr uint32_t kTileLanes = kTileSide * kTileSide;  // one wave
constexpr uint32_t kGroupLanes = 256;                   // a workgroup: four tiles
constexpr uint32_t kMinSplitK = 2 * kTileSide;          // below it a tile mixes the classes

// A tile's place in the tile grid; its blocks are rows 8 * row .. 8 * row + 7, columns alike.
struct TilePos {
  uint32_t row, col;
};

CEL_TILE_HD constexpr bool split_width(uint32_t k) { return k >= kMinSplitK && k % kMinSplitK == 0; }

// Tiles of each class: with h = k/16 tiles along half a side, h^2 inside Q0 and 3h^2 outside.
CEL_TILE_HD constexpr uint32_t q0_tiles(uint32_t k) { return (k / 16) * (k / 16); }
CEL_TILE_HD constexpr uint32_t par_tiles(uint32_t k) { return 3 * (k / 16) * (k / 16); }

// Q0 tile i: row-major over the h x h tiles of the upper left quarter.
CEL_TILE_HD constexpr TilePos q0_tile(uint32_t i, uint32_t k) {
  const uint32_t h = k / 16;
  return TilePos{i / h, i % h};
}

// Parity tile i: first the right half of tile rows 0..h-1 (Q1, h tiles a row), then tile rows
// h..2h-1 whole (Q2 and Q3, 2h tiles a row), each row-major.
CEL_TILE_HD constexpr TilePos par_tile(uint32_t i, uint32_t k) {
  const uint32_t h = k / 16;
  if (i < h * h) return TilePos{i / h, h + i % h};
  const uint32_t j = i - h * h;
  return TilePos{h + j / (2 * h), j % (2 * h)};
}

// Workgroups (grid x) of a class's launch: lanes past the last tile return.
CEL_TILE_HD constexpr uint32_t groups_for(uint32_t tiles) {
  return (tiles * kTileLanes + kGroupLanes - 1) / kGroupLanes;
}

}  // namespace quad
}  // namespace cel
