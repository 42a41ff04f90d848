// Tile geometry, shared by the host library (g++) and the HIP engine (hipcc, host and device): which bases a tile's
// string covers and how many frames it has.  Every kernel prologue and every host-side count of frames takes the rule
// from here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GR_GEOM_HD __host__ __device__ __forceinline__
#else
#define GR_GEOM_HD inline
#endif

namespace gr {
namespace geom {

// lanes of a workgroup of the engine's kernels (grpath_hip.hip THREADS)
constexpr uint32_t WG_THREADS = 256;

// Frames of a full tile.  The tile string is tile + k - 1 bases with the reference's -k (read_hashing.cpp:44-45), and a
// frame exists while seed 0, the shortest, can roll (multiLensfrHashIterator.hpp:29-68).  Seed 0 spans span0 = k bases,
// or k - 1 at odd k (make_seed_pattern's halves are k/2 positions each, spaced_seeds.cpp:27-66): tile + k - span0
// frames, one more than tile at odd k.  The longest seed spans span0 + h - 1 bases, the minimum length of a read that
// takes part in the fill.
GR_GEOM_HD uint32_t
frames_per_tile(uint32_t tile, uint32_t k, uint32_t span0)
{
  return tile + k - span0;
}

// Tile ti of a read of len bases (len > ti * tile): its string is seq.substr(ti * tile, tile + k - 1)
// (read_hashing.cpp:44-45) — Lp bases from `start`, fewer in the read's last tile — and has Lp - span0 + 1 frames, none
// where seed 0 does not fit.
struct TileExtent
{
  uint32_t start;
  uint32_t Lp;
  uint32_t frames;
};

GR_GEOM_HD TileExtent
tile_extent(uint32_t tile, uint32_t k, uint32_t span0, uint32_t len, uint32_t ti)
{
  TileExtent e;
  e.start = ti * tile;
  const uint32_t full = tile + k - 1u, rest = len - e.start;
  e.Lp = full < rest ? full : rest;
  e.frames = (e.Lp >= span0) ? (e.Lp - span0 + 1u) : 0u;
  return e;
}

// units of WG_THREADS frames per tile of the kernels that walk a tile that way (one workgroup per unit)
GR_GEOM_HD uint32_t
tile_parts(uint32_t frames_per_tile)
{
  return (frames_per_tile + WG_THREADS - 1u) / WG_THREADS;
}

// Frames per pass of the query's helper-lane layout (k_query): the first three waves of a workgroup end on H - 1 helper
// lanes, the last wave has none
constexpr uint32_t
helper_pass_frames(int H)
{
  static_assert(WG_THREADS == 256, "the helper-lane layout is written for four waves per workgroup");
  return 3u * (64u - ((uint32_t)H - 1u)) + 64u;
}

} // namespace geom
} // namespace gr
