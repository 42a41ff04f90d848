// Stripe ownership of a streaming window (grp_classify_stream_begin_striped): stripe t = reads [t * stripe_reads,
// (t + 1) * stripe_reads) of the window belongs to rank t % n_owners, and a rank's launch draws only its own reads'
// tiles.  One owner: the whole window is that launch's.  Everything the engine derives from the rule is here; plain
// C++, no HIP types (tests/stream_stripes_main.cpp holds it against the tests' Python model).
#pragma once
#include <stdint.h>

namespace gr {
namespace stripes {

struct Window
{
  const uint64_t* tile0 = nullptr; // of the batch: read i has tiles [tile0[i], tile0[i + 1])
  uint32_t first = 0, count = 0;   // the window's reads in the batch
  uint32_t stripe_reads = 0, n_owners = 1, owner = 0;

  bool striped() const { return n_owners > 1; }
  // j: window index of a read
  bool owns(uint32_t j) const { return !striped() || (j / stripe_reads) % n_owners == owner; }
  uint64_t tiles_of(uint32_t j) const { return tile0[first + j + 1] - tile0[first + j]; }
};

struct Totals
{
  uint64_t n_mine = 0;         // tiles of the owner's reads: what its launch draws
  uint32_t n_decidable = 0;    // the owner's reads with at least one tile (the launch decides these; reads without a tile are the host's)
  uint64_t max_tiles_read = 0; // the most tiles of any read of the window, whoever owns it (any of them may insert)
};

inline Totals
totals(const Window& w)
{
  Totals t;
  for (uint32_t j = 0; j < w.count; ++j) {
    const uint64_t ntj = w.tiles_of(j);
    t.max_tiles_read = ntj > t.max_tiles_read ? ntj : t.max_tiles_read;
    if (ntj != 0 && w.owns(j)) {
      t.n_mine += ntj;
      ++t.n_decidable;
    }
  }
  return t;
}

// the owner's tiles as window indices (tile - tile0[first]), in order: Totals::n_mine entries
inline void
tile_list(const Window& w, uint32_t* out)
{
  const uint64_t t0 = w.tile0[w.first];
  uint64_t n = 0;
  for (uint32_t j = 0; j < w.count; ++j) {
    if (w.owns(j)) {
      for (uint64_t t = w.tile0[w.first + j]; t < w.tile0[w.first + j + 1]; ++t) {
        out[n++] = (uint32_t)(t - t0);
      }
    }
  }
}

// an insert at read x of the window (anybody's): where the owner's launch carries on
struct Resume
{
  uint32_t decided_base = 0; // the owner's decidable reads up to and including x
  uint64_t resume_tile = 0;  // the owner's tiles up to and including x: where its dispenser starts over
};

inline Resume
resume_at(const Window& w, uint32_t x)
{
  Resume r;
  for (uint32_t j = 0; j <= x && j < w.count; ++j) {
    if (w.owns(j)) {
      const uint64_t ntj = w.tiles_of(j);
      r.decided_base += ntj != 0;
      r.resume_tile += ntj;
    }
  }
  return r;
}

} // namespace stripes
} // namespace gr
