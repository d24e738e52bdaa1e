// The host arithmetic of the image partitions: the tile deal of the multi-GPU render (lumc_tile_*, include/lum_core.h) and the pixel lists of the
// undersampling preview. No HIP call.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../../include/lum_core.h"
#include "tiles.h"

extern "C" {

// The tile deal ("block -> GPU by interleaved round-robin for load balance"). Round 5: a rank-1 lattice instead of t % world over the
// row-major grid. The old deal is periodic in x with period `world` tiles whenever the tile row length is a multiple of `world` - at 3840 px (120 tiles)
// and 8 ranks every rank owned vertical 32-pixel stripes. Now tile (x, y) belongs to rank (x + k * y) % world, with k chosen among the steps COPRIME to
// `world` so that a rank's tiles form the most isotropic lattice: k maximises the shortest distance between two tiles of one rank (world 8: k = 3, nearest
// own tiles at (2, 2) and (1, -3); world 2: the checkerboard; world 4 and 6: k = 1, the diagonals). Coprime (round 6, advisor): the row offset k * y then
// runs through every residue, so the tiles a row has beyond a multiple of `world` go to every rank in turn - with k = 2 at 4 ranks (round 5's choice, more
// isotropic) they always went to the same half (1376 x 1080: max / mean share 1.023). Balance bound: over any `world` consecutive tile rows every rank owns
// the same number of tiles; a frame's shares differ by at most (tiles_y % world) tiles (+ the clipped tiles of the right and bottom edge).
// LUM_TILE_DEAL=rowmajor restores t % world (A/B of the load-balance table, profiles/r05_load_balance.json).
uint32_t lumc_tile_lattice_step(uint32_t world) {
  if (world < 2) return 0;
  auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; };
  uint32_t best_k = 1; int64_t best = -1;
  for (uint32_t k = 1; k < world; k++) {
    if (gcd(k, world) != 1u) continue;
    int64_t shortest = INT64_MAX;
    for (int64_t b = -(int64_t) world; b <= (int64_t) world; b++)
      for (int64_t a = -(int64_t) world; a <= (int64_t) world; a++) {
        if ((a == 0 && b == 0) || ((a + (int64_t) k * b) % (int64_t) world) != 0) continue;
        shortest = std::min(shortest, a * a + b * b);
      }
    if (shortest > best) { best = shortest; best_k = k; }
  }
  return best_k;
}

static bool tile_deal_rowmajor() {
  static const bool v = [] { const char* e = std::getenv("LUM_TILE_DEAL"); return e && std::strcmp(e, "rowmajor") == 0; }();
  return v;
}

// the step of a world size, computed once per size (the search is cubic in `world`; the host's render threads call this concurrently)
static uint32_t tile_lattice_step_cached(uint32_t world) {
  static uint32_t step_of[65];
  static std::once_flag once;
  std::call_once(once, [] { for (uint32_t w = 0; w <= 64; w++) step_of[w] = lumc_tile_lattice_step(w); });
  if (world <= 64) return step_of[world];
  static std::mutex m;
  static std::map<uint32_t, uint32_t> beyond;
  std::lock_guard<std::mutex> lock(m);
  auto it = beyond.find(world);
  if (it == beyond.end()) it = beyond.emplace(world, lumc_tile_lattice_step(world)).first;
  return it->second;
}

uint32_t lumc_tile_owner(uint32_t tile_x, uint32_t tile_y, uint32_t tiles_x, uint32_t world) {
  if (world < 2) return 0;
  if (tile_deal_rowmajor()) return (uint32_t) (((uint64_t) tile_y * tiles_x + tile_x) % world);
  return (uint32_t) (((uint64_t) tile_x + (uint64_t) tile_lattice_step_cached(world) * tile_y) % world);
}

// Writes the rank's pixel indices (x + y * width): its tiles in row-major tile order, rows within a tile; `out` may be NULL to query the count.
int lumc_tile_pixels(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, uint32_t tile, uint32_t* out, uint32_t* count) {
  if (!count || world == 0 || rank >= world || tile == 0) return 1;
  const uint32_t tx = (width + tile - 1) / tile, ty = (height + tile - 1) / tile;
  uint32_t n = 0;
  for (uint32_t j = 0; j < ty; j++)
    for (uint32_t i = 0; i < tx; i++) {
      if (lumc_tile_owner(i, j, tx, world) != rank) continue;
      const uint32_t x0 = i * tile, y0 = j * tile;
      for (uint32_t y = y0; y < std::min(y0 + tile, height); y++)
        for (uint32_t x = x0; x < std::min(x0 + tile, width); x++) { if (out) out[n] = x + y * width; n++; }
    }
  *count = n;
  return 0;
}

}  // extern "C"

// The pixels of one iteration of the undersampling preview (tasks_create, cuda/kernels.cuh:47-95, whole-frame window): one per block of
// 2^stage pixels, at the block's corner or half a block in, by the iteration's two bits.
std::vector<uint32_t> undersampling_pixels(uint32_t width, uint32_t height, uint32_t stage, uint32_t iteration) {
  const uint32_t scale = 1u << stage;
  const uint32_t uw = (width + scale - 1) >> stage, uh = (height + scale - 1) >> stage;
  std::vector<uint32_t> px;
  px.reserve((size_t) uw * uh);
  for (uint32_t id = 0; id < uw * uh; id++) {
    uint32_t y = id / uw, x = id - y * uw;
    if (scale > 1) {
      x = x * scale + ((iteration & 1u) ? 0u : scale >> 1);
      y = y * scale + ((iteration & 2u) ? 0u : scale >> 1);
    }
    if (x >= width || y >= height) continue;
    px.push_back(x + y * width);
  }
  return px;
}
