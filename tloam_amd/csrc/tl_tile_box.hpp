// tl_tile_box.hpp -- the host arithmetic of the tiled fields (the route's, tl_api_route.hip; the frontiers',
// tl_api_frontier.hip, section 32): the tile counts of a box whose sides are no multiple of the tile, the field's and the flags'
// bytes against max_bytes, the bound that keeps every value of a field below its sentinels, a path call's output bytes and the
// cluster table's bytes once the roots are counted, every product checked before it is trusted.  No HIP and no context in here,
// so that a stand-alone program can drive it under the host sanitizers (tests/host/route_box_main.cpp, frontier_box_main.cpp),
// as tl_clear_box.hpp.  (need, the squared radius a body asks for, is tlc::need_d2 there: the one function.)
#pragma once

#include <stdint.h>

namespace tlt {

constexpr int kTileX = 32, kTileY = 8, kTileZ = 4;   // a tile's cells: x along the lanes, one block of 256 threads a tile
constexpr uint64_t kRouteOutside = 0xFFFFFFFDull;    // TLOAM_ROUTE_OUTSIDE: the route's lowest sentinel
constexpr uint64_t kFrontOutside = 0xFFFFFFFCull;    // TLOAM_FRONTIER_OUTSIDE: the frontiers' lowest sentinel; a label is a cell's index below it
// make_box's cells_below, the first count of cells a field refuses.  The route: 5 * cells >= kRouteOutside, without forming
// 5 * cells (a path of all the cells by vertex steps would meet a sentinel).  The frontiers: a cell's index would meet a sentinel
constexpr uint64_t kRouteCellsBelow = (kRouteOutside + 4u) / 5u;
constexpr uint64_t kFrontCellsBelow = kFrontOutside;
constexpr uint64_t kClusterBytes = 64 + 64 + 4 + 4;  // a component's share of the table: its record, the kept list's copy of it,
                                                     // its root and its index in the kept list

struct TileBox {
  int64_t n[3];       // cells per axis
  int64_t tiles[3];   // tiles per axis: ceil(n / tile), the last one partial when n is no multiple
  uint64_t cells;     // n[0] * n[1] * n[2]
  uint64_t ntiles;    // tiles[0] * tiles[1] * tiles[2]
  uint64_t bytes;     // 4 * cells (the field) + 2 * 4 * ntiles (the two flag arrays, a word a tile)
};

// The field over n[] cells per axis (each in [1, 2^21], as tlc::make_field leaves them; nz = 1 is the column form).  false: a
// count out of that range, a product that overflows, more than max_bytes bytes, or cells >= cells_below (kRouteCellsBelow,
// kFrontCellsBelow); *out is then not to be used.
inline bool make_box(const int64_t n[3], int64_t max_bytes, uint64_t cells_below, TileBox* out) {
  const int tile[3] = {kTileX, kTileY, kTileZ};
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 1 || n[a] > ((int64_t)1 << 21)) return false;
    out->n[a] = n[a];
    out->tiles[a] = (n[a] + tile[a] - 1) / tile[a];   // <= 2^21
  }
  if (max_bytes < 4) return false;
  const uint64_t cap_cells = (uint64_t)max_bytes / 4u;
  // n[a] <= 2^21: the product of two fits 42 bits; the third is checked by division before it is formed
  const uint64_t plane = (uint64_t)n[0] * (uint64_t)n[1];
  if (plane > cap_cells || (uint64_t)n[2] > cap_cells / plane) return false;
  out->cells = plane * (uint64_t)n[2];                 // <= max_bytes / 4 < 2^61
  if (out->cells >= cells_below) return false;
  // tiles[a] <= n[a]: ntiles <= cells < 2^32, and 8 * ntiles + 4 * cells < 2^36
  out->ntiles = (uint64_t)out->tiles[0] * (uint64_t)out->tiles[1] * (uint64_t)out->tiles[2];
  out->bytes = 4u * out->cells + 8u * out->ntiles;
  return out->bytes <= (uint64_t)max_bytes;
}

// a path call's centres: n * max_cells * 24 bytes held to max_bytes.  false: n or max_cells is 0, or the product (checked by
// division, never formed before) is more; *waypoints = n * max_cells
inline bool path_room(uint64_t n, uint64_t max_cells, int64_t max_bytes, uint64_t* waypoints) {
  if (n == 0 || max_cells == 0 || max_bytes < 24) return false;
  const uint64_t cap = (uint64_t)max_bytes / 24u;
  if (n > cap || max_cells > cap / n) return false;
  *waypoints = n * max_cells;
  return true;
}

// The cluster table of `clusters` components beside a field of field_bytes (a TileBox's): kClusterBytes a component.  false:
// field and table together are more than max_bytes (checked by division: the product is formed only when it fits).
inline bool table_room(uint64_t clusters, uint64_t field_bytes, int64_t max_bytes, uint64_t* table_bytes) {
  if (max_bytes < 0 || field_bytes > (uint64_t)max_bytes) return false;
  const uint64_t left = (uint64_t)max_bytes - field_bytes;
  if (clusters > left / kClusterBytes) return false;
  *table_bytes = clusters * kClusterBytes;
  return true;
}

}  // namespace tlt
