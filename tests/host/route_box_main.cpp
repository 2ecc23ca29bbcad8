// A stand-alone driver of the route field's host arithmetic (tloam_amd/csrc/tl_tile_box.hpp: the tile counts of a box whose
// sides are no multiple of the tile, the field's and the flags' bytes against max_bytes, the bound 5 * cells < TLOAM_ROUTE_OUTSIDE,
// a path call's n * max_cells * 24 bytes, every product checked), meant to be compiled for the host alone with
// -fsanitize=address,undefined and run on a machine without a GPU (tests/test_closed_map_route_host.py does).  No HIP in here.
// Prints "ok <checks>" and exits 0 when every check holds.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <limits>

#include "../../tloam_amd/csrc/tl_tile_box.hpp"

namespace {

int checks = 0;
#define CHECK(x)                                                       \
  do {                                                                 \
    ++checks;                                                          \
    if (!(x)) {                                                        \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);          \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

const int64_t kGiB = (int64_t)1 << 30, kMost = std::numeric_limits<int64_t>::max();

int64_t up(int64_t n, int64_t t) { return (n + t - 1) / t; }

void check_tiles() {
  tlt::TileBox B;
  // every side from one cell to a little over two tiles: full tiles, partial last tiles, boxes thinner than a tile
  for (int64_t x = 1; x <= 2 * tlt::kTileX + 3; x += (x < 4 || x > 28) ? 1 : 5)
    for (int64_t y = 1; y <= 2 * tlt::kTileY + 2; ++y)
      for (int64_t z = 1; z <= 2 * tlt::kTileZ + 1; ++z) {
        const int64_t n[3] = {x, y, z};
        CHECK(tlt::make_box(n, kGiB, tlt::kRouteCellsBelow, &B));
        CHECK(B.n[0] == x && B.n[1] == y && B.n[2] == z && B.cells == (uint64_t)(x * y * z));
        CHECK(B.tiles[0] == up(x, tlt::kTileX) && B.tiles[1] == up(y, tlt::kTileY) && B.tiles[2] == up(z, tlt::kTileZ));
        CHECK(B.ntiles == (uint64_t)(B.tiles[0] * B.tiles[1] * B.tiles[2]) && B.bytes == 4 * B.cells + 8 * B.ntiles);
        for (int a = 0; a < 3; ++a) {
          const int64_t tile = a == 0 ? tlt::kTileX : a == 1 ? tlt::kTileY : tlt::kTileZ;
          CHECK(B.tiles[a] * tile >= n[a] && (B.tiles[a] - 1) * tile < n[a]);   // the last tile holds at least one cell
        }
        // exactly the bytes it needs, and one less
        CHECK(tlt::make_box(n, (int64_t)B.bytes, tlt::kRouteCellsBelow, &B));
        tlt::TileBox C;
        CHECK(!tlt::make_box(n, (int64_t)B.bytes - 1, tlt::kRouteCellsBelow, &C));
      }
  const int64_t wall[3] = {76, 56, 56};
  CHECK(tlt::make_box(wall, kGiB, tlt::kRouteCellsBelow, &B) && B.tiles[0] == 3 && B.tiles[1] == 7 && B.tiles[2] == 14 && B.bytes == 4 * 238336 + 8 * 294);
  const int64_t layer[3] = {76, 56, 1};
  CHECK(tlt::make_box(layer, kGiB, tlt::kRouteCellsBelow, &B) && B.ntiles == 21 && B.bytes == 4 * 4256 + 8 * 21);
}

void check_refusals() {
  tlt::TileBox B;
  const int64_t one[3] = {4, 4, 4};
  for (int64_t bad : {(int64_t)0, (int64_t)-1, (int64_t)3, std::numeric_limits<int64_t>::min()}) CHECK(!tlt::make_box(one, bad, tlt::kRouteCellsBelow, &B));
  CHECK(tlt::make_box(one, 4 * 64 + 8, tlt::kRouteCellsBelow, &B) && !tlt::make_box(one, 4 * 64 + 7, tlt::kRouteCellsBelow, &B));
  const int64_t single[3] = {1, 1, 1};
  CHECK(!tlt::make_box(single, 4, tlt::kRouteCellsBelow, &B) && !tlt::make_box(single, 11, tlt::kRouteCellsBelow, &B) && tlt::make_box(single, 12, tlt::kRouteCellsBelow, &B) && B.bytes == 12);
  for (int a = 0; a < 3; ++a)
    for (int64_t bad : {(int64_t)0, (int64_t)-4, ((int64_t)1 << 21) + 1, kMost}) {
      int64_t n[3] = {8, 8, 8};
      n[a] = bad;
      CHECK(!tlt::make_box(n, kMost, tlt::kRouteCellsBelow, &B));
    }
  // the largest sides: every product would overflow 64 bits if it were formed unchecked
  const int64_t huge[3] = {(int64_t)1 << 21, (int64_t)1 << 21, (int64_t)1 << 21};
  CHECK(!tlt::make_box(huge, kGiB, tlt::kRouteCellsBelow, &B) && !tlt::make_box(huge, kMost, tlt::kRouteCellsBelow, &B));
  // 5 * cells >= 0xFFFFFFFD: 858 993 459 cells is the first count refused, whatever max_bytes allows
  const uint64_t first_refused = (tlt::kRouteOutside + 4) / 5;
  CHECK(first_refused == 858993459ull && 5 * first_refused >= tlt::kRouteOutside && 5 * (first_refused - 1) < tlt::kRouteOutside);
  CHECK(tlt::kRouteCellsBelow == first_refused);
  const int64_t below[3] = {858993458, 1, 1};  // (a side beyond 2^21: refused for that alone)
  CHECK(!tlt::make_box(below, kMost, tlt::kRouteCellsBelow, &B));
  const int64_t ok[3] = {(int64_t)1 << 21, 409, 1};           // 857 735 168 cells: under the bound
  CHECK(tlt::make_box(ok, kMost, tlt::kRouteCellsBelow, &B) && 5 * B.cells < tlt::kRouteOutside);
  const int64_t over[3] = {(int64_t)1 << 21, 410, 1};         // 859 832 320 cells: over it
  CHECK(!tlt::make_box(over, kMost, tlt::kRouteCellsBelow, &B));
  const int64_t cube[3] = {1024, 1024, 819};                  // 858 783 744: under
  CHECK(tlt::make_box(cube, kMost, tlt::kRouteCellsBelow, &B));
  const int64_t cube1[3] = {1024, 1024, 820};                 // 859 832 320: over
  CHECK(!tlt::make_box(cube1, kMost, tlt::kRouteCellsBelow, &B));
  // under 1 GiB the bound cannot bind: the bytes bind first
  const int64_t gib[3] = {1024, 1024, 256};
  CHECK(!tlt::make_box(gib, kGiB, tlt::kRouteCellsBelow, &B) && tlt::make_box(gib, kGiB + 8 * 32 * 128 * 64, tlt::kRouteCellsBelow, &B));
}

void check_paths() {
  uint64_t w = 7;
  CHECK(!tlt::path_room(0, 5, kGiB, &w) && !tlt::path_room(5, 0, kGiB, &w) && !tlt::path_room(1, 1, 23, &w) && w == 7);
  CHECK(tlt::path_room(1, 1, 24, &w) && w == 1);
  for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 257ull, 100000ull})
    for (uint64_t m : {1ull, 2ull, 599ull, 65536ull}) {
      const uint64_t bytes = n * m * 24;
      CHECK(tlt::path_room(n, m, (int64_t)bytes, &w) && w == n * m);
      CHECK(!tlt::path_room(n, m, (int64_t)bytes - 1, &w));
      CHECK(tlt::path_room(n, m, kGiB, &w) == (bytes <= (uint64_t)kGiB));
    }
  // products that overflow 64 bits are refused, never formed
  const uint64_t big = std::numeric_limits<uint64_t>::max();
  CHECK(!tlt::path_room(big, big, kMost, &w) && !tlt::path_room(big, 2, kMost, &w) && !tlt::path_room(2, big, kMost, &w));
  CHECK(!tlt::path_room((uint64_t)1 << 40, (uint64_t)1 << 40, kMost, &w));
  CHECK(!tlt::path_room(1, 1, -1, &w) && !tlt::path_room(1, 1, std::numeric_limits<int64_t>::min(), &w));
}

}  // namespace

int main() {
  check_tiles();
  check_refusals();
  check_paths();
  printf("ok %d\n", checks);
  return 0;
}
