// A stand-alone driver of the frontier field's host arithmetic (tloam_amd/csrc/tl_tile_box.hpp: the tile counts of a box whose
// sides are no multiple of the tile, the field's and the flags' bytes against max_bytes, the bound cells < TLOAM_FRONTIER_OUTSIDE,
// the cluster table's 136 bytes a component beside the field, every product checked), meant to be compiled for the host alone
// with -fsanitize=address,undefined and run on a machine without a GPU (tests/test_closed_map_frontier_host.py does).  No HIP in
// here.  Prints "ok <checks>" and exits 0 when every check holds.
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
        CHECK(tlt::make_box(n, kGiB, tlt::kFrontCellsBelow, &B));
        CHECK(B.n[0] == x && B.n[1] == y && B.n[2] == z && B.cells == (uint64_t)(x * y * z));
        CHECK(B.tiles[0] == up(x, tlt::kTileX) && B.tiles[1] == up(y, tlt::kTileY) && B.tiles[2] == up(z, tlt::kTileZ));
        CHECK(B.ntiles == (uint64_t)(B.tiles[0] * B.tiles[1] * B.tiles[2]) && B.bytes == 4 * B.cells + 8 * B.ntiles);
        for (int a = 0; a < 3; ++a) {
          const int64_t tile = a == 0 ? tlt::kTileX : a == 1 ? tlt::kTileY : tlt::kTileZ;
          CHECK(B.tiles[a] * tile >= n[a] && (B.tiles[a] - 1) * tile < n[a]);   // the last tile holds at least one cell
        }
        // exactly the bytes it needs, and one less
        CHECK(tlt::make_box(n, (int64_t)B.bytes, tlt::kFrontCellsBelow, &B));
        tlt::TileBox C;
        CHECK(!tlt::make_box(n, (int64_t)B.bytes - 1, tlt::kFrontCellsBelow, &C));
      }
  const int64_t wall[3] = {76, 56, 56};
  CHECK(tlt::make_box(wall, kGiB, tlt::kFrontCellsBelow, &B) && B.tiles[0] == 3 && B.tiles[1] == 7 && B.tiles[2] == 14 && B.bytes == 4 * 238336 + 8 * 294);
  const int64_t layer[3] = {76, 56, 1};
  CHECK(tlt::make_box(layer, kGiB, tlt::kFrontCellsBelow, &B) && B.ntiles == 21 && B.bytes == 4 * 4256 + 8 * 21);
}

void check_refusals() {
  tlt::TileBox B;
  const int64_t one[3] = {4, 4, 4};
  for (int64_t bad : {(int64_t)0, (int64_t)-1, (int64_t)3, std::numeric_limits<int64_t>::min()}) CHECK(!tlt::make_box(one, bad, tlt::kFrontCellsBelow, &B));
  CHECK(tlt::make_box(one, 4 * 64 + 8, tlt::kFrontCellsBelow, &B) && !tlt::make_box(one, 4 * 64 + 7, tlt::kFrontCellsBelow, &B));
  const int64_t single[3] = {1, 1, 1};
  CHECK(!tlt::make_box(single, 4, tlt::kFrontCellsBelow, &B) && !tlt::make_box(single, 11, tlt::kFrontCellsBelow, &B) && tlt::make_box(single, 12, tlt::kFrontCellsBelow, &B) && B.bytes == 12);
  for (int a = 0; a < 3; ++a)
    for (int64_t bad : {(int64_t)0, (int64_t)-4, ((int64_t)1 << 21) + 1, kMost}) {
      int64_t n[3] = {8, 8, 8};
      n[a] = bad;
      CHECK(!tlt::make_box(n, kMost, tlt::kFrontCellsBelow, &B));
    }
  // the largest sides: every product would overflow 64 bits if it were formed unchecked
  const int64_t huge[3] = {(int64_t)1 << 21, (int64_t)1 << 21, (int64_t)1 << 21};
  CHECK(!tlt::make_box(huge, kGiB, tlt::kFrontCellsBelow, &B) && !tlt::make_box(huge, kMost, tlt::kFrontCellsBelow, &B));
  // cells >= 0xFFFFFFFC: 4 294 967 292 cells is the first count refused, whatever max_bytes allows
  CHECK(tlt::kFrontOutside == 4294967292ull && tlt::kFrontCellsBelow == tlt::kFrontOutside);
  const int64_t under[3] = {(int64_t)1 << 21, 2047, 1};         // 4 292 870 144 cells: under the bound
  CHECK(tlt::make_box(under, kMost, tlt::kFrontCellsBelow, &B) && B.cells == 4292870144ull && B.cells < tlt::kFrontOutside);
  const int64_t at[3] = {(int64_t)1 << 21, 2048, 1};            // 2^32 cells: over it
  CHECK(!tlt::make_box(at, kMost, tlt::kFrontCellsBelow, &B));
  const int64_t just[3] = {1073741823, 4, 1};                   // (a side beyond 2^21: refused for that alone)
  CHECK(!tlt::make_box(just, kMost, tlt::kFrontCellsBelow, &B));
  const int64_t cube[3] = {2048, 2048, 1023};                   // 4 290 772 992: under
  CHECK(tlt::make_box(cube, kMost, tlt::kFrontCellsBelow, &B));
  const int64_t cube1[3] = {2048, 2048, 1024};                  // 2^32: over
  CHECK(!tlt::make_box(cube1, kMost, tlt::kFrontCellsBelow, &B));
  // under 1 GiB the bound cannot bind: the bytes bind first
  const int64_t gib[3] = {1024, 1024, 256};
  CHECK(!tlt::make_box(gib, kGiB, tlt::kFrontCellsBelow, &B) && tlt::make_box(gib, kGiB + 8 * 32 * 128 * 64, tlt::kFrontCellsBelow, &B));
}

void check_table() {
  uint64_t t = 7;
  CHECK(tlt::kClusterBytes == 136);
  CHECK(tlt::table_room(0, 0, 0, &t) && t == 0);
  CHECK(tlt::table_room(0, 100, 100, &t) && t == 0);
  t = 7;
  CHECK(!tlt::table_room(0, 101, 100, &t) && !tlt::table_room(1, 0, -1, &t) && !tlt::table_room(1, 0, std::numeric_limits<int64_t>::min(), &t) && t == 7);
  for (uint64_t field : {(uint64_t)0, (uint64_t)12, (uint64_t)(4 * 238336 + 8 * 294), (uint64_t)kGiB - 136})
    for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)1025, (uint64_t)100000}) {
      const uint64_t need = field + 136 * k;
      CHECK(tlt::table_room(k, field, (int64_t)need, &t) && t == 136 * k);
      CHECK(!tlt::table_room(k, field, (int64_t)need - 1, &t));
      CHECK(tlt::table_room(k, field, kGiB, &t) == (need <= (uint64_t)kGiB));
    }
  // counts whose product overflows 64 bits are refused, never formed
  const uint64_t big = std::numeric_limits<uint64_t>::max();
  CHECK(!tlt::table_room(big, 0, kMost, &t) && !tlt::table_room(big / 2, 0, kMost, &t) && !tlt::table_room(big / 136 + 1, 0, kMost, &t));
  CHECK(tlt::table_room((uint64_t)kMost / 136, 0, kMost, &t) && t == ((uint64_t)kMost / 136) * 136);
  CHECK(!tlt::table_room((uint64_t)kMost / 136 + 1, 0, kMost, &t));
}

}  // namespace

int main() {
  check_tiles();
  check_refusals();
  check_table();
  printf("ok %d\n", checks);
  return 0;
}
