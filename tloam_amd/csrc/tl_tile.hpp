// tl_tile.hpp -- the tile-round engine of the dense uint32 fields (TileField: the route's costs, tl_route.hip, DESIGN.md section
// 31; the frontiers' labels, tl_frontier.hip, section 32; the engine itself: section 31.1): a field's index arithmetic and one
// round of a monotone min-fixpoint over it, as a device function each field's kernel wraps with its policy.  Device code; the
// host side of the rounds is tl_ctx.hpp's tile_rounds, the box arithmetic tl_tile_box.hpp.
//
// One round (tile_round<P>, tiles x 256): a block per tile of 32 x 8 x 4 cells, gone at once when its flag in `now` is down.
// Else the tile and a halo of one cell (34 x 10 x 6 words, 8160 bytes) are staged in LDS, every sentinel (a word >= P::kSentinel)
// and what is outside the box as P::kNothing; a thread owns the four cells of a column along z and keeps which of them may fall
// in a register mask.  It relaxes them in place, min(neighbour + P::weight(steps)) over the 26 neighbours, until a block-wide vote
// says nothing fell or P::kPasses passes are done; on the cap the tile flags itself for the next round.  Only cells that fell
// are written back; each neighbouring tile that holds a cell next to one that fell is flagged in `next` (an atomic OR: a flag
// found down is a fresh mark) and the fresh marks are added to the round's counter, one atomic a block.
//
// Why any schedule gives the same bytes: a cell's value only ever falls, and only to some neighbour's value + w; the policy's
// operator is monotone and bounded below (each field's file says why), so no value goes below the least fixpoint.  A halo value
// read while its owner lowers it may be old; it is then an upper bound, and the owner's mark runs the reader again in the next
// round, after the kernel boundary has made the new value visible.  The host stops when a round marked nothing: no cell can be
// lowered, which is the fixpoint, and the least fixpoint of a monotone min operator from one start is unique.  No block waits on
// another: no spin, no grid barrier.  All integer: no floating-point atomics, no run-time indexed private arrays, no scratch.
//
// A policy P gives:
//   kNothing   what stands in LDS for a sentinel and for outside the box: kNothing + weight does not wrap, min never takes it
//   kSentinel  a field word at or above it is a sentinel
//   kPasses    passes over a tile in LDS before it hands itself to the next round
//   weight(steps)  constexpr: what a move along `steps` (1 .. 3) axes adds
//   kLiveFromField, kDead  true: a cell may fall when its word in the field is not kDead, read from the thread's own four words
//              before the first barrier; false: when its word in LDS is not kNothing (kDead is then not asked for)
#pragma once

#include "tl_common.hpp"
#include "tl_tile_box.hpp"

namespace tl {

constexpr int kTX = tlt::kTileX, kTY = tlt::kTileY, kTZ = tlt::kTileZ;
constexpr int kHX = kTX + 2, kHY = kTY + 2, kHZ = kTZ + 2, kHalo = kHX * kHY * kHZ;
static_assert(kTX * kTY == 256 && kTZ == 4, "a thread per column of four cells");

// the index of cell (cx, cy, cz) in the field, -1 outside the box
__device__ __forceinline__ long long tile_index(const TileField& f, int cx, int cy, int cz) {
  const unsigned x = (unsigned)(cx - f.lo[0]), y = (unsigned)(cy - f.lo[1]), z = (unsigned)(cz - f.lo[2]);
  if (!(x < (unsigned)f.n[0] && y < (unsigned)f.n[1] && z < (unsigned)f.n[2])) return -1;
  return ((long long)z * f.n[1] + (long long)y) * f.n[0] + (long long)x;
}
// index -> box-local (x, y, z)
__device__ __forceinline__ void tile_xyz(const TileField& f, long long idx, int* x, int* y, int* z) {
  const long long row = idx / f.n[0];
  *x = (int)(idx - row * f.n[0]);
  *z = (int)(row / f.n[1]);
  *y = (int)(row - (long long)*z * f.n[1]);
}
// the tile of the box-local cell (x, y, z)
__device__ __forceinline__ long long tile_of(const TileField& f, int x, int y, int z) {
  return ((long long)(z / kTZ) * f.tiles[1] + y / kTY) * f.tiles[0] + x / kTX;
}

// min(cur, neighbour + w) over the 26 neighbours of the cell at s[at]
template <class P>
__device__ __forceinline__ unsigned relax_cell(const unsigned* s, int at, unsigned cur) {
  unsigned best = cur;
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dz == 0 && dy == 0 && dx == 0) continue;
        best = min(best, s[at + (dz * kHY + dy) * kHX + dx] + P::weight((dz != 0) + (dy != 0) + (dx != 0)));
      }
  return best;
}

// the neighbouring tiles, as bits dz * 9 + dy * 3 + dx of (-1, 0, 1) + 1 each, that hold a cell next to cell (x, y, z) of a tile
__device__ __forceinline__ unsigned tiles_next_to(int x, int y, int z) {
  const unsigned ax = (x == 0 ? 1u : 0u) | 2u | (x == kTX - 1 ? 4u : 0u);
  const unsigned ay = (y == 0 ? 1u : 0u) | 2u | (y == kTY - 1 ? 4u : 0u);
  const unsigned az = (z == 0 ? 1u : 0u) | 2u | (z == kTZ - 1 ? 4u : 0u);
  const unsigned m9 = (ay & 1u ? ax : 0u) | (ax << 3) | (ay & 4u ? ax << 6 : 0u);
  return (az & 1u ? m9 : 0u) | (m9 << 9) | (az & 4u ? m9 << 18 : 0u);
}

// One round, as the head of this file states it.  Called by the whole block of 256 threads, blockIdx.x the tile.
template <class P>
__device__ __forceinline__ void tile_round(const TileField& f, unsigned* __restrict__ now, unsigned* __restrict__ next,
                                           unsigned long long* __restrict__ marks) {
  __shared__ unsigned s[kHalo];
  __shared__ unsigned s_mask;
  const long long tile = blockIdx.x;
  if (now[tile] == 0u) return;   // (the block's own flag: nobody writes it in this launch before the barrier below)
  const int tx = (int)(tile % f.tiles[0]);
  const long long rest = tile / f.tiles[0];
  const int ty = (int)(rest % f.tiles[1]), tz = (int)(rest / f.tiles[1]);
  const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ;
  for (int i = threadIdx.x; i < kHalo; i += 256) {
    const int lx = i % kHX, r = i / kHX, ly = r % kHY, lz = r / kHY;
    const int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = z0 + lz - 1;
    unsigned v = P::kNothing;
    if ((unsigned)gx < (unsigned)f.n[0] && (unsigned)gy < (unsigned)f.n[1] && (unsigned)gz < (unsigned)f.n[2]) {
      v = f.v[((long long)gz * f.n[1] + gy) * f.n[0] + gx];
      if (v >= P::kSentinel) v = P::kNothing;
    }
    s[i] = v;
  }
  if (threadIdx.x == 0) s_mask = 0u;
  // this thread's column: the cells (x, y, 0 .. 3) of the tile; `live`: which of them may fall
  const int x = threadIdx.x & (kTX - 1), y = threadIdx.x >> 5;
  const int gx = x0 + x, gy = y0 + y;
  const long long plane = (long long)f.n[0] * f.n[1];
  const long long g0 = ((long long)z0 * f.n[1] + gy) * f.n[0] + gx;
  unsigned live = 0u;
  if constexpr (P::kLiveFromField) {
    if (gx < f.n[0] && gy < f.n[1]) {
      if (z0 + 0 < f.n[2] && f.v[g0] != P::kDead) live |= 1u;
      if (z0 + 1 < f.n[2] && f.v[g0 + plane] != P::kDead) live |= 2u;
      if (z0 + 2 < f.n[2] && f.v[g0 + 2 * plane] != P::kDead) live |= 4u;
      if (z0 + 3 < f.n[2] && f.v[g0 + 3 * plane] != P::kDead) live |= 8u;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) now[tile] = 0u;   // taken down: the array is all zero when it becomes `next`
  constexpr int kLayer = kHY * kHX;
  const int at = (kHY + y + 1) * kHX + x + 1;   // the column's cell z = 0 in the halo
  const unsigned o0 = s[at], o1 = s[at + kLayer], o2 = s[at + 2 * kLayer], o3 = s[at + 3 * kLayer];
  if constexpr (!P::kLiveFromField)   // (what is outside the box is kNothing too)
    live = (o0 != P::kNothing ? 1u : 0u) | (o1 != P::kNothing ? 2u : 0u) | (o2 != P::kNothing ? 4u : 0u) | (o3 != P::kNothing ? 8u : 0u);
  unsigned c0 = o0, c1 = o1, c2 = o2, c3 = o3;
  int again = 0;
  for (int it = 0; it < P::kPasses; ++it) {
    int fell = 0;
    // in place: a neighbour read while its owner writes it is the old or the new value, both upper bounds
    if (live & 1u) { const unsigned b = relax_cell<P>(s, at, c0); if (b < c0) { c0 = b; s[at] = b; fell = 1; } }
    if (live & 2u) { const unsigned b = relax_cell<P>(s, at + kLayer, c1); if (b < c1) { c1 = b; s[at + kLayer] = b; fell = 1; } }
    if (live & 4u) { const unsigned b = relax_cell<P>(s, at + 2 * kLayer, c2); if (b < c2) { c2 = b; s[at + 2 * kLayer] = b; fell = 1; } }
    if (live & 8u) { const unsigned b = relax_cell<P>(s, at + 3 * kLayer, c3); if (b < c3) { c3 = b; s[at + 3 * kLayer] = b; fell = 1; } }
    again = __syncthreads_or(fell);
    if (!again) break;
  }
  unsigned m = 0u;
  if (c0 < o0) { f.v[g0] = c0; m |= tiles_next_to(x, y, 0); }
  if (c1 < o1) { f.v[g0 + plane] = c1; m |= tiles_next_to(x, y, 1); }
  if (c2 < o2) { f.v[g0 + 2 * plane] = c2; m |= tiles_next_to(x, y, 2); }
  if (c3 < o3) { f.v[g0 + 3 * plane] = c3; m |= tiles_next_to(x, y, 3); }
  m &= ~(1u << 13);                                   // (the tile itself: only the cap below flags it)
  if (again && threadIdx.x == 0) m |= 1u << 13;       // the cap was met with cells still falling
  if (m) atomicOr(&s_mask, m);
  __syncthreads();
  if (threadIdx.x < 64) {                             // the first wave: a lane per direction
    bool fresh = false;
    const int d = threadIdx.x;
    if (d < 27 && (s_mask >> d & 1u)) {
      const int nx = tx + d % 3 - 1, ny = ty + d / 3 % 3 - 1, nz = tz + d / 9 - 1;
      if ((unsigned)nx < (unsigned)f.tiles[0] && (unsigned)ny < (unsigned)f.tiles[1] && (unsigned)nz < (unsigned)f.tiles[2])
        fresh = atomicOr(&next[((long long)nz * f.tiles[1] + ny) * f.tiles[0] + nx], 1u) == 0u;
    }
    const unsigned long long bal = __ballot(fresh);
    if (threadIdx.x == 0 && bal) atomicAdd(marks, (unsigned long long)__popcll(bal));
  }
}

}  // namespace tl
