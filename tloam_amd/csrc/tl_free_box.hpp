// tl_free_box.hpp -- the host arithmetic of the free-space grid's box (tl_api_free.hip): the auto box over
// the closed map's poses, a box of cells rounded out to bricks, the brick counts and the byte size, every product checked for
// overflow before it is trusted, and the band of z cells of a column read.  No HIP and no context in here, so that a stand-alone
// program can drive it under the host sanitizers (tests/host/free_box_main.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

namespace tlf {

constexpr int64_t kCellLimit = (int64_t)1 << 20;   // a cell of the closed map's grid has |c| < 2^20 on every axis

struct FreeBox {
  int64_t blo[3];       // the lowest brick per axis
  int64_t nb[3];        // bricks per axis
  uint64_t words;       // nb[0] * nb[1] * nb[2]
  uint64_t bytes;       // 8 * words
};

// floor(c / 4) without shifting a negative value
inline int64_t brick_of(int64_t c) { return c >= 0 ? c / 4 : -((-c + 3) / 4); }

// The auto box over K poses (column-major, the translation at [12..14]), in cells, inclusive: per axis c_k = floor((O_k - o) / v),
// R = (int64) ceil(max_range / v) + 1, lo = min c_k - R, hi = max c_k + R, both clamped to +-(2^20 - 1); in double, in that order.
// Without a pose the box is the one cell 0.
inline void auto_box(const double* poses, size_t K, const double origin[3], double voxel, double max_range, int64_t lo[3],
                     int64_t hi[3]) {
  const double limit = (double)(kCellLimit - 1);
  double Rd = ceil(max_range / voxel);
  if (!(Rd < 2.0 * (double)kCellLimit)) Rd = 2.0 * (double)kCellLimit;   // (beyond the clamp either way; NaN too)
  const int64_t R = (int64_t)Rd + 1;
  for (int a = 0; a < 3; ++a) {
    double cmin = 0.0, cmax = 0.0;
    for (size_t k = 0; k < K; ++k) {
      const double ck = floor((poses[16 * k + 12 + a] - origin[a]) / voxel);
      if (k == 0 || ck < cmin) cmin = ck;
      if (k == 0 || ck > cmax) cmax = ck;
    }
    double l = K ? cmin - (double)R : 0.0, h = K ? cmax + (double)R : 0.0;
    if (!(l >= -limit)) l = -limit;   // (a NaN goes to the clamp as well)
    if (!(l <= limit)) l = limit;
    if (!(h <= limit)) h = limit;
    if (!(h >= -limit)) h = -limit;
    lo[a] = (int64_t)l;
    hi[a] = (int64_t)h;
  }
}

// The box of the cells [lo, hi] (inclusive) rounded out to bricks.  false: lo > hi on an axis, a cell beyond the grid
// (|c| >= 2^20), a product that overflows, or more than max_bytes bytes; *out is then not to be used.
inline bool make_box(const int64_t lo[3], const int64_t hi[3], int64_t max_bytes, FreeBox* out) {
  for (int a = 0; a < 3; ++a) {
    if (lo[a] > hi[a] || lo[a] <= -kCellLimit || hi[a] >= kCellLimit) return false;
    out->blo[a] = brick_of(lo[a]);
    out->nb[a] = brick_of(hi[a]) - out->blo[a] + 1;   // in [1, 2^19]
  }
  if (max_bytes < 8) return false;
  const uint64_t cap_words = (uint64_t)max_bytes / 8u;
  // nb[a] <= 2^19: the product of two fits 38 bits; the third is checked by division before it is formed
  const uint64_t plane = (uint64_t)out->nb[0] * (uint64_t)out->nb[1];
  if (plane > cap_words || (uint64_t)out->nb[2] > cap_words / plane) return false;
  out->words = plane * (uint64_t)out->nb[2];   // <= cap_words <= 2^60
  out->bytes = out->words * 8u;
  return true;
}

// The band of z cells floor((z_lo - o) / v) .. floor((z_hi - o) / v) clipped to the box's cells [4 blo, 4 (blo + nb) - 1].
// false: a bound that is not finite, or z_lo > z_hi.  *z0 > *z1: the band misses the box.
inline bool z_band(double z_lo, double z_hi, double origin_z, double voxel, int64_t blo_z, int64_t nb_z, int64_t* z0, int64_t* z1) {
  if (!(z_lo - z_lo == 0.0) || !(z_hi - z_hi == 0.0) || z_lo > z_hi) return false;
  const double box0 = (double)(4 * blo_z), box1 = (double)(4 * (blo_z + nb_z) - 1);
  double a = floor((z_lo - origin_z) / voxel), b = floor((z_hi - origin_z) / voxel);
  if (!(a >= box0)) a = box0;          // (an overflowed quotient is clipped like any other)
  if (!(b <= box1)) b = box1;
  if (a > box1 || b < box0) { *z0 = 1; *z1 = 0; return true; }
  *z0 = (int64_t)a;
  *z1 = (int64_t)b;
  return true;
}

}  // namespace tlf
