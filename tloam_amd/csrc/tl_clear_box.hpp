// tl_clear_box.hpp -- the host arithmetic of the clearance field (tl_api_clear.hip): the truncation radius
// in cells, the squared radius a segment check needs, and the field's cell and byte counts over a box of bricks, every product
// checked before it is trusted.  No HIP and no context in here, so that a stand-alone program can drive it under the host
// sanitizers (tests/host/clear_box_main.cpp), as tl_free_box.hpp.
#pragma once

#include <math.h>
#include <stdint.h>

namespace tlc {

constexpr int kMaxRadius = 128;   // 3 * 128^2 = 49 152 < 0xFFFE: every sum inside the passes fits 16 bits beside the two sentinels

// R = (int) ceil(max_distance / voxel), in double.  false: the quotient is not finite or R is outside 1 .. kMaxRadius
inline bool radius_cells(double max_distance, double voxel, int* R) {
  const double r = ceil(max_distance / voxel);
  if (!(r >= 1.0 && r <= (double)kMaxRadius)) return false;   // (a NaN fails both)
  *R = (int)r;
  return true;
}

// need = (int64) ceil(q * q), q = radius / voxel, in double, in that order.  false: radius is not finite or negative, or
// need > R * R + 1 (the field cannot vouch for more than R cells)
inline bool need_d2(double radius, double voxel, int R, int64_t* need) {
  if (!(radius - radius == 0.0) || radius < 0.0) return false;
  const double q = radius / voxel;
  const double n = ceil(q * q);
  const double most = (double)((int64_t)R * R + 1);
  if (!(n <= most)) return false;   // (an overflowed square fails here)
  *need = (int64_t)n;
  return true;
}

struct ClearBox {
  int64_t n[3];      // cells per axis: 4 * nb
  uint64_t cells;    // n[0] * n[1] * n[2]
  uint64_t bytes;    // 2 buffers * 2 bytes * cells
};

// The field over nb[] bricks per axis (each in [1, 2^19], as tlf::make_box leaves them).  false: a count out of that range, a
// product that overflows, or more than max_bytes bytes for the two buffers; *out is then not to be used.
inline bool make_field(const int64_t nb[3], int64_t max_bytes, ClearBox* out) {
  for (int a = 0; a < 3; ++a) {
    if (nb[a] < 1 || nb[a] > ((int64_t)1 << 19)) return false;
    out->n[a] = 4 * nb[a];   // <= 2^21
  }
  if (max_bytes < 2) return false;
  const uint64_t cap_cells = (uint64_t)max_bytes / 4u;   // two buffers of two bytes a cell
  // n[a] <= 2^21: the product of two fits 42 bits; the third is checked by division before it is formed
  const uint64_t plane = (uint64_t)out->n[0] * (uint64_t)out->n[1];
  if (plane > cap_cells || (uint64_t)out->n[2] > cap_cells / plane) return false;
  out->cells = plane * (uint64_t)out->n[2];   // <= cap_cells < 2^61
  out->bytes = out->cells * 4u;
  return true;
}

}  // namespace tlc
