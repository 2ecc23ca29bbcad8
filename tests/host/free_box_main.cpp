// A stand-alone driver of the free-space grid's host arithmetic (tloam_amd/csrc/tl_free_box.hpp: the auto box over the poses, a
// box of cells rounded out to bricks, the brick counts and the byte size with every product checked, the band of z cells),
// meant to be compiled for the host alone with -fsanitize=address,undefined and run on a machine without a GPU
// (tests/test_closed_map_free_host.py does).  No HIP in here.
// Prints "ok <checks>" and exits 0 when every check holds.
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "../../tloam_amd/csrc/tl_free_box.hpp"

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

const int64_t kLim = tlf::kCellLimit;

std::vector<double> poses_at(const std::vector<double>& xyz) {
  std::vector<double> P(16 * (xyz.size() / 3), 0.0);
  for (size_t k = 0; k < xyz.size() / 3; ++k) {
    for (int i = 0; i < 4; ++i) P[16 * k + 5 * i] = 1.0;
    for (int a = 0; a < 3; ++a) P[16 * k + 12 + a] = xyz[3 * k + a];
  }
  return P;
}

void check_bricks() {
  // the brick of a cell floors: every cell of a brick gives it, negative ones too
  for (int64_t c = -4100; c <= 4100; ++c) {
    const int64_t b = tlf::brick_of(c);
    CHECK(4 * b <= c && c <= 4 * b + 3);
  }
  CHECK(tlf::brick_of(-kLim + 1) == -(kLim / 4) && tlf::brick_of(kLim - 1) == kLim / 4 - 1);
}

void check_make_box() {
  tlf::FreeBox B;
  const int64_t big = (int64_t)1 << 40;
  {
    const int64_t lo[3] = {-5, -1, 3}, hi[3] = {2, 0, 3};
    CHECK(tlf::make_box(lo, hi, big, &B));
    CHECK(B.blo[0] == -2 && B.blo[1] == -1 && B.blo[2] == 0 && B.nb[0] == 3 && B.nb[1] == 2 && B.nb[2] == 1);
    CHECK(B.words == 6 && B.bytes == 48);
    CHECK(tlf::make_box(lo, hi, 48, &B) && !tlf::make_box(lo, hi, 47, &B) && !tlf::make_box(lo, hi, 0, &B));
    CHECK(!tlf::make_box(lo, hi, -1, &B) && !tlf::make_box(lo, hi, std::numeric_limits<int64_t>::min(), &B));
  }
  // every box of a small range against the definition
  for (int64_t l = -9; l <= 9; ++l)
    for (int64_t h = -9; h <= 9; ++h) {
      const int64_t lo[3] = {l, 0, -3}, hi[3] = {h, 0, 3};
      const bool ok = tlf::make_box(lo, hi, big, &B);
      CHECK(ok == (l <= h));
      if (!ok) continue;
      CHECK(4 * B.blo[0] <= l && l <= 4 * B.blo[0] + 3);
      const int64_t top = 4 * (B.blo[0] + B.nb[0]) - 1;
      CHECK(top - 3 <= h && h <= top);
      CHECK(B.nb[1] == 1 && B.nb[2] == 2 && B.words == (uint64_t)(2 * B.nb[0]) && B.bytes == 8 * B.words);
    }
  // the grid's limits: |c| < 2^20
  {
    const int64_t lo[3] = {-kLim + 1, 0, 0}, hi[3] = {kLim - 1, 0, 0};
    CHECK(tlf::make_box(lo, hi, big, &B) && B.nb[0] == kLim / 2 && B.words == (uint64_t)(kLim / 2));
    const int64_t lo2[3] = {-kLim, 0, 0}, hi2[3] = {0, kLim, 0};
    CHECK(!tlf::make_box(lo2, hi, big, &B) && !tlf::make_box(lo, hi2, big, &B));
    const int64_t far_lo[3] = {std::numeric_limits<int64_t>::min(), 0, 0}, far_hi[3] = {std::numeric_limits<int64_t>::max(), 0, 0};
    CHECK(!tlf::make_box(far_lo, hi, big, &B) && !tlf::make_box(lo, far_hi, big, &B) && !tlf::make_box(far_lo, far_hi, big, &B));
  }
  // the whole grid: 2^57 words, refused by any max_bytes that is an int64 of bytes below 2^60; never an overflow
  {
    const int64_t lo[3] = {-kLim + 1, -kLim + 1, -kLim + 1}, hi[3] = {kLim - 1, kLim - 1, kLim - 1};
    CHECK(!tlf::make_box(lo, hi, (int64_t)1 << 30, &B));
    CHECK(!tlf::make_box(lo, hi, ((int64_t)1 << 60) - 1, &B));
    CHECK(tlf::make_box(lo, hi, std::numeric_limits<int64_t>::max(), &B) && B.words == (uint64_t)1 << 57 && B.bytes == (uint64_t)1 << 60);
    const int64_t hi2[3] = {kLim - 1, kLim - 1, -kLim + 1};   // a plane of 2^38 words
    CHECK(!tlf::make_box(lo, hi2, ((int64_t)1 << 41) - 1, &B) && tlf::make_box(lo, hi2, (int64_t)1 << 41, &B) && B.words == (uint64_t)1 << 38);
  }
}

void check_auto_box() {
  int64_t lo[3], hi[3];
  const double o[3] = {0.0, 0.0, 0.0};
  tlf::auto_box(nullptr, 0, o, 0.5, 60.0, lo, hi);
  for (int a = 0; a < 3; ++a) CHECK(lo[a] == 0 && hi[a] == 0);
  // the wall scene's poses span x 2 .. 10 at y 0, z 1.5 or so: R = ceil(12 / 0.5) + 1 = 25
  const std::vector<double> P = poses_at({2.0, 0.0, 1.5, 10.0, 0.0, 1.5, 6.0, -0.25, 1.5});
  tlf::auto_box(P.data(), 3, o, 0.5, 12.0, lo, hi);
  CHECK(lo[0] == 4 - 25 && hi[0] == 20 + 25 && lo[1] == -1 - 25 && hi[1] == 0 + 25 && lo[2] == 3 - 25 && hi[2] == 3 + 25);
  const double o2[3] = {100.0, -7.25, 0.125};
  tlf::auto_box(P.data(), 3, o2, 0.25, 1.0, lo, hi);   // R = 5; every cell negative on x
  CHECK(lo[0] == -392 - 5 && hi[0] == -360 + 5 && lo[1] == 28 - 5 && hi[1] == 29 + 5 && lo[2] == 5 - 5 && hi[2] == 5 + 5);
  // clamped: a tiny voxel, a huge range, poses far away; never a cast of a value out of range
  tlf::auto_box(P.data(), 3, o, 1e-300, 60.0, lo, hi);   // (the poses' own cells are beyond the clamp: x and z above it)
  CHECK(lo[0] == kLim - 1 && hi[0] == kLim - 1 && lo[1] == -kLim + 1 && hi[1] == kLim - 1 && lo[2] == kLim - 1 && hi[2] == kLim - 1);
  const double cases[][2] = {{1e-5, 60.0}, {0.5, 1e300}, {0.5, std::numeric_limits<double>::infinity()},
                             {0.5, std::numeric_limits<double>::quiet_NaN()}};
  for (const auto& cs : cases) {
    tlf::auto_box(P.data(), 3, o, cs[0], cs[1], lo, hi);
    for (int a = 0; a < 3; ++a) CHECK(lo[a] == -kLim + 1 && hi[a] == kLim - 1);
  }
  const std::vector<double> far = poses_at({1e300, -1e300, std::numeric_limits<double>::infinity()});
  tlf::auto_box(far.data(), 1, o, 0.5, 12.0, lo, hi);
  CHECK(lo[0] == kLim - 1 && hi[0] == kLim - 1 && lo[1] == -kLim + 1 && hi[1] == -kLim + 1 && lo[2] == kLim - 1 && hi[2] == kLim - 1);
  const std::vector<double> nan = poses_at({std::numeric_limits<double>::quiet_NaN(), 0.0, 0.0});
  tlf::auto_box(nan.data(), 1, o, 0.5, 12.0, lo, hi);
  CHECK(lo[0] >= -kLim + 1 && hi[0] <= kLim - 1);
  // whatever the auto box gives is a box make_box takes (when the bytes allow it)
  tlf::FreeBox B;
  tlf::auto_box(P.data(), 3, o, 0.5, 12.0, lo, hi);
  CHECK(tlf::make_box(lo, hi, (int64_t)1 << 30, &B) && B.nb[0] == 18 && B.nb[1] == 14 && B.nb[2] == 14 && B.bytes == 8u * 18 * 14 * 14);
}

void check_z_band() {
  int64_t z0, z1;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(tlf::z_band(0.5, 2.9, 0.0, 0.5, -6, 14, &z0, &z1) && z0 == 1 && z1 == 5);
  CHECK(tlf::z_band(-1e9, 1e9, 0.0, 0.5, -6, 14, &z0, &z1) && z0 == -24 && z1 == 31);
  CHECK(tlf::z_band(-1e308, 1e308, 0.0, 1e-300, -6, 14, &z0, &z1) && z0 == -24 && z1 == 31);   // the quotients overflow
  CHECK(tlf::z_band(100.0, 200.0, 0.0, 0.5, -6, 14, &z0, &z1) && z0 > z1);
  CHECK(tlf::z_band(-200.0, -100.0, 0.0, 0.5, -6, 14, &z0, &z1) && z0 > z1);
  CHECK(tlf::z_band(1e308, 1e308, 0.0, 1e-300, -6, 14, &z0, &z1) && z0 > z1);
  CHECK(tlf::z_band(1.0, 1.0, 0.0, 0.5, -6, 14, &z0, &z1) && z0 == 2 && z1 == 2);
  CHECK(tlf::z_band(-0.25, -0.25, 0.0, 0.5, -6, 14, &z0, &z1) && z0 == -1 && z1 == -1);
  CHECK(!tlf::z_band(2.0, 1.0, 0.0, 0.5, -6, 14, &z0, &z1));
  CHECK(!tlf::z_band(nan, 1.0, 0.0, 0.5, -6, 14, &z0, &z1) && !tlf::z_band(0.0, nan, 0.0, 0.5, -6, 14, &z0, &z1));
  CHECK(!tlf::z_band(-inf, 1.0, 0.0, 0.5, -6, 14, &z0, &z1) && !tlf::z_band(0.0, inf, 0.0, 0.5, -6, 14, &z0, &z1));
  // at the grid's limits
  CHECK(tlf::z_band(-1e9, 1e9, 0.0, 0.5, -kLim / 4, kLim / 2, &z0, &z1) && z0 == -kLim && z1 == kLim - 1);
}

}  // namespace

int main() {
  check_bricks();
  check_make_box();
  check_auto_box();
  check_z_band();
  printf("ok %d\n", checks);
  return 0;
}
