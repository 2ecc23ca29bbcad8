// A stand-alone driver of the clearance field's host arithmetic (tloam_amd/csrc/tl_clear_box.hpp: the truncation radius in
// cells, the squared radius a segment check needs, the field's cell and byte counts with every product checked), meant to be
// compiled for the host alone with -fsanitize=address,undefined and run on a machine without a GPU
// (tests/test_closed_map_clearance_host.py does).  No HIP in here.
// Prints "ok <checks>" and exits 0 when every check holds.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <limits>

#include "../../tloam_amd/csrc/tl_clear_box.hpp"

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

const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

void check_radius() {
  int R = -7;
  // on an integer, and just off it on either side
  for (int k = 1; k <= tlc::kMaxRadius; ++k)
    for (double v : {0.5, 0.25, 1.0, 0.1, 0.3}) {
      const double on = (double)k * v;
      CHECK(tlc::radius_cells(on, v, &R) && R == (int)ceil(on / v) && (R == k || R == k + 1));   // (k * 0.1 / 0.1 may round up)
      const double below = nextafter(on, 0.0);
      CHECK(tlc::radius_cells(below, v, &R) && R == (int)ceil(below / v) && R >= k - 1 && R <= k + 1);
      const double above = nextafter(on, kInf);
      const double q = ceil(above / v);
      CHECK(tlc::radius_cells(above, v, &R) == (q <= (double)tlc::kMaxRadius) && (q > (double)tlc::kMaxRadius || R == (int)q));
    }
  CHECK(tlc::radius_cells(4.0, 0.5, &R) && R == 8);
  CHECK(tlc::radius_cells(nextafter(4.0, kInf), 0.5, &R) && R == 9);
  CHECK(tlc::radius_cells(nextafter(4.0, 0.0), 0.5, &R) && R == 8);
  CHECK(tlc::radius_cells(1e-300, 0.5, &R) && R == 1);
  CHECK(tlc::radius_cells(64.0, 0.5, &R) && R == 128);
  R = -7;
  CHECK(!tlc::radius_cells(nextafter(64.0, kInf), 0.5, &R) && !tlc::radius_cells(0.0, 0.5, &R) && !tlc::radius_cells(-1.0, 0.5, &R));
  CHECK(!tlc::radius_cells(kInf, 0.5, &R) && !tlc::radius_cells(kNaN, 0.5, &R) && !tlc::radius_cells(1e300, 1e-300, &R));
  CHECK(!tlc::radius_cells(4.0, 0.0, &R) && !tlc::radius_cells(4.0, kNaN, &R) && !tlc::radius_cells(0.0, 0.0, &R));
  CHECK(R == -7);   // a refusal writes nothing
}

void check_need() {
  int64_t need = -7;
  // radius at exactly k cells: need = k * k; just above: k * k + 1; just below: k * k
  for (int k = 0; k <= 8; ++k) {
    const double on = 0.5 * (double)k;
    CHECK(tlc::need_d2(on, 0.5, 8, &need) && need == (int64_t)k * k);
    if (k > 0) CHECK(tlc::need_d2(nextafter(on, 0.0), 0.5, 8, &need) && need == (int64_t)k * k);
    if (k > 0) CHECK(tlc::need_d2(nextafter(on, kInf), 0.5, 8, &need) && need == (int64_t)k * k + 1);   // (k = 8: 65 = R * R + 1, the most)
  }
  CHECK(tlc::need_d2(nextafter(0.0, kInf), 0.5, 8, &need) && need == 0);   // (the square of a denormal quotient is 0)
  CHECK(tlc::need_d2(1e-150, 0.5, 8, &need) && need == 1);
  CHECK(tlc::need_d2(0.0, 0.5, 1, &need) && need == 0);
  CHECK(tlc::need_d2(1.25, 0.5, 8, &need) && need == 7);
  for (int R = 1; R <= tlc::kMaxRadius; ++R) {
    CHECK(tlc::need_d2((double)R, 1.0, R, &need) && need == (int64_t)R * R);
    need = -7;
    CHECK(!tlc::need_d2((double)R + 1.0, 1.0, R, &need) && need == -7);   // a refusal writes nothing
  }
  CHECK(!tlc::need_d2(-0.0 - 1e-300, 0.5, 8, &need) && !tlc::need_d2(kNaN, 0.5, 8, &need) && !tlc::need_d2(kInf, 0.5, 8, &need));
  CHECK(!tlc::need_d2(1e200, 1e-200, 128, &need) && !tlc::need_d2(1.0, 0.0, 8, &need) && !tlc::need_d2(0.0, 0.0, 8, &need));
  CHECK(tlc::need_d2(-0.0, 0.5, 8, &need) && need == 0);
}

void check_field() {
  tlc::ClearBox B;
  const int64_t big = std::numeric_limits<int64_t>::max();
  {
    const int64_t nb[3] = {19, 14, 14};
    CHECK(tlc::make_field(nb, big, &B) && B.n[0] == 76 && B.n[1] == 56 && B.n[2] == 56 && B.cells == 238336 && B.bytes == 953344);
    CHECK(tlc::make_field(nb, 953344, &B) && !tlc::make_field(nb, 953343, &B));
  }
  {
    const int64_t nb[3] = {1, 1, 1};
    CHECK(tlc::make_field(nb, 256, &B) && B.cells == 64 && B.bytes == 256 && !tlc::make_field(nb, 255, &B));
    CHECK(!tlc::make_field(nb, 1, &B) && !tlc::make_field(nb, 0, &B) && !tlc::make_field(nb, -1, &B));
    CHECK(!tlc::make_field(nb, std::numeric_limits<int64_t>::min(), &B));
  }
  // every small shape against the definition
  for (int64_t a = 1; a <= 6; ++a)
    for (int64_t b = 1; b <= 6; ++b)
      for (int64_t c = 1; c <= 6; ++c) {
        const int64_t nb[3] = {a, b, c};
        const int64_t bytes = 4 * 64 * a * b * c;
        CHECK(tlc::make_field(nb, bytes, &B) && (int64_t)B.bytes == bytes && (int64_t)B.cells == 64 * a * b * c);
        CHECK(!tlc::make_field(nb, bytes - 1, &B));
      }
  // the grid's limits: 2^19 bricks an axis, 2^63 cells in all: no product is formed before it is known to fit
  const int64_t top = (int64_t)1 << 19;
  {
    const int64_t nb[3] = {top, top, top};
    CHECK(!tlc::make_field(nb, big, &B));
    const int64_t line[3] = {top, 1, 1}, plane[3] = {top, top, 1}, slab[3] = {top, top, 64};
    CHECK(tlc::make_field(line, big, &B) && B.n[0] == 4 * top && B.cells == (uint64_t)top * 64);
    CHECK(tlc::make_field(plane, big, &B) && B.cells == (uint64_t)top * top * 64 && B.bytes == B.cells * 4);
    CHECK(tlc::make_field(slab, big, &B) && B.cells == ((uint64_t)1 << 50) && B.bytes == ((uint64_t)1 << 52));
    const int64_t most[3] = {top, top, (int64_t)1 << 15};   // 2^59 cells, 2^61 bytes: fits; twice that does not
    CHECK(tlc::make_field(most, big, &B) && B.bytes == ((uint64_t)1 << 61));
    const int64_t over[3] = {top, top, (int64_t)1 << 17};
    CHECK(!tlc::make_field(over, big, &B));
    CHECK(!tlc::make_field(plane, ((int64_t)1 << 46) - 1, &B) && tlc::make_field(plane, (int64_t)1 << 46, &B));
  }
  for (int a = 0; a < 3; ++a) {
    int64_t nb[3] = {2, 2, 2};
    nb[a] = 0;
    CHECK(!tlc::make_field(nb, big, &B));
    nb[a] = -3;
    CHECK(!tlc::make_field(nb, big, &B));
    nb[a] = top + 1;
    CHECK(!tlc::make_field(nb, big, &B));
    nb[a] = std::numeric_limits<int64_t>::max();
    CHECK(!tlc::make_field(nb, big, &B));
    nb[a] = std::numeric_limits<int64_t>::min();
    CHECK(!tlc::make_field(nb, big, &B));
  }
}

}  // namespace

int main() {
  check_radius();
  check_need();
  check_field();
  printf("ok %d\n", checks);
  return 0;
}
