// A stand-alone driver of the view gain's host arithmetic (tloam_amd/csrc/tl_view_box.hpp: the side, the bits, the words and the
// bytes of a view's window, which form takes it, the global form's chunks, a launch's blocks, every refusal), meant to be compiled
// for the host alone with -fsanitize=address,undefined and run on a machine without a GPU (tests/test_closed_map_view_host.py
// does).  No HIP in here.  Prints "ok <checks>" and exits 0 when every check holds.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <limits>

#include "../../tloam_amd/csrc/tl_view_box.hpp"

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

const int64_t kMiB = (int64_t)1 << 20, kMost = std::numeric_limits<int64_t>::max();
const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

void check_windows() {
  tlv::Window w;
  // max_range / voxel integral: W = the quotient + 1
  CHECK(tlv::make_window(20.0, 0.5, &w) && w.W == 41 && w.S == 83 && w.bits == 571787 && w.words == 17869 && w.bytes == 71476);
  CHECK(tlv::make_window(10.0, 0.5, &w) && w.W == 21 && w.S == 43 && w.bits == 79507 && w.words == 2485);
  CHECK(tlv::make_window(1.0, 1.0, &w) && w.W == 2 && w.S == 5 && w.bits == 125 && w.words == 4 && w.bytes == 16);
  // just off it, either way
  CHECK(tlv::make_window(nextafter(20.0, 21.0), 0.5, &w) && w.W == 42 && w.S == 85);
  CHECK(tlv::make_window(nextafter(20.0, 0.0), 0.5, &w) && w.W == 41);
  CHECK(tlv::make_window(0.4, 0.5, &w) && w.W == 2 && w.S == 5 && w.bits == 125 && w.words == 4);   // 125 bits: no multiple of 32
  CHECK(tlv::make_window(1e-300, 1.0, &w) && w.W == 2);
  for (int q = 1; q <= 200; ++q) {
    CHECK(tlv::make_window((double)q, 1.0, &w));
    CHECK(w.W == q + 1 && w.S == 2 * q + 3 && w.bits == (uint64_t)w.S * w.S * w.S);
    CHECK(w.words * 32 >= w.bits && (w.words - 1) * 32 < w.bits && w.bytes == 4 * w.words);
    CHECK(tlv::make_window((double)q + 0.25, 1.0, &w) && w.W == q + 2);
  }
  // the refusals
  for (double bad : {0.0, -1.0, kInf, -kInf, kNaN}) {
    CHECK(!tlv::make_window(bad, 0.5, &w));
    CHECK(!tlv::make_window(20.0, bad, &w));
  }
  CHECK(!tlv::make_window(1e-320, 1e300, &w));                       // the quotient underflows to 0
  CHECK(!tlv::make_window(1e300, 1e-300, &w));                       // ... overflows to inf
  // the largest side: S^3 stays below 2^63
  CHECK(tlv::make_window((double)(tlv::kMostW - 2), 1.0, &w) && w.W == tlv::kMostW - 1 && w.S == 2 * tlv::kMostW - 1);
  CHECK(w.bits == (uint64_t)w.S * (uint64_t)w.S * (uint64_t)w.S && w.bits < ((uint64_t)1 << 63) && w.bytes / 4 == w.words);
  CHECK(tlv::make_window((double)(tlv::kMostW - 1), 1.0, &w) && w.W == tlv::kMostW && w.S == 2 * tlv::kMostW + 1 && w.S < ((int64_t)1 << 21));
  CHECK(w.bits < ((uint64_t)1 << 63));
  CHECK(!tlv::make_window((double)tlv::kMostW, 1.0, &w) && !tlv::make_window(1e18, 1.0, &w) && !tlv::make_window(1e300, 1.0, &w));
}

void check_forms() {
  int ran = 7;
  // a window of exactly lds_bytes fits; one word above it does not
  for (uint64_t bytes : {(uint64_t)16, (uint64_t)71476, (uint64_t)131072}) {
    CHECK(tlv::choose_form(0, bytes, (int64_t)bytes, &ran) && ran == tlv::kFormLds);
    CHECK(tlv::choose_form(1, bytes, (int64_t)bytes, &ran) && ran == tlv::kFormLds);
    CHECK(tlv::choose_form(2, bytes, (int64_t)bytes, &ran) && ran == tlv::kFormGlobal);
    CHECK(tlv::choose_form(0, bytes + 4, (int64_t)bytes, &ran) && ran == tlv::kFormGlobal);
    ran = 7;
    CHECK(!tlv::choose_form(1, bytes + 4, (int64_t)bytes, &ran) && ran == 7);
    CHECK(tlv::choose_form(2, bytes + 4, (int64_t)bytes, &ran) && ran == tlv::kFormGlobal);
  }
  CHECK(tlv::choose_form(0, 16, 0, &ran) && ran == tlv::kFormGlobal);   // lds_bytes 0: never the LDS form
  CHECK(!tlv::choose_form(1, 16, 0, &ran));
  for (int bad : {-1, 3, 100}) CHECK(!tlv::choose_form(bad, 16, 131072, &ran));
  CHECK(!tlv::choose_form(0, 16, -1, &ran));
  CHECK(tlv::choose_form(0, std::numeric_limits<uint64_t>::max(), kMost, &ran) && ran == tlv::kFormGlobal);
}

void check_chunks() {
  uint64_t per = 7, chunks = 7;
  const uint64_t wb = 71476;
  // max_bytes of one window, one byte less, and many
  CHECK(tlv::make_chunks(33, wb, (int64_t)wb, &per, &chunks) && per == 1 && chunks == 33);
  per = chunks = 7;
  CHECK(!tlv::make_chunks(33, wb, (int64_t)wb - 1, &per, &chunks) && per == 7 && chunks == 7);
  CHECK(tlv::make_chunks(33, wb, 16 * (int64_t)wb, &per, &chunks) && per == 16 && chunks == 3);
  CHECK(tlv::make_chunks(33, wb, 17 * (int64_t)wb - 1, &per, &chunks) && per == 16 && chunks == 3);
  CHECK(tlv::make_chunks(32, wb, 16 * (int64_t)wb, &per, &chunks) && per == 16 && chunks == 2);
  CHECK(tlv::make_chunks(33, wb, 256 * kMiB, &per, &chunks) && per == 33 && chunks == 1);
  CHECK(tlv::make_chunks(1, wb, kMost, &per, &chunks) && per == 1 && chunks == 1);
  for (uint64_t views = 1; views <= 70; ++views)
    for (uint64_t hold = 1; hold <= 9; ++hold) {
      CHECK(tlv::make_chunks(views, 16, (int64_t)(16 * hold + 15), &per, &chunks));
      CHECK(per == (hold < views ? hold : views) && chunks == (views + per - 1) / per && (chunks - 1) * per < views);
    }
  // the refusals
  for (int64_t bad : {(int64_t)3, (int64_t)0, (int64_t)-1, std::numeric_limits<int64_t>::min()}) CHECK(!tlv::make_chunks(4, 4, bad, &per, &chunks));
  CHECK(!tlv::make_chunks(0, 16, kMiB, &per, &chunks) && !tlv::make_chunks(4, 0, kMiB, &per, &chunks));
  CHECK(!tlv::make_chunks(4, (uint64_t)kMost + 1, kMost, &per, &chunks));
  // more views than a launch's grid: the chunk is held to it
  CHECK(tlv::make_chunks((uint64_t)1 << 40, 4, kMost, &per, &chunks) && per == tlv::kMostBlocks && chunks == (((uint64_t)1 << 40) + per - 1) / per);
  // blocks a view, held to the grid
  CHECK(tlv::blocks_per_view(1, 23) == 23 && tlv::blocks_per_view(16, 1) == 1 && tlv::blocks_per_view(16, 0) == 1);
  CHECK(tlv::blocks_per_view(tlv::kMostBlocks, 2) == 1 && tlv::blocks_per_view(tlv::kMostBlocks / 2, 3) == 2);
  CHECK(tlv::blocks_per_view(1, std::numeric_limits<uint64_t>::max()) == tlv::kMostBlocks && tlv::blocks_per_view(0, 5) == 1);
  for (uint64_t v : {(uint64_t)1, (uint64_t)33, (uint64_t)65536, tlv::kMostBlocks})
    for (uint64_t want : {(uint64_t)1, (uint64_t)8, (uint64_t)100000, tlv::kMostBlocks}) {
      const uint64_t b = tlv::blocks_per_view(v, want);
      CHECK(b >= 1 && b <= want && b <= tlv::kMostBlocks / v);
    }
}

void check_rays() {
  uint64_t total = 7;
  CHECK(tlv::ray_count(1, 1, &total) && total == 1);
  CHECK(tlv::ray_count(33, 5760, &total) && total == 33 * 5760);
  total = 7;
  CHECK(!tlv::ray_count(0, 5, &total) && !tlv::ray_count(5, 0, &total) && !tlv::ray_count(0, 0, &total) && total == 7);
  // V * R near the integer limits: the product is never formed before it is known to fit
  const uint64_t big = std::numeric_limits<uint64_t>::max(), most = tlv::kMostInt64;
  CHECK(!tlv::ray_count(big, 1, &total) && !tlv::ray_count(1, big, &total) && !tlv::ray_count(big, big, &total));
  CHECK(!tlv::ray_count((uint64_t)1 << 32, (uint64_t)1 << 31, &total));                        // 2^63
  CHECK(tlv::ray_count((uint64_t)1 << 31, (uint64_t)1 << 31, &total) && total == (uint64_t)1 << 62);
  CHECK(tlv::ray_count(most / 128, 1, &total) && !tlv::ray_count(most / 128 + 1, 1, &total));   // the poses' bytes
  CHECK(tlv::ray_count(1, most / 24, &total) && !tlv::ray_count(1, most / 24 + 1, &total));     // the ends' bytes
  CHECK(tlv::ray_count(3, most / 24 / 3, &total) && total <= most);
  CHECK(tlv::ray_count(24, most / 24, &total) && !tlv::ray_count(25, most / 24, &total));
  CHECK(tlv::ray_count(7, most / 7 / 24, &total));
  CHECK(!tlv::ray_count(most / 128, most / 24, &total) && total <= most);
}

}  // namespace

int main() {
  check_windows();
  check_forms();
  check_chunks();
  check_rays();
  printf("ok %d\n", checks);
  return 0;
}
