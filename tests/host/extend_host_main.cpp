// A stand-alone driver of the closed map's host bookkeeping (tloam_amd/csrc/tl_extend_host.hpp: the span table of a keyframe
// range, the choice of a build's or an extension's poses, the 2^30 point bound, the infos' arithmetic), meant to be compiled for
// the host alone with -fsanitize=address,undefined and run on a machine without a GPU (tests/test_closed_map_extend_host.py
// does).  No HIP in here.
// Prints "ok <checks>" and exits 0 when every check holds.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../tloam_amd/csrc/tl_extend_host.hpp"

namespace {

struct Span { long long off, start; int kf, reserved0; };   // tl::CmapSpan's layout
struct Keyframe {                                           // what the table reads of PlaceState::Keyframe
  double pose[16];
  size_t off[8], n[8];
};

int checks = 0;
#define CHECK(x)                                                       \
  do {                                                                 \
    ++checks;                                                          \
    if (!(x)) {                                                        \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);          \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

std::vector<Keyframe> keyframes(size_t K) {
  std::vector<Keyframe> kf(K);
  size_t at = 0;
  for (size_t k = 0; k < K; ++k) {
    for (int i = 0; i < 16; ++i) kf[k].pose[i] = (i % 5 == 0) ? 1.0 : 0.0;
    kf[k].pose[12] = (double)k;
    for (int j = 0; j < 8; ++j) {
      kf[k].n[j] = (k % 4 == 3) ? 0 : (size_t)((k * 7 + j * 3) % 5);   // every fourth keyframe is empty, some slots are
      kf[k].off[j] = at;
      at += 3 * kf[k].n[j];
    }
  }
  return kf;
}

// the table of [first, last) against the definition, and against the tail of the table of [0, last)
void check_table(const std::vector<Keyframe>& kf, size_t first, size_t last, int mask) {
  std::vector<Span> part, whole;
  long long n = -1, n_whole = -1, n_before = -1;
  int64_t empty = 0, empty_whole = 0, empty_before = 0;
  tlx::span_range_table(kf.data(), kf.size(), first, last, mask, &part, &n, &empty);
  tlx::span_range_table(kf.data(), kf.size(), 0, last, mask, &whole, &n_whole, &empty_whole);
  std::vector<Span> before;
  tlx::span_range_table(kf.data(), kf.size(), 0, first, mask, &before, &n_before, &empty_before);
  CHECK(!part.empty() && part.back().start == n && part.back().kf == 0);
  CHECK(n + n_before == n_whole && empty + empty_before == empty_whole);
  CHECK(part.size() - 1 + before.size() - 1 == whole.size() - 1);
  long long at = 0;
  for (size_t s = 0; s + 1 < part.size(); ++s) {
    const Span& a = part[s];
    const Span& b = whole[before.size() - 1 + s];
    CHECK(a.start == at && a.off == b.off && a.start == b.start - n_before && a.kf == b.kf - (int)first);
    CHECK(a.kf >= 0 && (size_t)a.kf < (last < kf.size() ? last : kf.size()) - first);
    CHECK(part[s + 1].start > a.start);   // spans of at least one point
    at = part[s + 1].start;
  }
  CHECK(at == n);
}

void check_poses() {
  const size_t K = 3, n_kf = 7;
  std::vector<Keyframe> kf = keyframes(n_kf);
  auto stored = [&](size_t k, double* d) { memcpy(d, kf[k].pose, sizeof(double) * 16); };
  auto corrected = [&](size_t k, double* d) { stored(k, d); d[13] = 100.0 + (double)k; };
  auto carried = [&](size_t k, double* d) { stored(k, d); d[13] = -1.0; };
  auto rigid = [&](const double* p) { return p[0] == 1.0 && p[5] == 1.0 && p[10] == 1.0 && p[15] == 1.0; };
  std::vector<double> out;
  CHECK(tlx::extend_poses(0, nullptr, 0, K, n_kf, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_OK);
  CHECK(out.size() == 16 * (n_kf - K) && out[12] == 3.0 && out[16 * 3 + 12] == 6.0);
  CHECK(tlx::extend_poses(1, nullptr, 0, K, n_kf, false, 5, stored, corrected, carried, rigid, &out) == TLOAM_E_NOT_READY);
  CHECK(tlx::extend_poses(1, nullptr, 0, K, n_kf, true, 0, stored, corrected, carried, rigid, &out) == TLOAM_E_NOT_READY);
  CHECK(tlx::extend_poses(1, nullptr, 0, K, n_kf, true, 5, stored, corrected, carried, rigid, &out) == TLOAM_OK);
  CHECK(out[13] == 103.0 && out[16 + 13] == 104.0 && out[32 + 13] == -1.0 && out[48 + 13] == -1.0);
  CHECK(tlx::extend_poses(1, nullptr, 0, K, K, true, 0, stored, corrected, carried, rigid, &out) == TLOAM_OK && out.empty());
  std::vector<double> mine(16 * (n_kf - K));
  for (size_t k = K; k < n_kf; ++k) stored(k, &mine[16 * (k - K)]);
  CHECK(tlx::extend_poses(2, mine.data(), n_kf - K, K, n_kf, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_OK);
  CHECK(out == mine);
  CHECK(tlx::extend_poses(2, mine.data(), n_kf - K - 1, K, n_kf, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
  CHECK(tlx::extend_poses(2, mine.data(), n_kf, K, n_kf, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
  CHECK(tlx::extend_poses(2, nullptr, n_kf - K, K, n_kf, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
  CHECK(tlx::extend_poses(2, nullptr, 0, K, K, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_OK && out.empty());
  std::vector<double> bad = mine;
  bad[16 * 2 + 14] = NAN;
  CHECK(tlx::extend_poses(2, bad.data(), n_kf - K, K, n_kf, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
  bad = mine;
  bad[16 * 3 + 5] = 2.0;
  CHECK(tlx::extend_poses(2, bad.data(), n_kf - K, K, n_kf, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
  CHECK(tlx::extend_poses(3, nullptr, 0, K, n_kf, true, 5, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
  CHECK(tlx::extend_poses(-1, nullptr, 0, K, n_kf, true, 5, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
  CHECK(tlx::extend_poses(0, nullptr, 0, n_kf, K, false, 0, stored, corrected, carried, rigid, &out) == TLOAM_E_INVALID);
}

void check_infos() {
  tloam_closed_map_info I{};
  tloam_closed_map_surfel_info S{};
  tloam_closed_map_carve_info V{};
  I.n_keyframes = 4; I.added_keyframes = 3; I.empty_keyframes = 1; I.n_voxels = 100; I.n_points = 1000; I.pose_source = 2;
  I.launches = 4;
  S.n_keyframes = 4; S.n_points = 1000; S.solved_voxels = 60; S.launches = 4;
  V.n_keyframes = 4; V.n_rays = 1100; V.skipped_rays = 7; V.steps = 9000; V.tested = 800; V.misses = 90; V.voxels_missed = 30;
  V.launches = 3;
  tlx::ExtendCounts C{};
  C.n_new = 3; C.empty = 1; C.overflow = 1;
  C.points = 250; C.fresh = 20; C.touched = 55;
  C.surfel_points = 250; C.surfel_newly_solved = 12;
  C.rays = 260; C.skipped = 2; C.steps = 2000; C.tested = 150; C.misses = 11; C.voxels_missed = 36;
  const tloam_closed_map_info I0 = I;
  const tloam_closed_map_surfel_info S0 = S;
  const tloam_closed_map_carve_info V0 = V;
  tloam_closed_map_extend_info E{};
  tlx::extend_apply(C, 0, true, true, &I, &S, &V, &E);
  CHECK(E.first_keyframe == 4 && E.n_keyframes == 3 && E.added_keyframes == 1 && E.empty_keyframes == 1 && E.overflow_keyframes == 1);
  CHECK(E.points == 250 && E.new_voxels == 20 && E.touched_voxels == 55 && E.solved_voxels == 72);
  CHECK(E.rays == 260 && E.skipped_rays == 2 && E.steps == 2000 && E.tested == 150 && E.misses == 11);
  CHECK(I.n_keyframes == 7 && I.added_keyframes == 4 && I.empty_keyframes == 2 && I.overflow_keyframes == 1);
  CHECK(I.n_keyframes == I.added_keyframes + I.empty_keyframes + I.overflow_keyframes);
  CHECK(I.n_voxels == 120 && I.n_points == 1250 && I.pose_source == 0 && I.launches == 4);
  CHECK(S.n_keyframes == 7 && S.n_points == 1250 && S.solved_voxels == 72 && S.orphan_points == 0 && S.launches == 4);
  CHECK(V.n_keyframes == 7 && V.n_rays == 1360 && V.skipped_rays == 9 && V.steps == 11000 && V.tested == 950 && V.misses == 101);
  CHECK(V.voxels_missed == 36 && V.launches == 3);
  // a map without surfels or a carve: their infos are not touched, the call's own fields stay zero
  I = I0; S = S0; V = V0;
  tloam_closed_map_extend_info F{};
  tlx::extend_apply(C, 2, false, false, &I, &S, &V, &F);
  CHECK(memcmp(&S, &S0, sizeof(S)) == 0 && memcmp(&V, &V0, sizeof(V)) == 0);
  CHECK(F.rays == 0 && F.misses == 0 && F.solved_voxels == 0 && F.points == 250 && I.n_voxels == 120);
}

// the 2^30 bound on the points the rows would hold: at it, one past it, and nothing of the info written
void check_point_bound() {
  const int64_t kMax = (int64_t)1 << 30;
  CHECK(tlx::kMaxMapPoints == kMax);
  tloam_closed_map_info I{};
  I.n_keyframes = 9; I.added_keyframes = 9; I.n_voxels = 1234; I.n_points = kMax - 1000; I.capacity_voxels = 5000; I.pose_source = 2;
  I.launches = 4;
  const tloam_closed_map_info I0 = I;
  CHECK(tlx::extend_points_check(I, 0) == TLOAM_OK);
  CHECK(tlx::extend_points_check(I, 999) == TLOAM_OK);
  CHECK(tlx::extend_points_check(I, 1000) == TLOAM_OK);            // exactly 2^30
  CHECK(tlx::extend_points_check(I, 1001) == TLOAM_E_INVALID);     // one past it
  CHECK(tlx::extend_points_check(I, kMax) == TLOAM_E_INVALID);
  CHECK(tlx::extend_points_check(I, INT64_MAX) == TLOAM_E_INVALID);   // (no overflow on the way)
  CHECK(tlx::extend_points_check(I, -1) == TLOAM_E_INVALID);
  CHECK(memcmp(&I, &I0, sizeof(I)) == 0);
  I.n_points = kMax;
  CHECK(tlx::extend_points_check(I, 0) == TLOAM_OK && tlx::extend_points_check(I, 1) == TLOAM_E_INVALID);
  I.n_points = 0;
  CHECK(tlx::extend_points_check(I, kMax) == TLOAM_OK && tlx::extend_points_check(I, kMax + 1) == TLOAM_E_INVALID);
  I.n_points = kMax + 1;   // (a map no build makes)
  CHECK(tlx::extend_points_check(I, 0) == TLOAM_E_INVALID);
}

}  // namespace

int main() {
  for (size_t K : {(size_t)0, (size_t)1, (size_t)5, (size_t)12}) {
    const std::vector<Keyframe> kf = keyframes(K);
    for (int mask : {0x10, 0xF0, 0xFF, 0x01, 0xA5})
      for (size_t first = 0; first <= K; ++first)
        for (size_t last = first; last <= K + 2; ++last) check_table(kf, first, last, mask);   // (last past the end: clipped)
  }
  check_poses();
  check_infos();
  check_point_bound();
  printf("ok %d\n", checks);
  return 0;
}
