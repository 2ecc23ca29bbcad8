// tl_extend_host.hpp -- the host-side bookkeeping of the closed map's span tables and of its extension (tl_api_cmap.hip,
// tl_api_extend.hip, DESIGN.md sections 19 and 27): the span table of a keyframe range, the choice of the new keyframes' poses,
// and the arithmetic of the infos.  No HIP and no context in here, so that a stand-alone program can drive it under the host
// sanitizers (tests/host/extend_host_main.cpp); everything that needs the context comes in as a callable.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/tloam_hip.h"

namespace tlx {

// The span table for `mask` over keyframes [first, min(last, nkf)) of kf[nkf] (off[8] in doubles, n[8] in points per keyframe):
// keyframes ascending, a keyframe's selected clouds in slot order, empty clouds left out, the end sentinel last
// (spans->back().start = *n).  A span's kf counts from `first`.  *empty (may be null) grows by the keyframes that add no span.
template <class Span, class Keyframe>
void span_range_table(const Keyframe* kf, size_t nkf, size_t first, size_t last, int mask, std::vector<Span>* spans, long long* n,
                      int64_t* empty) {
  long long at = 0;
  for (size_t k = first; k < last && k < nkf; ++k) {
    const long long before = at;
    for (int j = 0; j < 8; ++j) {
      if (!((mask >> j) & 1) || kf[k].n[j] == 0) continue;
      spans->push_back(Span{(long long)kf[k].off[j], at, (int)(k - first), 0});
      at += (long long)kf[k].n[j];
    }
    if (at == before && empty) ++*empty;
  }
  spans->push_back(Span{0, at, 0, 0});
  *n = at;
}

// The poses of keyframes [K, n_kf) for an extension, [16 (n_kf - K)] column-major in *out; TLOAM_OK, TLOAM_E_INVALID or
// TLOAM_E_NOT_READY.  pose_source 0: stored(k, dst); 1: the build's rule -- the corrected pose of a keyframe the last optimise
// covered (corrected(k, dst), k < n_corrected), the correction of the last covered keyframe carried to a later one
// (carried(k, dst)), TLOAM_E_NOT_READY without an optimise; 2: the caller's n_caller poses, each finite and rigid(pose).
template <class Stored, class Corrected, class Carried, class Rigid>
int extend_poses(int pose_source, const double* caller, size_t n_caller, size_t K, size_t n_kf, bool graph_have, size_t n_corrected,
                 Stored stored, Corrected corrected, Carried carried, Rigid rigid, std::vector<double>* out) {
  if (n_kf < K) return TLOAM_E_INVALID;
  const size_t m = n_kf - K;
  out->assign(16 * m, 0.0);
  if (pose_source == TLOAM_CLOSED_MAP_POSES_CALLER) {
    if (n_caller != m || (m > 0 && !caller)) return TLOAM_E_INVALID;
    for (size_t k = 0; k < m; ++k) {
      for (int i = 0; i < 16; ++i)
        if (!isfinite(caller[16 * k + i])) return TLOAM_E_INVALID;
      if (!rigid(caller + 16 * k)) return TLOAM_E_INVALID;
    }
    if (m) memcpy(out->data(), caller, sizeof(double) * 16 * m);
  } else if (pose_source == TLOAM_CLOSED_MAP_POSES_CORRECTED) {
    if (!graph_have || (n_corrected == 0 && m > 0)) return TLOAM_E_NOT_READY;
    for (size_t k = K; k < n_kf; ++k) {
      if (k < n_corrected) corrected(k, out->data() + 16 * (k - K));
      else carried(k, out->data() + 16 * (k - K));
    }
  } else if (pose_source == TLOAM_CLOSED_MAP_POSES_STORED) {
    for (size_t k = K; k < n_kf; ++k) stored(k, out->data() + 16 * (k - K));
  } else {
    return TLOAM_E_INVALID;
  }
  return TLOAM_OK;
}

// The rows hold at most 2^30 points (slots and ids are 32-bit: the build's bound).  An extension by `n_new` points -- the points
// of the new keyframes' spans, an upper bound of what it adds -- onto a map of I.n_points is TLOAM_OK while the sum stays within
// the bound and TLOAM_E_INVALID beyond it; nothing is written.
constexpr int64_t kMaxMapPoints = (int64_t)1 << 30;
inline int extend_points_check(const tloam_closed_map_info& I, long long n_new) {
  if (n_new < 0 || I.n_points < 0 || I.n_points > kMaxMapPoints) return TLOAM_E_INVALID;
  return n_new <= kMaxMapPoints - I.n_points ? TLOAM_OK : TLOAM_E_INVALID;
}

// what the device counted in one extension
struct ExtendCounts {
  int64_t n_new;                       // keyframes taken
  int64_t empty, overflow;             // of them
  int64_t points, fresh, touched;      // the row pass
  int64_t surfel_points, surfel_orphans, surfel_newly_solved;   // the surfels (zero without them)
  int64_t rays, skipped, steps, tested, misses, voxels_missed;  // the carve (zero without it); voxels_missed: of the stored M
};

// the infos after the extension; *E is the call's own
inline void extend_apply(const ExtendCounts& C, int pose_source, bool surfeled, bool carved, tloam_closed_map_info* I,
                         tloam_closed_map_surfel_info* S, tloam_closed_map_carve_info* V, tloam_closed_map_extend_info* E) {
  E->first_keyframe = I->n_keyframes;
  E->n_keyframes = C.n_new;
  E->empty_keyframes = C.empty;
  E->overflow_keyframes = C.overflow;
  E->added_keyframes = C.n_new - C.empty - C.overflow;
  E->points = C.points;
  E->new_voxels = C.fresh;
  E->touched_voxels = C.touched;
  I->n_keyframes += C.n_new;
  I->empty_keyframes += C.empty;
  I->overflow_keyframes += C.overflow;
  I->added_keyframes += E->added_keyframes;
  I->n_voxels += C.fresh;
  I->n_points += C.points;
  I->pose_source = pose_source;
  if (surfeled) {
    S->n_keyframes = I->n_keyframes;
    S->n_points += C.surfel_points;
    S->orphan_points += C.surfel_orphans;
    S->solved_voxels += C.surfel_newly_solved;
    E->solved_voxels = S->solved_voxels;
  }
  if (carved) {
    V->n_keyframes = I->n_keyframes;
    V->n_rays += C.rays;
    V->skipped_rays += C.skipped;
    V->steps += C.steps;
    V->tested += C.tested;
    V->misses += C.misses;           // (M of a new id starts at 0: the stored sum grows by the call's misses)
    V->voxels_missed = C.voxels_missed;
    E->rays = C.rays;
    E->skipped_rays = C.skipped;
    E->steps = C.steps;
    E->tested = C.tested;
    E->misses = C.misses;
  }
}

}  // namespace tlx
