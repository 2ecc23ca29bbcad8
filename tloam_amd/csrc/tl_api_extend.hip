// tl_api_extend.hip -- C ABI of the closed map's extension (include/tloam_hip.h: tloam_closed_map_extend, _get_extend_info;
// DESIGN.md section 27; kernels in tl_extend.hip, tl_cmap.hip, tl_surfel.hip and tl_carve.hip; the host bookkeeping in
// tl_extend_host.hpp).
//
// An extension takes the keyframes [K, n_kf) of the host's keyframe table (PlaceState::kf) and a pose for each, uploads a span
// table of those keyframes alone, and enqueues on the context's stream: the build's clear | flag | stage into a staging sized by
// the NEW points, k_ext_emit and k_ext_commit (the map's rows and table written), then, when the map has surfels,
// k_surfel_accum over the new spans and k_surfel_solve_staged, and, when it is carved, k_carve_rays over the new ray spans and
// k_carve_count.  It waits once, at its end -- unless the new points could outgrow the rows: then the fresh voxels are read
// after the emit, and the rows and every array beside them are reallocated, copied and rehashed before the commit.  The staging
// is the call's own and freed with it; nothing is sized by the map.
#include <float.h>
#include <math.h>

#include "tl_ctx.hpp"
#include "tl_extend_host.hpp"

using namespace tl;

namespace {

// the call's device staging, freed with it (hipFree waits for the launches that use it)
struct Staging {
  DBuf<unsigned long long> fkey, flead, fsum, look, ctl;
  DBuf<int> slot_of_pt, kf_over, fid;
  SpanUpload up, up_rays;
};

// `b` holds `want` elements, its first `keep` kept (grown by doubling: a run of extends does not copy every time); the stream is
// idle when the old storage goes
template <class T>
int grow_keep(tloam_ctx* c, DBuf<T>& b, size_t keep, size_t want) {
  if (want <= b.cap) return TLOAM_OK;
  DBuf<T> nb;
  HIPC(c, nb.reserve(std::max(want, 2 * b.cap)));
  if (keep && b.p) HIPC(c, hipMemcpyAsync(nb.p, b.p, sizeof(T) * keep, hipMemcpyDeviceToDevice, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  b = std::move(nb);
  return TLOAM_OK;
}

// the arrays beside the rows hold `ids` ids -- the ids the call can reach, not the rows' capacity: a carve sizes M by the voxels
// it counted, a pass or a load the surfels' arrays by the capacity -- what they hold of ids [0, base) kept
int sides_reserve(tloam_ctx* c, size_t base, size_t ids) {
  CmapState& M = c->cmap;
  const size_t cap = std::max<size_t>(ids, 1);
  int rc = TLOAM_OK;
  if (M.carved) rc = grow_keep(c, M.miss, base, cap);
  if (rc == TLOAM_OK && M.surfeled) {
    rc = grow_keep(c, M.surfel_sums, kSurfelSums * base, kSurfelSums * cap);
    if (rc == TLOAM_OK) rc = grow_keep(c, M.surfel_nrm, 3 * base, 3 * cap);
    if (rc == TLOAM_OK) rc = grow_keep(c, M.surfel_ev, 3 * base, 3 * cap);
  }
  return rc;
}

// the rows reallocated for `need` voxels: the `base` rows copied, the table rebuilt from their keys, the side arrays following
// (the localiser's records are stale after an extension and sized again by their next prepare)
int rows_grow(tloam_ctx* c, size_t base, size_t need, int* launches) {
  CmapState& M = c->cmap;
  VoxelRowStore& R = M.rows;
  const size_t want = std::max(need, 2 * R.cap);
  size_t tsize = 1024;
  while (tsize < 2 * want) tsize <<= 1;
  VoxelRowStore N;
  HIPC(c, N.key.reserve(want));
  for (DBuf<long long>* a : {&N.n, &N.qx, &N.qy, &N.qz}) HIPC(c, a->reserve(want));
  HIPC(c, N.tab.reserve(tsize));
  N.cap = want;
  N.tmask = tsize - 1;
  const hipMemcpyKind D2D = hipMemcpyDeviceToDevice;
  if (base) {
    HIPC(c, hipMemcpyAsync(N.key.p, R.key.p, sizeof(unsigned long long) * base, D2D, c->stream));
    HIPC(c, hipMemcpyAsync(N.n.p, R.n.p, sizeof(long long) * base, D2D, c->stream));
    HIPC(c, hipMemcpyAsync(N.qx.p, R.qx.p, sizeof(long long) * base, D2D, c->stream));
    HIPC(c, hipMemcpyAsync(N.qy.p, R.qy.p, sizeof(long long) * base, D2D, c->stream));
    HIPC(c, hipMemcpyAsync(N.qz.p, R.qz.p, sizeof(long long) * base, D2D, c->stream));
  }
  HIPC(c, hipMemsetAsync(N.tab.p, 0xff, sizeof(int) * tsize, c->stream));
  launch_vmap_rehash(N.table(), base, c->stream, true);   // (launched without a row too: the count depends on `grown` alone)
  HIPC(c, hipGetLastError());
  *launches += 1;
  HIPC(c, hipStreamSynchronize(c->stream));
  R = std::move(N);
  return sides_reserve(c, base, need);
}

// the enqueue, the waits and the counts of an extension whose inputs have been checked.  *launched: a launch has been made (a
// failure from there on empties the closed map)
int extend_body(tloam_ctx* c, size_t K, size_t n_kf, int pose_source, const std::vector<double>& poses,
                tloam_closed_map_extend_info& E, bool* launched) {
  CmapState& M = c->cmap;
  const PlaceState& P = c->place;
  const size_t n_new = n_kf - K, base = (size_t)M.info.n_voxels;
  tlx::ExtendCounts C;
  memset(&C, 0, sizeof(C));
  C.n_new = (int64_t)n_new;
  std::vector<CmapSpan> spans, ray_spans;
  long long n = 0, n_rays = 0;
  cmap_span_table(P, K, n_kf, M.cfg.cloud_mask, &spans, &n, &C.empty);
  // the 2^30 bound of the build, on the points the rows would then hold (refused before anything is allocated or launched)
  if (tlx::extend_points_check(M.info, n) != TLOAM_OK) return TLOAM_E_INVALID;
  if (M.carved) cmap_span_table(P, K, n_kf, M.carve_cfg.ray_mask ? M.carve_cfg.ray_mask : M.cfg.cloud_mask, &ray_spans, &n_rays, nullptr);
  HIPC(c, hipSetDevice(c->device));
  // the ids the call can reach without growing; `may_grow`: the fresh voxels are read before the commit
  const bool may_grow = base + (size_t)n > M.rows.cap;
  size_t upper = std::min(base + (size_t)n, M.rows.cap);
  HIPC(c, hipStreamSynchronize(c->stream));   // (a side array replaced may still be read)
  int rc = sides_reserve(c, base, upper);
  if (rc != TLOAM_OK) return rc;
  Staging S;
  const size_t m = std::max<size_t>((size_t)n, 1), T = voxel_table_size(m), blocks = (m + 255) / 256;
  HIPC(c, S.fkey.reserve(T)); HIPC(c, S.flead.reserve(T)); HIPC(c, S.fsum.reserve(4 * T)); HIPC(c, S.fid.reserve(T));
  HIPC(c, S.slot_of_pt.reserve(m)); HIPC(c, S.look.reserve(blocks + 1)); HIPC(c, S.ctl.reserve(8));
  HIPC(c, S.kf_over.reserve(std::max<size_t>(n_new, 1)));
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  ExtendWork X;
  memset(&X, 0, sizeof(X));
  CmapWork& W = X.w;
  rc = S.up.upload(c, spans, n, poses.data(), n_new, &W.in);
  if (rc != TLOAM_OK) return rc;
  W.runs = getenv("TLOAM_CMAP_NO_RUNS") ? 0 : 1;   // (the build's A/B switch)
  W.kf_over = S.kf_over.p;
  W.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) W.origin[a] = M.cfg.origin[a];
  W.fmask = T - 1;
  W.fkey = S.fkey.p; W.flead = S.flead.p; W.fsum = S.fsum.p; W.slot_of_pt = S.slot_of_pt.p;
  W.look = S.look.p; W.ctl = S.ctl.p;
  W.rows = M.rows.table();
  W.row_cap = (long long)M.rows.cap;
  X.fid = S.fid.p;
  X.base = (long long)base;
  X.side_cap = (long long)upper;
  *launched = true;
  E.launches = launch_cmap_stage(W, c->stream);
  HIPC(c, hipGetLastError());
  E.launches += launch_extend_emit(X, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long ctl[8];
  if (may_grow) {
    HIPC(c, hipMemcpyAsync(ctl, S.ctl.p, sizeof(ctl), D2H, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (ctl[3]) {
      c->last_error = "closed map extend: a look-back of k_ext_emit timed out";
      return TLOAM_E_HIP;
    }
    if (ctl[4] > ctl[0] || base + (size_t)ctl[4] > (size_t)tlx::kMaxMapPoints) {
      c->last_error = "closed map extend: more voxels numbered than staged";
      return TLOAM_E_HIP;
    }
    upper = base + (size_t)ctl[4];
    if (upper > M.rows.cap) {
      int extra = 0;
      rc = rows_grow(c, base, upper, &extra);
      if (rc != TLOAM_OK) return rc;
      E.launches += extra;
      E.grown = 1;
      W.rows = M.rows.table();
      W.row_cap = (long long)M.rows.cap;
    }
    X.side_cap = (long long)upper;
  }
  // M of the ids the call may create starts at 0 whether or not it creates them: k_carve_count then reads [0, upper)
  if (M.carved && upper > base) HIPC(c, hipMemsetAsync(M.miss.p + base, 0, sizeof(unsigned long long) * (upper - base), c->stream));
  X.miss = M.carved ? M.miss.p : nullptr;
  X.sums = M.surfeled ? M.surfel_sums.p : nullptr;
  E.launches += launch_extend_commit(X, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long sctl[8] = {0}, cctl[8] = {0};
  if (M.surfeled) {
    HIPC(c, M.surfel_ctl.reserve(8));
    HIPC(c, hipMemsetAsync(M.surfel_ctl.p, 0, sizeof(sctl), c->stream));
    SurfelWork SW;
    memset(&SW, 0, sizeof(SW));
    SW.in = W.in;
    SW.kf_over = S.kf_over.p;   // the row pass's flags: the same rule, the same keyframes
    SW.grid = map_grid_of(M);   // (the rows as the commit left them)
    SW.grid.nv = (long long)upper;
    SW.runs = getenv("TLOAM_SURFEL_NO_RUNS") ? 0 : 1;
    SW.min_points = M.surfel_cfg.min_points;
    SW.sums = M.surfel_sums.p; SW.normal = M.surfel_nrm.p; SW.eval = M.surfel_ev.p;
    SW.ctl = M.surfel_ctl.p;
    E.launches += launch_surfel_accum(SW, c->stream);
    E.launches += launch_surfel_solve_staged(SW, StagedVoxels{W.fmask, S.fkey.p, S.fid.p, S.fsum.p}, c->stream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(sctl, M.surfel_ctl.p, sizeof(sctl), D2H, c->stream));
  }
  if (M.carved) {
    const tloam_closed_map_carve_config& g = M.carve_cfg;
    HIPC(c, M.carve_ctl.reserve(8));
    HIPC(c, hipMemsetAsync(M.carve_ctl.p, 0, sizeof(cctl), c->stream));
    CarveWork CW;
    memset(&CW, 0, sizeof(CW));
    rc = S.up_rays.upload(c, ray_spans, n_rays, poses.data(), n_new, &CW.in);
    if (rc != TLOAM_OK) return rc;
    CW.grid = map_grid_of(M);
    CW.grid.nv = (long long)upper;
    CW.max_range = g.max_range; CW.end_margin = g.end_margin; CW.radius2 = g.radius * g.radius;
    CW.miss = M.miss.p;
    CW.ctl = M.carve_ctl.p;
    E.launches += launch_carve_rays(CW, c->stream);
    E.launches += launch_carve_count(CW, c->stream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(cctl, M.carve_ctl.p, sizeof(cctl), D2H, c->stream));
  }
  std::vector<int> over(std::max<size_t>(n_new, 1));
  HIPC(c, hipMemcpyAsync(ctl, S.ctl.p, sizeof(ctl), D2H, c->stream));
  HIPC(c, hipMemcpyAsync(over.data(), S.kf_over.p, sizeof(int) * n_new, D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (ctl[3]) {
    c->last_error = "closed map extend: a look-back of k_ext_emit timed out";
    return TLOAM_E_HIP;
  }
  if (ctl[4] > ctl[0] || base + (size_t)ctl[4] > upper) {
    c->last_error = "closed map extend: the voxels numbered are not the voxels the rows hold";
    return TLOAM_E_HIP;
  }
  for (size_t k = 0; k < n_new; ++k) C.overflow += over[k] ? 1 : 0;
  C.points = (int64_t)ctl[1];
  C.fresh = (int64_t)ctl[4];
  C.touched = (int64_t)ctl[0];
  C.surfel_points = (int64_t)sctl[0]; C.surfel_orphans = (int64_t)sctl[1]; C.surfel_newly_solved = (int64_t)sctl[2];
  C.rays = (int64_t)n_rays;
  C.skipped = (int64_t)cctl[0]; C.steps = (int64_t)cctl[1]; C.tested = (int64_t)cctl[2]; C.misses = (int64_t)cctl[3];
  C.voxels_missed = (int64_t)cctl[4];
  tlx::extend_apply(C, pose_source, M.surfeled, M.carved, &M.info, &M.surfel_info, &M.carve_info, &E);
  return TLOAM_OK;
}

}  // namespace

extern "C" {

int tloam_closed_map_get_extend_info(tloam_ctx* c, tloam_closed_map_extend_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.extend_info;
  return TLOAM_OK;
}

int tloam_closed_map_extend(tloam_ctx* c, int pose_source, const double* poses, size_t n_poses, tloam_closed_map_extend_info* info) {
  if (!c || c->nranks > 1 || !place_clouds_on(c)) return TLOAM_E_INVALID;
  if (pose_source < TLOAM_CLOSED_MAP_POSES_STORED || pose_source > TLOAM_CLOSED_MAP_POSES_CALLER) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built) return TLOAM_E_NOT_READY;
  const PlaceState& P = c->place;
  const GraphState& G = c->graph;
  const size_t K = (size_t)M.info.n_keyframes, n_kf = P.kf.size(), nc = G.corrected.size() / 16;
  std::vector<double> used;
  int rc = tlx::extend_poses(
      pose_source, poses, n_poses, K, n_kf, G.have, nc,
      [&](size_t k, double* dst) { memcpy(dst, P.kf[k].pose, sizeof(double) * 16); },
      [&](size_t k, double* dst) { memcpy(dst, &G.corrected[16 * k], sizeof(double) * 16); },
      [&](size_t k, double* dst) { graph_correct_pose(c, nc - 1, P.kf[k].pose, dst); },   // a keyframe added since the optimise
      [&](const double* pose) { Pose unused; return pose_from_matrix(pose, &unused); },   // (the rigid test of tloam_graph_solve)
      &used);
  if (rc != TLOAM_OK) return rc;
  tloam_closed_map_extend_info E;
  memset(&E, 0, sizeof(E));
  E.first_keyframe = (int64_t)K;
  E.solved_voxels = M.surfeled ? M.surfel_info.solved_voxels : 0;
  if (n_kf == K) {   // nothing to take: nothing changes
    M.extend_info = E;
    if (info) *info = E;
    return TLOAM_OK;
  }
  bool launched = false;
  rc = extend_body(c, K, n_kf, pose_source, used, E, &launched);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);   // (nothing of the call is in flight when its staging goes)
    if (launched) M.drop();                  // the rows may be half written: the closed map is empty, as after a failed build
    return rc;
  }
  M.poses.insert(M.poses.end(), used.begin(), used.end());
  M.drop_localise();   // the voxel records are those of the map before
  M.drop_diff();
  M.free.drop_fields();   // the clearance and the frontiers were built from the voxels of the map before (the free-space grid stays)
  M.extend_info = E;
  if (info) *info = E;
  return TLOAM_OK;
}

}  // extern "C"
