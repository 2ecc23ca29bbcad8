// tl_api_cmap.hip -- C ABI of the closed map (include/tloam_hip.h: tloam_closed_map_*; kernels in
// tl_cmap.hip, reads by tlh::voxel_rows_read / _read_box).  The span table, its upload and the side arrays' range check that the
// carve and the surfels share with the build are defined here (tlh::cmap_span_table, SpanUpload, cmap_side_range).
//
// A build takes the host's keyframe table (PlaceState::kf: where every stored cloud lies in the arena) and a pose per keyframe,
// uploads one span table and the poses, and enqueues four launches on the context's stream -- behind any k_place_clouds still in
// flight.  The rows are sized before the numbering writes them: a build of no more points than the rows hold waits once, at its
// end; a larger one reads the count of distinct voxels first.  The staging (the build table, a slot per point) is the build's
// own and is freed when it ends.  Nothing else in the context is read or written.
#include <float.h>
#include <math.h>

#include "tl_ctx.hpp"
#include "tl_extend_host.hpp"

using namespace tl;

namespace {

constexpr size_t kCmapDefaultReserve = (size_t)1 << 20;   // voxels (40 MiB of rows, 8 MiB of table): reserve_voxels = 0
constexpr size_t kCmapMaxPoints = (size_t)1 << 30;        // slots and ids are 32-bit

bool cmap_config_ok(const tloam_closed_map_config& m) {
  return m.voxel > 0.0 && m.voxel <= DBL_MAX && std::isfinite(m.origin[0]) && std::isfinite(m.origin[1]) &&
         std::isfinite(m.origin[2]) && m.cloud_mask > 0 && m.cloud_mask <= 0xFF && m.reserve_voxels >= 0;
}

bool cmap_on(const tloam_ctx* c) { return c && c->nranks == 1 && place_clouds_on(c); }

// a build's device staging, freed with it (hipFree waits for the launches that use it)
struct Staging {
  DBuf<unsigned long long> fkey, flead, fsum, look, ctl;
  DBuf<int> slot_of_pt, kf_over;
  SpanUpload up;
};

// the rows hold `need` voxels; the closed map is being replaced, so nothing is copied
int rows_reserve(tloam_ctx* c, size_t need) {
  VoxelRowStore& R = c->cmap.rows;
  if (need <= R.cap) return TLOAM_OK;
  const size_t want = std::max(need, 2 * R.cap);
  size_t tsize = 1024;
  while (tsize < 2 * want) tsize <<= 1;
  HIPC(c, hipStreamSynchronize(c->stream));   // (a launch in flight may still write the rows replaced)
  R = VoxelRowStore();
  HIPC(c, R.key.reserve(want));
  for (DBuf<long long>* a : {&R.n, &R.qx, &R.qy, &R.qz}) HIPC(c, a->reserve(want));
  HIPC(c, R.tab.reserve(tsize));
  R.cap = want;
  R.tmask = tsize - 1;
  return TLOAM_OK;
}

// the enqueue, the waits and the counts of a build whose inputs have been checked; the closed map has been dropped
int build_body(tloam_ctx* c, const std::vector<double>& poses, tloam_closed_map_info& I) {
  CmapState& M = c->cmap;
  const PlaceState& P = c->place;
  const size_t K = P.kf.size();
  std::vector<CmapSpan> spans;
  long long n = 0;
  cmap_span_table(P, 0, K, M.cfg.cloud_mask, &spans, &n, &I.empty_keyframes);
  if ((size_t)n > kCmapMaxPoints) {
    c->last_error = "closed map: more than 2^30 points";
    return TLOAM_E_HIP;
  }
  HIPC(c, hipSetDevice(c->device));
  int rc = rows_reserve(c, M.cfg.reserve_voxels > 0 ? (size_t)M.cfg.reserve_voxels : kCmapDefaultReserve);
  if (rc != TLOAM_OK) return rc;
  Staging S;
  const size_t m = std::max<size_t>((size_t)n, 1), T = voxel_table_size(m), blocks = (m + 255) / 256;
  HIPC(c, S.fkey.reserve(T)); HIPC(c, S.flead.reserve(T)); HIPC(c, S.fsum.reserve(4 * T)); HIPC(c, S.slot_of_pt.reserve(m));
  HIPC(c, S.look.reserve(blocks + 1)); HIPC(c, S.ctl.reserve(8)); HIPC(c, S.kf_over.reserve(std::max<size_t>(K, 1)));
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  static const bool no_runs = getenv("TLOAM_CMAP_NO_RUNS") != nullptr;   // A/B of the wave's run aggregation
  CmapWork W;
  memset(&W, 0, sizeof(W));
  rc = S.up.upload(c, spans, n, poses.data(), K, &W.in);
  if (rc != TLOAM_OK) return rc;
  W.runs = no_runs ? 0 : 1;
  W.kf_over = S.kf_over.p;
  W.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) W.origin[a] = M.cfg.origin[a];
  W.fmask = T - 1;
  W.fkey = S.fkey.p; W.flead = S.flead.p; W.fsum = S.fsum.p; W.slot_of_pt = S.slot_of_pt.p;
  W.look = S.look.p; W.ctl = S.ctl.p;
  I.launches = launch_cmap_stage(W, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long ctl[8];
  if ((size_t)n > M.rows.cap) {   // more points than rows: the rows are sized by the count of distinct voxels
    HIPC(c, hipMemcpyAsync(ctl, S.ctl.p, sizeof(ctl), D2H, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    rc = rows_reserve(c, (size_t)ctl[0]);
    if (rc != TLOAM_OK) return rc;
  }
  HIPC(c, hipMemsetAsync(M.rows.tab.p, 0xff, sizeof(int) * (size_t)(M.rows.tmask + 1), c->stream));
  W.rows = M.rows.table();
  W.row_cap = (long long)M.rows.cap;
  I.launches += launch_cmap_emit(W, c->stream);
  HIPC(c, hipGetLastError());
  std::vector<int> over(std::max<size_t>(K, 1));
  HIPC(c, hipMemcpyAsync(ctl, S.ctl.p, sizeof(ctl), D2H, c->stream));
  if (K) HIPC(c, hipMemcpyAsync(over.data(), S.kf_over.p, sizeof(int) * K, D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (ctl[3]) {
    c->last_error = "closed map: a look-back of k_cmap_emit timed out";
    return TLOAM_E_HIP;
  }
  if (ctl[4] != ctl[0] || ctl[4] > M.rows.cap) {
    c->last_error = "closed map: the voxels numbered are not the voxels counted";
    return TLOAM_E_HIP;
  }
  for (size_t k = 0; k < K; ++k) I.overflow_keyframes += over[k] ? 1 : 0;
  I.added_keyframes = (int64_t)K - I.empty_keyframes - I.overflow_keyframes;
  I.n_voxels = (int64_t)ctl[4];
  I.n_points = (int64_t)ctl[1];
  return TLOAM_OK;
}

}  // namespace

namespace tlh {

bool cmap_config_valid(const tloam_closed_map_config& cfg) { return cmap_config_ok(cfg); }
size_t cmap_default_reserve() { return kCmapDefaultReserve; }

void cmap_span_table(const PlaceState& P, size_t first, size_t K, int mask, std::vector<CmapSpan>* spans, long long* n,
                     int64_t* empty_keyframes) {
  tlx::span_range_table(P.kf.data(), P.kf.size(), first, K, mask, spans, n, empty_keyframes);
}

int SpanUpload::upload(tloam_ctx* c, const std::vector<CmapSpan>& spans, long long n, const double* poses, size_t K, SpanInput* in) {
  HIPC(c, span.reserve(spans.size())); HIPC(c, pose.reserve(std::max<size_t>(16 * K, 16)));
  HIPC(c, hipMemcpyAsync(span.p, spans.data(), sizeof(CmapSpan) * spans.size(), hipMemcpyHostToDevice, c->stream));
  if (K) HIPC(c, hipMemcpyAsync(pose.p, poses, sizeof(double) * 16 * K, hipMemcpyHostToDevice, c->stream));
  *in = SpanInput{c->place.arena.p, span.p, (int)spans.size() - 1, (int)K, n, pose.p};
  return TLOAM_OK;
}

int cmap_side_range(const tloam_ctx* c, bool ran, size_t first, size_t count) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const CmapState& M = c->cmap;
  if (!M.built || !ran) return TLOAM_E_NOT_READY;
  const size_t nv = (size_t)M.info.n_voxels;
  if (first > nv || count > nv - first) return TLOAM_E_INVALID;
  return TLOAM_OK;
}

}  // namespace tlh

extern "C" {

void tloam_closed_map_default_config(tloam_closed_map_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->voxel = 1.0;
  cfg->origin[0] = cfg->origin[1] = cfg->origin[2] = 0.0;
  cfg->cloud_mask = 0xF0;
  cfg->reserve_voxels = 0;
}

int tloam_closed_map_configure(tloam_ctx* c, const tloam_closed_map_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_config want = cfg_or_default(cfg, tloam_closed_map_default_config);
  if (!cmap_config_ok(want)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  M.drop();
  if (M.rows.cap) {   // (the next build reserves what the new configuration asks for)
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    M.rows = VoxelRowStore();
  }
  M.cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_info(tloam_ctx* c, tloam_closed_map_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.info;
  info->capacity_voxels = (int64_t)c->cmap.rows.cap;
  return TLOAM_OK;
}

int tloam_closed_map_build(tloam_ctx* c, int pose_source, const double* poses, size_t n_poses, tloam_closed_map_info* info) {
  if (!cmap_on(c) || pose_source < TLOAM_CLOSED_MAP_POSES_STORED || pose_source > TLOAM_CLOSED_MAP_POSES_CALLER)
    return TLOAM_E_INVALID;
  if (c->cmap.detached) return TLOAM_E_NOT_READY;   // (loaded without its clouds: DESIGN.md 25)
  const PlaceState& P = c->place;
  const GraphState& G = c->graph;
  const size_t K = P.kf.size();
  // the pose rule is the extension's over the whole range (tl_extend_host.hpp): one body, so that an extension's rows are those
  // of a build under the same poses
  const size_t nc = G.corrected.size() / 16;
  std::vector<double> used;
  const int prc = tlx::extend_poses(
      pose_source, poses, n_poses, 0, K, G.have, nc,
      [&](size_t k, double* dst) { memcpy(dst, P.kf[k].pose, sizeof(double) * 16); },
      [&](size_t k, double* dst) { memcpy(dst, &G.corrected[16 * k], sizeof(double) * 16); },
      [&](size_t k, double* dst) { graph_correct_pose(c, nc - 1, P.kf[k].pose, dst); },   // a keyframe added since the optimise
      [&](const double* pose) { Pose unused; return pose_from_matrix(pose, &unused); },   // (the rigid test of tloam_graph_solve)
      &used);
  if (prc != TLOAM_OK) return prc;
  CmapState& M = c->cmap;
  M.drop();   // from here on a failure leaves the closed map empty
  tloam_closed_map_info I;
  memset(&I, 0, sizeof(I));
  I.n_keyframes = (int64_t)K;
  I.pose_source = pose_source;
  const int rc = build_body(c, used, I);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);   // (nothing of the build is in flight when its staging goes)
    return rc;
  }
  M.info = I;
  M.poses.swap(used);
  M.built = true;
  if (info) {
    *info = I;
    info->capacity_voxels = (int64_t)M.rows.cap;
  }
  return TLOAM_OK;
}

int tloam_closed_map_read(tloam_ctx* c, size_t first, size_t count, double* centroids_aos, int64_t* counts) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built) return TLOAM_E_NOT_READY;
  return voxel_rows_read(c, voxel_rows_of(M, (size_t)M.info.n_voxels, "closed map"), first, count, centroids_aos, counts);
}

int tloam_closed_map_read_box(tloam_ctx* c, const double lo[3], const double hi[3], int64_t min_count, size_t capacity, size_t* n,
                              double* centroids_aos, int64_t* counts) {
  if (n) *n = 0;
  if (!c || !lo || !hi || !n || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built) return TLOAM_E_NOT_READY;
  return voxel_rows_read_box(c, voxel_rows_of(M, (size_t)M.info.n_voxels, "closed map"), lo, hi, min_count, capacity, n,
                             centroids_aos, counts, "k_vmap_box", {},
                             [&](const VmapReadArgs& A) { launch_vmap_read_box(A, c->stream); });
}

int tloam_closed_map_read_poses(tloam_ctx* c, size_t first, size_t count, double* poses) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const CmapState& M = c->cmap;
  if (!M.built) return TLOAM_E_NOT_READY;
  const size_t K = M.poses.size() / 16;
  if (first > K || count > K - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!poses) return TLOAM_E_INVALID;
  memcpy(poses, M.poses.data() + 16 * first, sizeof(double) * 16 * count);
  return TLOAM_OK;
}

}  // extern "C"
