// tl_api_surfel.hip -- C ABI of the closed map's surfels (include/tloam_hip.h: tloam_closed_map_surfel*, _surfels, _read_moments,
// _read_surfels, _read_surfels_box; kernels in tl_surfel.hip).
//
// A pass takes the built closed map (CmapState: its table, the poses and the cloud mask it was built with) and the host's
// keyframe table (PlaceState::kf) for the build's keyframes, uploads one span table and the poses, and enqueues four launches on
// the context's stream; it waits once, for the counters.  The sums, normals and variances live beside the rows in id order and go
// with the closed map (CmapState::drop).  Nothing of the closed map, of a carve's counts or of anything else in the context is
// written.
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

// the enqueue, the wait and the counters of a pass; the previous surfels have been dropped
int surfel_body(tloam_ctx* c, tloam_closed_map_surfel_info& I) {
  CmapState& M = c->cmap;
  const size_t cap = std::max<size_t>(M.rows.cap, 1), K1 = std::max<size_t>(M.poses.size() / 16, 1);
  CmapPassOut R;
  const int rc = cmap_pass<SurfelWork>(
      c, M.cfg.cloud_mask, M.surfel_ctl,   // the build's span table
      [&]() -> int {
        if (M.surfel_sums.cap < kSurfelSums * cap || M.surfel_over.cap < K1 || M.surfel_ctl.cap < 8)
          HIPC(c, hipStreamSynchronize(c->stream));   // (the arrays replaced may still be read)
        HIPC(c, M.surfel_sums.reserve(kSurfelSums * cap)); HIPC(c, M.surfel_nrm.reserve(3 * cap)); HIPC(c, M.surfel_ev.reserve(3 * cap));
        HIPC(c, M.surfel_over.reserve(K1)); HIPC(c, M.surfel_ctl.reserve(8));
        return TLOAM_OK;
      },
      [&](SurfelWork& W) {
        W.kf_over = M.surfel_over.p;
        W.runs = getenv("TLOAM_SURFEL_NO_RUNS") ? 0 : 1;   // A/B of the wave's run aggregation, read per pass
        W.min_points = M.surfel_cfg.min_points;
        W.sums = M.surfel_sums.p;
        W.normal = M.surfel_nrm.p;
        W.eval = M.surfel_ev.p;
        return launch_surfels(W, c->stream);
      },
      &R);
  if (rc != TLOAM_OK) return rc;
  I.launches = R.launches;
  I.n_keyframes = (int64_t)R.K;
  I.n_points = (int64_t)R.ctl[0];
  I.orphan_points = (int64_t)R.ctl[1];
  I.solved_voxels = (int64_t)R.ctl[2];
  return TLOAM_OK;
}

}  // namespace

extern "C" {

void tloam_closed_map_surfel_default_config(tloam_closed_map_surfel_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->min_points = 5;
}

int tloam_closed_map_surfel_configure(tloam_ctx* c, const tloam_closed_map_surfel_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_surfel_config want = cfg_or_default(cfg, tloam_closed_map_surfel_default_config);
  if (want.min_points < 3) return TLOAM_E_INVALID;
  c->cmap.drop_surfels();
  c->cmap.surfel_cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_surfel_info(tloam_ctx* c, tloam_closed_map_surfel_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.surfel_info;
  return TLOAM_OK;
}

int tloam_closed_map_surfels(tloam_ctx* c, tloam_closed_map_surfel_info* info) {
  if (c && c->nranks == 1 && c->cmap.detached) return TLOAM_E_NOT_READY;   // (loaded without its clouds: DESIGN.md 25)
  return cmap_pass_entry(c, &CmapState::drop_surfels, &CmapState::surfel_info, &CmapState::surfeled, info,
                         [&](tloam_closed_map_surfel_info& I) { return surfel_body(c, I); });
}

int tloam_closed_map_read_moments(tloam_ctx* c, size_t first, size_t count, int64_t* out) {
  const int rc = cmap_side_range(c, c && c->cmap.surfeled, first, count);
  if (rc != TLOAM_OK || count == 0) return rc;
  if (!out) return TLOAM_E_INVALID;
  const CmapState& M = c->cmap;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(out, M.surfel_sums.p + kSurfelSums * first, sizeof(int64_t) * kSurfelSums * count, hipMemcpyDeviceToHost,
                         c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_read_surfels(tloam_ctx* c, size_t first, size_t count, double* normals_aos, double* evals_aos, int64_t* counts) {
  const int rc = cmap_side_range(c, c && c->cmap.surfeled, first, count);
  if (rc != TLOAM_OK || count == 0) return rc;
  const CmapState& M = c->cmap;
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  HIPC(c, hipSetDevice(c->device));
  if (normals_aos) HIPC(c, hipMemcpyAsync(normals_aos, M.surfel_nrm.p + 3 * first, sizeof(double) * 3 * count, D2H, c->stream));
  if (evals_aos) HIPC(c, hipMemcpyAsync(evals_aos, M.surfel_ev.p + 3 * first, sizeof(double) * 3 * count, D2H, c->stream));
  std::vector<int64_t> sums(counts ? kSurfelSums * count : 0);   // Ns is the first of a voxel's thirteen sums
  if (counts)
    HIPC(c, hipMemcpyAsync(sums.data(), M.surfel_sums.p + kSurfelSums * first, sizeof(int64_t) * sums.size(), D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (counts)
    for (size_t i = 0; i < count; ++i) counts[i] = sums[kSurfelSums * i];
  return TLOAM_OK;
}

int tloam_closed_map_read_surfels_box(tloam_ctx* c, const double* lo, const double* hi, int64_t min_count, double max_sigma,
                                      double min_planarity, size_t capacity, size_t* n, double* centroids_aos, double* normals_aos,
                                      double* evals_aos, int64_t* counts) {
  if (n) *n = 0;
  if (!c || !n || (lo == nullptr) != (hi == nullptr) || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built || !M.surfeled) return TLOAM_E_NOT_READY;
  SurfelReadArgs A;
  A.sums = M.surfel_sums.p;
  A.normal = M.surfel_nrm.p;
  A.eval = M.surfel_ev.p;
  A.min_points = M.surfel_cfg.min_points;
  A.boxed = lo ? 1 : 0;
  A.max_sigma2 = max_sigma * max_sigma;
  A.min_planarity = min_planarity;
  return voxel_rows_read_box(c, voxel_rows_of(M, (size_t)M.info.n_voxels, "closed map"), lo, hi, min_count, capacity, n,
                             centroids_aos, counts, "k_surfel_box",
                             {BoxColumn{normals_aos, &M.rd_nrm, 3, sizeof(double)}, BoxColumn{evals_aos, &M.rd_ev, 3, sizeof(double)}},
                             [&](const VmapReadArgs& rows) {
                               A.rows = rows;
                               A.out_nrm = (double*)M.rd_nrm.p; A.out_ev = (double*)M.rd_ev.p;
                               launch_surfel_read(A, c->stream);
                             });
}

}  // extern "C"
