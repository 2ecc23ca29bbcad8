// tl_api_carve.hip -- C ABI of the closed map's carve (include/tloam_hip.h: tloam_closed_map_carve*, _read_misses,
// _read_carved; kernels in tl_carve.hip).
//
// A carve takes the built closed map (CmapState: its rows, its table, the poses it was built with) and the host's keyframe
// table (PlaceState::kf) for the build's keyframes, uploads one span table for the ray mask and the poses, and enqueues three
// launches on the context's stream; it waits once, for the counters.  The counts M live beside the rows in id order and go with
// the closed map (CmapState::drop).  Nothing of the closed map or of anything else in the context is written.
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

bool carve_config_ok(const tloam_closed_map_carve_config& m) {
  return m.max_range > 0.0 && std::isfinite(m.max_range) && m.end_margin >= 0.0 && std::isfinite(m.end_margin) && m.radius > 0.0 &&
         m.ray_mask >= 0 && m.ray_mask <= 0xFF;
}

// the enqueue, the wait and the counters of a carve; the previous counts have been dropped
int carve_body(tloam_ctx* c, tloam_closed_map_carve_info& I) {
  CmapState& M = c->cmap;
  const tloam_closed_map_carve_config& g = M.carve_cfg;
  const size_t nv = std::max<size_t>((size_t)M.info.n_voxels, 1);
  CmapPassOut R;
  const int rc = cmap_pass<CarveWork>(
      c, g.ray_mask ? g.ray_mask : M.cfg.cloud_mask, M.carve_ctl,
      [&]() -> int {
        if (M.miss.cap < nv || M.carve_ctl.cap < 8) HIPC(c, hipStreamSynchronize(c->stream));   // (the counts replaced may still be read)
        HIPC(c, M.miss.reserve(nv)); HIPC(c, M.carve_ctl.reserve(8));
        return TLOAM_OK;
      },
      [&](CarveWork& W) {
        W.max_range = g.max_range;
        W.end_margin = g.end_margin;
        W.radius2 = g.radius * g.radius;
        W.miss = M.miss.p;
        return launch_carve(W, c->stream);
      },
      &R);
  if (rc != TLOAM_OK) return rc;
  I.launches = R.launches;
  I.n_keyframes = (int64_t)R.K;
  I.n_rays = (int64_t)R.n;
  I.skipped_rays = (int64_t)R.ctl[0];
  I.steps = (int64_t)R.ctl[1];
  I.tested = (int64_t)R.ctl[2];
  I.misses = (int64_t)R.ctl[3];
  I.voxels_missed = (int64_t)R.ctl[4];
  return TLOAM_OK;
}

}  // namespace

namespace tlh {
bool carve_config_valid(const tloam_closed_map_carve_config& cfg) { return carve_config_ok(cfg); }
}  // namespace tlh

extern "C" {

void tloam_closed_map_carve_default_config(tloam_closed_map_carve_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_range = 60.0;
  cfg->end_margin = 1.0;
  cfg->radius = 0.25;
  cfg->ray_mask = 0;
}

int tloam_closed_map_carve_configure(tloam_ctx* c, const tloam_closed_map_carve_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_carve_config want = cfg_or_default(cfg, tloam_closed_map_carve_default_config);
  if (!carve_config_ok(want)) return TLOAM_E_INVALID;
  c->cmap.drop_carve();
  c->cmap.carve_cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_carve_info(tloam_ctx* c, tloam_closed_map_carve_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.carve_info;
  return TLOAM_OK;
}

int tloam_closed_map_carve(tloam_ctx* c, tloam_closed_map_carve_info* info) {
  if (c && c->nranks == 1 && c->cmap.detached) return TLOAM_E_NOT_READY;   // (loaded without its clouds: DESIGN.md 25)
  return cmap_pass_entry(c, &CmapState::drop_carve, &CmapState::carve_info, &CmapState::carved, info,
                         [&](tloam_closed_map_carve_info& I) { return carve_body(c, I); });
}

int tloam_closed_map_read_misses(tloam_ctx* c, size_t first, size_t count, int64_t* misses) {
  const int rc = cmap_side_range(c, c && c->cmap.carved, first, count);
  if (rc != TLOAM_OK || count == 0) return rc;
  if (!misses) return TLOAM_E_INVALID;
  const CmapState& M = c->cmap;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(misses, M.miss.p + first, sizeof(int64_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_read_carved(tloam_ctx* c, const double* lo, const double* hi, int64_t min_count, int64_t min_miss,
                                 double miss_ratio, size_t capacity, size_t* n, double* centroids_aos, int64_t* counts,
                                 int64_t* misses) {
  if (n) *n = 0;
  if (!c || !n || (lo == nullptr) != (hi == nullptr) || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built || !M.carved) return TLOAM_E_NOT_READY;
  CarveReadArgs A;
  A.gate = CarveGate{(const long long*)M.miss.p, min_count, min_miss, miss_ratio, 1, 0};   // (min_count: the box read's own test)
  A.boxed = lo ? 1 : 0;
  return voxel_rows_read_box(c, voxel_rows_of(M, (size_t)M.info.n_voxels, "closed map"), lo, hi, min_count, capacity, n,
                             centroids_aos, counts, "k_carve_box", {BoxColumn{misses, &M.rd_m, 1, sizeof(int64_t)}},
                             [&](const VmapReadArgs& rows) {
                               A.rows = rows;
                               A.out_m = (long long*)M.rd_m.p;
                               launch_carve_read(A, c->stream);
                             });
}

}  // extern "C"
