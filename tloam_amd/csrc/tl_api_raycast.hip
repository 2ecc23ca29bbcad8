// tl_api_raycast.hip -- C ABI of the closed map's ray-cast (include/tloam_hip.h: tloam_closed_map_raycast*, DESIGN.md section 28;
// the kernel in tl_raycast.hip).
//
// A ray-cast takes the built closed map with its surfels (CmapState: its rows, its table, the localiser's voxel records, the
// carve's counts when the gate is on) and goes through the scan-form runner (tl_ctx.hpp: cmap_scan_call): the segment ends
// uploaded where the localiser's scan goes, the records' rebuild enqueued when they are stale, the one launch on the context's
// stream, one wait, for the counters, the statuses, the ranges and the ids.  The pose check is pose_finite_rigid.  Nothing of the closed map, of a carve, of the surfels, of a diff's counts or of anything else in the context is
// written, so a detached (loaded) map is cast through like any other.  Stored: the configuration and the last info.
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

bool raycast_config_ok(const tloam_closed_map_raycast_config& m) {
  return m.max_range > 0.0 && std::isfinite(m.max_range) && m.radius_cells > 0.0 && m.radius_cells <= 2.0 && m.planes >= 0 &&
         m.planes <= 2 && m.min_count >= 1 && m.min_miss >= 0 && m.miss_ratio == m.miss_ratio &&
         (m.carve_gate == 0 || m.carve_gate == 1);
}

// the enqueue and the wait of a cast whose arguments have been checked; ctl: the control words as the launch left them
int raycast_body(tloam_ctx* c, const double* ends_aos, size_t n, const double* pose, uint8_t* status, double* range, int32_t* ids,
                 unsigned long long ctl[kRaycastCtl], int* prepared) {
  CmapState& M = c->cmap;
  const tloam_closed_map_raycast_config& g = M.raycast_cfg;
  return cmap_scan_call(
      c, CmapScanCall{ends_aos, n, pose, true, &M.scan_ctl, kRaycastCtl, ctl}, prepared,
      [&](auto room) -> int {
        HIPC(c, room(M.scan_u8, n)); HIPC(c, room(M.raycast_range, n));
        if (ids) HIPC(c, room(M.scan_ids, n));
        return TLOAM_OK;
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        RaycastWork W;
        memset(&W, 0, sizeof(W));
        W.scan = scan;
        W.grid = grid;
        W.max_range = g.max_range;
        const double radius = g.radius_cells * M.cfg.voxel;
        W.radius2 = radius * radius;
        W.gate = CarveGate{(const long long*)M.miss.p, g.min_count, g.min_miss, g.miss_ratio, g.carve_gate, 0};
        W.planes = g.planes;
        W.rec = M.loc_rec.p;
        W.status = M.scan_u8.p; W.range = M.raycast_range.p;
        W.ids = ids ? M.scan_ids.p : nullptr;
        W.ctl = M.scan_ctl.p;
        launch_raycast(W, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(status, M.scan_u8.p, n, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(range, M.raycast_range.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        if (ids) HIPC(c, hipMemcpyAsync(ids, M.scan_ids.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
}

}  // namespace

extern "C" {

void tloam_closed_map_raycast_default_config(tloam_closed_map_raycast_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_range = 120.0;
  cfg->radius_cells = 0.75;
  cfg->min_count = 1;
  cfg->min_miss = 3;
  cfg->miss_ratio = 1.0;
  cfg->planes = 1;
  cfg->carve_gate = 0;
}

int tloam_closed_map_raycast_configure(tloam_ctx* c, const tloam_closed_map_raycast_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_raycast_config want = cfg_or_default(cfg, tloam_closed_map_raycast_default_config);
  if (!raycast_config_ok(want)) return TLOAM_E_INVALID;
  c->cmap.drop_raycast();
  c->cmap.raycast_cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_raycast_info(tloam_ctx* c, tloam_closed_map_raycast_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.raycast_info;
  return TLOAM_OK;
}

int tloam_closed_map_raycast(tloam_ctx* c, const double* ends_aos, size_t n, const double* pose, uint8_t* status, double* range,
                             int32_t* ids, tloam_closed_map_raycast_info* info) {
  if (!c || c->nranks > 1 || !ends_aos || !pose || !status || !range || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built || !M.surfeled || (M.raycast_cfg.carve_gate && !M.carved)) return TLOAM_E_NOT_READY;
  if (!pose_finite_rigid(pose)) return TLOAM_E_INVALID;   // (only the check: the cast runs at the matrix as it stands)
  unsigned long long ctl[kRaycastCtl];
  int prepared = 0;
  const int rc = raycast_body(c, ends_aos, n, pose, status, range, ids, ctl, &prepared);
  if (rc != TLOAM_OK) return rc;
  tloam_closed_map_raycast_info I;
  memset(&I, 0, sizeof(I));
  I.rays = (int64_t)n;
  I.skipped = (int64_t)ctl[0]; I.missed = (int64_t)ctl[1]; I.hits_centroid = (int64_t)ctl[2]; I.hits_plane = (int64_t)ctl[3];
  I.steps = (int64_t)ctl[4]; I.tested = (int64_t)ctl[5];
  I.launches = 1 + prepared;
  I.prepared = prepared;
  M.raycast_info = I;
  if (info) *info = I;
  return TLOAM_OK;
}

}  // extern "C"
