// tl_api_raycast.hip -- C ABI of the closed map's ray-cast (include/tloam_hip.h: tloam_closed_map_raycast*, DESIGN.md section 28;
// the kernel in tl_raycast.hip).
//
// A ray-cast takes the built closed map with its surfels (CmapState: its rows, its table, the localiser's voxel records, the
// carve's counts when the gate is on), uploads the segment ends where the localiser's scan goes, enqueues the records' rebuild
// when they are stale and the one launch on the context's stream, and waits once, for the counters, the statuses, the ranges and
// the ids.  Nothing of the closed map, of a carve, of the surfels, of a diff's counts or of anything else in the context is
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
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, M.loc_pts.reserve(3 * n)); HIPC(c, M.raycast_status.reserve(n)); HIPC(c, M.raycast_range.reserve(n));
  if (ids) HIPC(c, M.raycast_ids.reserve(n));
  HIPC(c, M.raycast_ctl.reserve(kRaycastCtl));
  HIPC(c, hipMemcpyAsync(M.loc_pts.p, ends_aos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  const int rc = loc_records_prepare(c, prepared);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, hipMemsetAsync(M.raycast_ctl.p, 0, sizeof(unsigned long long) * kRaycastCtl, c->stream));
  RaycastWork W;
  memset(&W, 0, sizeof(W));
  W.ends = M.loc_pts.p;
  W.n = (long long)n;
  memcpy(W.M, pose, sizeof(W.M));   // the matrix as it stands
  W.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) W.origin[a] = M.cfg.origin[a];
  W.max_range = g.max_range;
  const double radius = g.radius_cells * M.cfg.voxel;
  W.radius2 = radius * radius;
  W.min_count = g.min_count; W.min_miss = g.min_miss; W.miss_ratio = g.miss_ratio; W.gate = g.carve_gate; W.planes = g.planes;
  W.map = M.rows.view();
  W.rec = M.loc_rec.p;
  W.miss = (const long long*)M.miss.p;
  W.status = M.raycast_status.p; W.range = M.raycast_range.p;
  W.ids = ids ? M.raycast_ids.p : nullptr;
  W.ctl = M.raycast_ctl.p;
  launch_raycast(W, c->stream);
  HIPC(c, hipGetLastError());
  HIPC(c, hipMemcpyAsync(ctl, M.raycast_ctl.p, sizeof(unsigned long long) * kRaycastCtl, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipMemcpyAsync(status, M.raycast_status.p, n, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipMemcpyAsync(range, M.raycast_range.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  if (ids) HIPC(c, hipMemcpyAsync(ids, M.raycast_ids.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
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
  for (int i = 0; i < 16; ++i)
    if (!(pose[i] - pose[i] == 0.0)) return TLOAM_E_INVALID;
  Pose rigid;   // (only the check that `pose` is a rigid transform: the cast runs at the matrix as it stands)
  if (!pose_from_matrix(pose, &rigid)) return TLOAM_E_INVALID;
  unsigned long long ctl[kRaycastCtl];
  int prepared = 0;
  const int rc = raycast_body(c, ends_aos, n, pose, status, range, ids, ctl, &prepared);
  if (rc != TLOAM_OK) {   // nothing of the call stays in flight; the records are rebuilt by the next call
    (void)hipStreamSynchronize(c->stream);
    M.loc_ready = false;
    return rc;
  }
  M.loc_ready = true;
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
