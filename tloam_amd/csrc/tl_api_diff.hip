// tl_api_diff.hip -- C ABI of a scan diffed against the closed map (include/tloam_hip.h: tloam_closed_map_diff*, _read_diff,
// _read_gone; kernels in tl_diff.hip).
//
// A diff takes the built closed map with its surfels (CmapState: its rows, its table, the localiser's voxel records, the
// carve's counts when the gate is on) and goes through the scan-form runner (tl_ctx.hpp: cmap_scan_call): the scan uploaded
// where the localiser's goes, the records' rebuild enqueued when they are stale, the diff's launches on the context's stream,
// one wait, for the counters, the labels and the ids.  The pose check is the runner's neighbour pose_finite_rigid.  The counts
// through and hits live beside the rows in id order and go with the closed map (CmapState::drop).  Nothing of the closed map, of
// a carve, of the surfels or of anything else in the context is written, so a detached (loaded) map is diffed like any other.
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

bool diff_config_ok(const tloam_closed_map_diff_config& m) {
  return m.max_range > 0.0 && std::isfinite(m.max_range) && m.end_margin >= 0.0 && std::isfinite(m.end_margin) && m.radius > 0.0 &&
         m.plane_tol >= 0.0 && std::isfinite(m.plane_tol) && m.near >= 0.0 && std::isfinite(m.near) && m.min_miss >= 0 &&
         m.miss_ratio == m.miss_ratio && (m.carve_gate == 0 || m.carve_gate == 1);
}

// the enqueue and the wait of a diff whose arguments have been checked; ctl: the control words as the launches left them
int diff_body(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, bool fresh, bool clear_launch, uint8_t* labels,
              int32_t* ids, unsigned long long ctl[kDiffCtl], int* prepared, int* launches) {
  CmapState& M = c->cmap;
  const tloam_closed_map_diff_config& g = M.diff_cfg;
  const size_t cap = std::max<size_t>((size_t)M.info.n_voxels, 1);
  return cmap_scan_call(
      c, CmapScanCall{points_aos, n, pose, true, &M.scan_ctl, kDiffCtl, ctl}, prepared,
      [&](auto room) -> int {
        HIPC(c, room(M.scan_u8, n));
        if (ids) HIPC(c, room(M.scan_ids, n));
        HIPC(c, room(M.diff_through, cap)); HIPC(c, room(M.diff_hits, cap));
        return TLOAM_OK;
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        if (fresh && !clear_launch) {   // accumulating into nothing: the counts start at zero without a launch of their own
          HIPC(c, hipMemsetAsync(M.diff_through.p, 0, sizeof(unsigned long long) * cap, c->stream));
          HIPC(c, hipMemsetAsync(M.diff_hits.p, 0, sizeof(unsigned long long) * cap, c->stream));
        }
        DiffWork W;
        memset(&W, 0, sizeof(W));
        W.scan = scan;
        W.grid = grid;
        W.max_range = g.max_range; W.end_margin = g.end_margin; W.radius2 = g.radius * g.radius;
        W.plane_tol = g.plane_tol; W.near2 = g.near * g.near;
        W.gate = CarveGate{(const long long*)M.miss.p, 1, g.min_miss, g.miss_ratio, g.carve_gate, 0};
        W.rec = M.loc_rec.p;
        W.through = M.diff_through.p; W.hits = M.diff_hits.p;
        W.labels = M.scan_u8.p;
        W.ids = ids ? M.scan_ids.p : nullptr;
        W.ctl = M.scan_ctl.p;
        *launches = launch_diff(W, clear_launch, c->stream) + *prepared;
        return TLOAM_OK;
      },
      [&]() -> int {
        if (labels) HIPC(c, hipMemcpyAsync(labels, M.scan_u8.p, n, hipMemcpyDeviceToHost, c->stream));
        if (ids) HIPC(c, hipMemcpyAsync(ids, M.scan_ids.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
}

}  // namespace

extern "C" {

void tloam_closed_map_diff_default_config(tloam_closed_map_diff_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_range = 60.0;
  cfg->end_margin = 1.0;
  cfg->radius = 0.25;
  cfg->plane_tol = 0.1;
  cfg->near = 0.5;
  cfg->min_miss = 3;
  cfg->miss_ratio = 1.0;
  cfg->carve_gate = 0;
}

int tloam_closed_map_diff_configure(tloam_ctx* c, const tloam_closed_map_diff_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  tloam_closed_map_diff_config want = cfg_or_default(cfg, tloam_closed_map_diff_default_config);
  if (!diff_config_ok(want)) return TLOAM_E_INVALID;
  want.reserved0 = 0;
  c->cmap.drop_diff();
  c->cmap.diff_cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_diff_info(tloam_ctx* c, tloam_closed_map_diff_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.diff_info;
  return TLOAM_OK;
}

int tloam_closed_map_diff(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, int flags, uint8_t* labels,
                          int32_t* ids, tloam_closed_map_diff_info* info) {
  if (!c || c->nranks > 1 || !points_aos || !pose || n == 0 || n > kMaxPoints || (flags & ~TLOAM_DIFF_ACCUMULATE))
    return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built || !M.surfeled || (M.diff_cfg.carve_gate && !M.carved)) return TLOAM_E_NOT_READY;
  if (!pose_finite_rigid(pose)) return TLOAM_E_INVALID;   // (only the check: the diff runs at the matrix as it stands)
  const bool accumulate = (flags & TLOAM_DIFF_ACCUMULATE) != 0;
  const bool fresh = !accumulate || !M.diffed;   // the counts start at zero
  unsigned long long ctl[kDiffCtl];
  int prepared = 0, launches = 0;
  const int rc = diff_body(c, points_aos, n, pose, fresh, !accumulate, labels, ids, ctl, &prepared, &launches);
  if (rc != TLOAM_OK) {   // (the runner has drained the stream) its counts are gone
    M.drop_diff();
    return rc;
  }
  tloam_closed_map_diff_info I;
  memset(&I, 0, sizeof(I));
  I.n_points = (int64_t)n;
  I.n_invalid = (int64_t)ctl[0]; I.n_surface = (int64_t)ctl[1]; I.n_occupied = (int64_t)ctl[2]; I.n_new = (int64_t)ctl[3];
  I.rays = (int64_t)n;
  I.skipped_rays = (int64_t)ctl[4]; I.steps = (int64_t)ctl[5]; I.tested = (int64_t)ctl[6];
  I.through = (int64_t)ctl[7]; I.voxels_through = (int64_t)ctl[8]; I.voxels_hit = (int64_t)ctl[9];
  I.scans = fresh ? 1 : M.diff_info.scans + 1;
  I.launches = launches;
  I.prepared = prepared;
  I.cleared = accumulate ? 0 : 1;
  M.diff_info = I;
  M.diffed = true;
  if (info) *info = I;
  return TLOAM_OK;
}

int tloam_closed_map_read_diff(tloam_ctx* c, size_t first, size_t count, int64_t* through, int64_t* hits) {
  const int rc = cmap_side_range(c, c && c->cmap.diffed, first, count);
  if (rc != TLOAM_OK || count == 0) return rc;
  const CmapState& M = c->cmap;
  HIPC(c, hipSetDevice(c->device));
  if (through) HIPC(c, hipMemcpyAsync(through, M.diff_through.p + first, sizeof(int64_t) * count, hipMemcpyDeviceToHost, c->stream));
  if (hits) HIPC(c, hipMemcpyAsync(hits, M.diff_hits.p + first, sizeof(int64_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_read_gone(tloam_ctx* c, const double* lo, const double* hi, int64_t min_through, double gone_ratio,
                               size_t capacity, size_t* n, double* centroids_aos, int64_t* counts, int64_t* through, int64_t* hits) {
  if (n) *n = 0;
  if (!c || !n || (lo == nullptr) != (hi == nullptr) || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built || !M.diffed) return TLOAM_E_NOT_READY;
  DiffReadArgs A;
  memset(&A, 0, sizeof(A));
  A.through = (const long long*)M.diff_through.p;
  A.hits = (const long long*)M.diff_hits.p;
  A.min_through = min_through;
  A.gone_ratio = gone_ratio;
  A.boxed = lo ? 1 : 0;
  return voxel_rows_read_box(c, voxel_rows_of(M, (size_t)M.info.n_voxels, "closed map"), lo, hi, 1, capacity, n, centroids_aos,
                             counts, "k_diff_box",
                             {BoxColumn{through, &M.rd_through, 1, sizeof(int64_t)}, BoxColumn{hits, &M.rd_hits, 1, sizeof(int64_t)}},
                             [&](const VmapReadArgs& rows) {
                               A.rows = rows;
                               A.out_through = (long long*)M.rd_through.p;
                               A.out_hits = (long long*)M.rd_hits.p;
                               launch_diff_read(A, c->stream);
                             });
}

}  // extern "C"
