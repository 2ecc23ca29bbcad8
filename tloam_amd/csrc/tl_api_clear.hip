// tl_api_clear.hip -- C ABI of the closed map's clearance (include/tloam_hip.h: tloam_closed_map_clearance_*, _get_clearance_info,
// _read_clearance; kernels in tl_clear.hip; the radius, need and byte arithmetic in tl_clear_box.hpp).
//
// The field is a ClearState inside the free space's FreeState: a build resolves the states of the grid's box as the occupancy
// query does (free_query: the one carve gate), runs the three passes and counts; the point and segment queries go through the
// scan-form runner (cmap_scan_call, as the occupancy of a scan's points); the column field is computed per call from the grid.
// Every call enqueues a fixed number of launches on the context's stream and waits once.  Nothing of the closed map, of a carve,
// of the surfels, of a diff, of the free-space grid or of anything else in the context is written.
#include <math.h>

#include "tl_clear_box.hpp"
#include "tl_ctx.hpp"
#include "tl_free_box.hpp"

using namespace tl;

namespace {

using ClearState = CmapState::FreeState::ClearState;

bool clear_config_ok(const tloam_closed_map_clearance_config& m) {
  return m.max_distance > 0.0 && std::isfinite(m.max_distance) && m.max_segment > 0.0 && std::isfinite(m.max_segment) &&
         m.max_bytes >= 2 && (m.unknown_is_obstacle == 0 || m.unknown_is_obstacle == 1);
}

// the context, the grid and the field checked for a query of the field
int clear_ready(const tloam_ctx* c) {
  const int rc = free_read_ready(c);
  if (rc != TLOAM_OK) return rc;
  return c->cmap.free.clear.have ? TLOAM_OK : TLOAM_E_NOT_READY;
}

// a build failed with its launches possibly in flight: the stream drained, the field (half written, perhaps) gone
int clear_build_failed(tloam_ctx* c, int rc) {
  (void)hipStreamSynchronize(c->stream);
  c->cmap.free.clear.drop();
  return rc;
}

}  // namespace

extern "C" {

void tloam_closed_map_clearance_default_config(tloam_closed_map_clearance_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_distance = 4.0;
  cfg->max_segment = 120.0;
  cfg->max_bytes = (int64_t)1 << 30;
  cfg->unknown_is_obstacle = 1;
}

int tloam_closed_map_clearance_configure(tloam_ctx* c, const tloam_closed_map_clearance_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  tloam_closed_map_clearance_config want = cfg_or_default(cfg, tloam_closed_map_clearance_default_config);
  if (!clear_config_ok(want)) return TLOAM_E_INVALID;
  want.reserved0 = 0;
  c->cmap.free.clear.drop();
  c->cmap.free.clear.cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_clearance_info(tloam_ctx* c, tloam_closed_map_clearance_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.free.clear.info;
  return TLOAM_OK;
}

int tloam_closed_map_clearance_build(tloam_ctx* c, tloam_closed_map_clearance_info* info) {
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  CmapState::FreeState& F = M.free;
  ClearState& C = F.clear;
  int R = 0;
  if (!tlc::radius_cells(C.cfg.max_distance, M.cfg.voxel, &R)) return TLOAM_E_INVALID;
  const int64_t nb[3] = {F.grid.nb[0], F.grid.nb[1], F.grid.nb[2]};
  tlc::ClearBox B;
  if (!tlc::make_field(nb, C.cfg.max_bytes, &B)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (C.d2.cap < (size_t)B.cells || C.tmp.cap < (size_t)B.cells) HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, C.d2.reserve((size_t)B.cells));    // (a failure leaves the previous field: the same box has the same size)
  HIPC(c, C.tmp.reserve((size_t)B.cells));
  HIPC(c, M.scan_ctl.reserve(kDiffCtl));
  ClearBuildArgs A;
  memset(&A, 0, sizeof(A));
  A.q = free_query(M);
  for (int a = 0; a < 3; ++a) { A.f.lo[a] = 4 * F.grid.blo[a]; A.f.n[a] = (int)B.n[a]; }
  A.f.cells = (long long)B.cells;
  A.f.R = R;
  A.f.wrap = C.cfg.unknown_is_obstacle;
  A.out = C.d2.p;
  A.tmp = C.tmp.p;
  A.ctl = M.scan_ctl.p;
  // from here on the previous field is gone
  C.have = false;
  C.info = tloam_closed_map_clearance_info{};
  C.route.drop();   // (the route was built from the field this build replaces: DESIGN.md section 31)
  hipError_t e = hipMemsetAsync(M.scan_ctl.p, 0, sizeof(unsigned long long) * kClearCtl, c->stream);
  int launches = 0;
  if (e == hipSuccess) {
    launches = launch_clear_build(A, c->stream);
    e = hipGetLastError();
  }
  unsigned long long w[kClearCtl];
  if (e == hipSuccess) e = hipMemcpyAsync(w, M.scan_ctl.p, sizeof(w), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    c->last_error = std::string("tloam_closed_map_clearance_build: ") + hipGetErrorString(e);
    return clear_build_failed(c, TLOAM_E_HIP);
  }
  C.field = A.f;
  C.field.d2 = C.d2.p;
  for (int a = 0; a < 3; ++a) { C.info.lo_cells[a] = A.f.lo[a]; C.info.n_cells[a] = B.n[a]; }
  C.info.bytes = (int64_t)B.bytes;
  C.info.obstacle_cells = (int64_t)w[0];
  C.info.finite_cells = (int64_t)w[1];
  C.info.sum_d2 = (int64_t)w[2];
  C.info.max_d2 = (int64_t)w[3];
  C.info.radius_cells = R;
  C.info.launches = launches;
  C.have = true;
  if (info) *info = C.info;
  return TLOAM_OK;
}

int tloam_closed_map_read_clearance(tloam_ctx* c, size_t first, size_t count, uint16_t* d2) {
  const int ready = clear_ready(c);
  if (ready != TLOAM_OK) return ready;
  const ClearState& C = c->cmap.free.clear;
  const size_t cells = (size_t)C.field.cells;
  if (first > cells || count > cells - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!d2) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(d2, C.field.d2 + first, sizeof(uint16_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_clearance_points(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, uint8_t* state_out,
                                      uint16_t* d2_out, double* distance_out, int64_t* counts_out) {
  if (!c || c->nranks > 1 || !points_aos || !state_out || !d2_out || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const int ready = clear_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  ClearState& C = M.free.clear;
  unsigned long long w[4];
  int prepared = 0;
  const int rc = cmap_scan_call(
      c, CmapScanCall{points_aos, n, pose, false, &M.scan_ctl, 4, w}, &prepared,
      [&](auto room) -> int {
        HIPC(c, room(M.scan_u8, n));
        HIPC(c, room(C.out_u16, n));
        if (distance_out) HIPC(c, room(C.out_f64, n));
        return TLOAM_OK;
      },
      [&](const MapGrid&, const ScanAt& scan) -> int {
        ClearPointsArgs A;
        memset(&A, 0, sizeof(A));
        A.q = free_query(M);
        A.f = C.field;
        A.scan = scan;
        A.posed = pose ? 1 : 0;
        A.state = M.scan_u8.p;
        A.d2 = C.out_u16.p;
        A.distance = distance_out ? C.out_f64.p : nullptr;
        A.ctl = M.scan_ctl.p;
        launch_clear_points(A, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(state_out, M.scan_u8.p, n, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(d2_out, C.out_u16.p, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (distance_out) HIPC(c, hipMemcpyAsync(distance_out, C.out_f64.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
  if (rc != TLOAM_OK) return rc;
  if (counts_out)
    for (int k = 0; k < 4; ++k) counts_out[k] = (int64_t)w[k];
  return TLOAM_OK;
}

int tloam_closed_map_clearance_segments(tloam_ctx* c, const double* starts_aos, const double* ends_aos, size_t n, const double* pose,
                                        double radius, uint8_t* status_out, uint16_t* min_d2_out, double* t_block_out,
                                        int64_t* counts_out) {
  if (!c || c->nranks > 1 || !starts_aos || !ends_aos || !status_out || !min_d2_out || n == 0 || n > kMaxPoints)
    return TLOAM_E_INVALID;
  const int ready = clear_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  ClearState& C = M.free.clear;
  int64_t need = 0;
  if (!tlc::need_d2(radius, M.cfg.voxel, C.field.R, &need)) return TLOAM_E_INVALID;
  unsigned long long w[4];
  int prepared = 0;
  const int rc = cmap_scan_call(
      c, CmapScanCall{ends_aos, n, pose, false, &M.scan_ctl, 4, w}, &prepared,
      [&](auto room) -> int {
        HIPC(c, room(C.starts, 3 * n));
        HIPC(c, room(M.scan_u8, n));
        HIPC(c, room(C.out_u16, n));
        if (t_block_out) HIPC(c, room(C.out_f64, n));
        return TLOAM_OK;
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        HIPC(c, hipMemcpyAsync(C.starts.p, starts_aos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
        ClearSegmentsArgs A;
        memset(&A, 0, sizeof(A));
        A.grid = grid;
        A.f = C.field;
        A.scan = scan;
        A.starts = C.starts.p;
        A.posed = pose ? 1 : 0;
        A.need = (int)need;
        A.max_segment = C.cfg.max_segment;
        A.status = M.scan_u8.p;
        A.min_d2 = C.out_u16.p;
        A.t_block = t_block_out ? C.out_f64.p : nullptr;
        A.ctl = M.scan_ctl.p;
        launch_clear_segments(A, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(status_out, M.scan_u8.p, n, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(min_d2_out, C.out_u16.p, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (t_block_out) HIPC(c, hipMemcpyAsync(t_block_out, C.out_f64.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
  if (rc != TLOAM_OK) return rc;
  if (counts_out)
    for (int k = 0; k < 4; ++k) counts_out[k] = (int64_t)w[k];
  return TLOAM_OK;
}

int tloam_closed_map_clearance_columns(tloam_ctx* c, double z_lo, double z_hi, int64_t min_free, uint8_t* state_out, uint16_t* d2_out,
                                       size_t capacity, size_t* nx, size_t* ny) {
  if (nx) *nx = 0;
  if (ny) *ny = 0;
  if (!c || c->nranks > 1 || !nx || !ny || min_free < 1) return TLOAM_E_INVALID;
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  CmapState::FreeState& F = M.free;
  ClearState& C = F.clear;
  int R = 0;
  if (!tlc::radius_cells(C.cfg.max_distance, M.cfg.voxel, &R)) return TLOAM_E_INVALID;
  int64_t z0, z1;
  if (!tlf::z_band(z_lo, z_hi, M.cfg.origin[2], M.cfg.voxel, F.grid.blo[2], F.grid.nb[2], &z0, &z1)) return TLOAM_E_INVALID;
  const size_t cx = 4 * (size_t)F.grid.nb[0], cy = 4 * (size_t)F.grid.nb[1], cols = cx * cy;   // (nb <= 2^19 each: no overflow)
  *nx = cx;
  *ny = cy;
  if (capacity < cols || !d2_out) return TLOAM_E_INVALID;
  if (cols > (uint64_t)C.cfg.max_bytes / 4u) return TLOAM_E_INVALID;   // the two layers, two bytes a column each, are the field's too
  HIPC(c, hipSetDevice(c->device));
  if (M.scan_u8.cap < cols || C.col_a.cap < cols || C.col_b.cap < cols) HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, M.scan_u8.reserve(cols));
  HIPC(c, C.col_a.reserve(cols));
  HIPC(c, C.col_b.reserve(cols));
  FreeColumnsArgs S;
  memset(&S, 0, sizeof(S));
  S.q = free_query(M);
  S.z0 = (int)z0;
  S.z1 = (int)z1;
  S.min_free = min_free;
  S.state = M.scan_u8.p;
  launch_free_columns(S, c->stream);
  ClearColumnsArgs A;
  memset(&A, 0, sizeof(A));
  A.state = M.scan_u8.p;
  A.nx = (int)cx;
  A.ny = (int)cy;
  A.R = R;
  A.wrap = C.cfg.unknown_is_obstacle;
  A.out = C.col_a.p;
  A.tmp = C.col_b.p;
  (void)launch_clear_columns(A, c->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && state_out) e = hipMemcpyAsync(state_out, M.scan_u8.p, cols, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d2_out, C.col_a.p, sizeof(uint16_t) * cols, hipMemcpyDeviceToHost, c->stream);
  const hipError_t waited = hipStreamSynchronize(c->stream);   // (nothing of the call stays in flight, whatever failed)
  if (e == hipSuccess) e = waited;
  if (e != hipSuccess) {
    c->last_error = std::string("tloam_closed_map_clearance_columns: ") + hipGetErrorString(e);
    return TLOAM_E_HIP;
  }
  return TLOAM_OK;
}

}  // extern "C"
