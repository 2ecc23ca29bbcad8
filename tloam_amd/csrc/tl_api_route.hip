// tl_api_route.hip -- C ABI of the route through the closed map (include/tloam_hip.h: tloam_closed_map_route_*, _get_route_info,
// _read_route; kernels in tl_route.hip; the tile, byte and bound arithmetic in tl_tile_box.hpp; need in
// tl_clear_box.hpp, the one function the clearance's segments use).
//
// The field is a RouteState inside the clearance's ClearState: a build seeds it from the clearance field and the goals, enqueues
// rounds_per_wait rounds of the tiled relaxation between two waits and stops when a round marked no tile; the point and path
// queries go through the scan-form runner (cmap_scan_call); the column form runs the same relaxation over the layer the
// clearance's column call computes.  Nothing of the closed map, of the free-space grid, of the clearance field or of anything
// else in the context is written.
#include <math.h>

#include "tl_clear_box.hpp"
#include "tl_ctx.hpp"
#include "tl_free_box.hpp"

using namespace tl;

namespace {

using ClearState = CmapState::FreeState::ClearState;
using RouteState = ClearState::RouteState;

bool route_config_ok(const tloam_closed_map_route_config& m) {
  return m.max_bytes >= 4 && m.max_rounds >= 1 && m.rounds_per_wait >= 1 && m.rounds_per_wait <= kTileMaxBatch;
}

// the context, the grid, the clearance field and the route field checked for a query of the route
int route_ready(const tloam_ctx* c) {
  const int rc = free_read_ready(c);
  if (rc != TLOAM_OK) return rc;
  return c->cmap.free.clear.have && c->cmap.free.clear.route.have ? TLOAM_OK : TLOAM_E_NOT_READY;
}

// What a build and a column call share, their buffers reserved and their arguments checked: the goals uploaded, the seed, the
// rounds in batches of rounds_per_wait with one wait each, the count.  *info filled on TLOAM_OK; on a failure launches may be
// in flight: the caller drains the stream.
int route_run(tloam_ctx* c, const char* who, const TileField& f, const tlt::TileBox& B, const unsigned short* d2, int64_t need,
              bool flat, unsigned* flags, const double* goals_aos, size_t n, const double* pose, tloam_closed_map_route_info* info) {
  CmapState& M = c->cmap;
  RouteState& Rt = M.free.clear.route;
  unsigned long long* ctl = Rt.ctl.p;
  const size_t ntiles = (size_t)B.ntiles;
  HIPC(c, hipMemcpyAsync(M.loc_pts.p, goals_aos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemsetAsync(flags, 0, sizeof(unsigned) * 2 * ntiles, c->stream));
  HIPC(c, hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * kRouteCtl, c->stream));
  RouteSeedArgs S;
  memset(&S, 0, sizeof(S));
  S.f = f;
  S.d2 = d2;
  S.need = (int)std::max<int64_t>(need, 1);
  S.flat = flat ? 1 : 0;
  S.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) S.origin[a] = M.cfg.origin[a];
  S.goals.pts = M.loc_pts.p;
  S.goals.n = (long long)n;
  if (pose) memcpy(S.goals.M, pose, sizeof(S.goals.M));
  S.posed = pose ? 1 : 0;
  S.next = flags;
  S.ctl = ctl;
  launch_route_seed(S, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long head[8] = {0};   // the goals' marks are the first round's tiles
  TileRounds r;
  const int rc = tile_rounds(c, who, "field", Rt.cfg.max_rounds, Rt.cfg.rounds_per_wait, f, flags, ntiles, ctl + 8, launch_route_round,
                             ctl, head, 8, &r);
  if (rc != TLOAM_OK) return rc;
  launch_route_count(f, ctl + 4, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long w[4];
  HIPC(c, hipMemcpyAsync(w, ctl + 4, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  *info = tloam_closed_map_route_info{};
  for (int a = 0; a < 3; ++a) { info->lo_cells[a] = f.lo[a]; info->n_cells[a] = B.n[a]; }
  info->bytes = (int64_t)B.bytes;
  info->need = need;
  info->goals_accepted = (int64_t)head[0];
  info->goals_rejected = (int64_t)head[1];
  info->traversable_cells = (int64_t)w[0];
  info->reached_cells = (int64_t)w[1];
  info->sum_cost = (int64_t)w[2];
  info->max_cost = (int64_t)w[3];
  info->tile_updates = (int64_t)head[2] + r.updates;
  info->rounds = (int32_t)r.rounds;
  info->launches = (int32_t)(2 + r.enqueued + 1);
  info->waits = r.waits + 1;   // the rounds', and the count's
  return TLOAM_OK;
}

}  // namespace

extern "C" {

void tloam_closed_map_route_default_config(tloam_closed_map_route_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_bytes = (int64_t)1 << 30;
  cfg->max_rounds = 65536;
  cfg->rounds_per_wait = 16;
}

int tloam_closed_map_route_configure(tloam_ctx* c, const tloam_closed_map_route_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_route_config want = cfg_or_default(cfg, tloam_closed_map_route_default_config);
  if (!route_config_ok(want)) return TLOAM_E_INVALID;
  RouteState& Rt = c->cmap.free.clear.route;
  Rt.drop();
  Rt.cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_route_info(tloam_ctx* c, tloam_closed_map_route_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.free.clear.route.info;
  return TLOAM_OK;
}

int tloam_closed_map_route_build(tloam_ctx* c, const double* goals_aos, size_t n, const double* pose, double radius,
                                 tloam_closed_map_route_info* info) {
  if (!c || c->nranks > 1 || !goals_aos || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  ClearState& C = M.free.clear;
  RouteState& Rt = C.route;
  if (!C.have) return TLOAM_E_NOT_READY;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  int64_t need = 0;
  if (!tlc::need_d2(radius, M.cfg.voxel, C.field.R, &need)) return TLOAM_E_INVALID;
  const int64_t cells[3] = {C.field.n[0], C.field.n[1], C.field.n[2]};
  tlt::TileBox B;
  if (!tlt::make_box(cells, Rt.cfg.max_bytes, tlt::kRouteCellsBelow, &B)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (Rt.cost.cap < (size_t)B.cells || Rt.flags.cap < 2 * (size_t)B.ntiles || Rt.ctl.cap < (size_t)kRouteCtl || M.loc_pts.cap < 3 * n)
    HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, Rt.cost.reserve((size_t)B.cells));   // (a failure leaves the previous field: the same box has the same size)
  HIPC(c, Rt.flags.reserve(2 * (size_t)B.ntiles));
  HIPC(c, Rt.ctl.reserve(kRouteCtl));
  HIPC(c, M.loc_pts.reserve(3 * n));
  const TileField f = field_of(B, C.field.lo, Rt.cost.p);
  // from here on the previous field is gone
  Rt.have = false;
  Rt.info = tloam_closed_map_route_info{};
  Rt.field = TileField{};
  tloam_closed_map_route_info got;
  const int rc = route_run(c, "tloam_closed_map_route_build", f, B, C.field.d2, need, false, Rt.flags.p, goals_aos, n, pose, &got);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);   // the stream drained, the field (half relaxed, perhaps) gone
    Rt.drop();
    return rc;
  }
  Rt.field = f;
  Rt.info = got;
  Rt.have = true;
  if (info) *info = got;
  return TLOAM_OK;
}

int tloam_closed_map_read_route(tloam_ctx* c, size_t first, size_t count, uint32_t* cost) {
  const int ready = route_ready(c);
  if (ready != TLOAM_OK) return ready;
  const RouteState& Rt = c->cmap.free.clear.route;
  const size_t cells = (size_t)Rt.field.cells;
  if (first > cells || count > cells - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!cost) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(cost, Rt.field.v + first, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_route_points(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, uint32_t* cost_out,
                                  double* distance_out, int64_t* counts_out) {
  if (!c || c->nranks > 1 || !points_aos || !cost_out || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const int ready = route_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  RouteState& Rt = M.free.clear.route;
  unsigned long long w[4];
  int prepared = 0;
  const int rc = cmap_scan_call(
      c, CmapScanCall{points_aos, n, pose, false, &M.scan_ctl, 4, w}, &prepared,
      [&](auto room) -> int {
        HIPC(c, room(Rt.out_u32, n));
        if (distance_out) HIPC(c, room(Rt.out_f64, n));
        return TLOAM_OK;
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        RoutePointsArgs A;
        memset(&A, 0, sizeof(A));
        A.f = Rt.field;
        A.voxel = grid.voxel;
        for (int a = 0; a < 3; ++a) A.origin[a] = grid.origin[a];
        A.scan = scan;
        A.posed = pose ? 1 : 0;
        A.cost = Rt.out_u32.p;
        A.distance = distance_out ? Rt.out_f64.p : nullptr;
        A.ctl = M.scan_ctl.p;
        launch_route_points(A, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(cost_out, Rt.out_u32.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (distance_out) HIPC(c, hipMemcpyAsync(distance_out, Rt.out_f64.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
  if (rc != TLOAM_OK) return rc;
  if (counts_out)
    for (int k = 0; k < 4; ++k) counts_out[k] = (int64_t)w[k];
  return TLOAM_OK;
}

int tloam_closed_map_route_paths(tloam_ctx* c, const double* starts_aos, size_t n, const double* pose, size_t max_cells,
                                 uint8_t* status_out, int32_t* n_cells_out, uint32_t* cost_out, double* centres_aos_out) {
  if (!c || c->nranks > 1 || !starts_aos || !status_out || !n_cells_out || !cost_out || !centres_aos_out || n == 0 || n > kMaxPoints ||
      max_cells == 0 || max_cells > (size_t)INT32_MAX)
    return TLOAM_E_INVALID;
  const int ready = route_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  RouteState& Rt = M.free.clear.route;
  uint64_t waypoints = 0;
  if (!tlt::path_room(n, max_cells, Rt.cfg.max_bytes, &waypoints)) return TLOAM_E_INVALID;
  int prepared = 0;
  return cmap_scan_call(
      c, CmapScanCall{starts_aos, n, pose, false, nullptr, 0, nullptr}, &prepared,
      [&](auto room) -> int {
        HIPC(c, room(M.scan_u8, n));
        HIPC(c, room(Rt.out_i32, n));
        HIPC(c, room(Rt.out_u32, n));
        HIPC(c, room(Rt.out_f64, 3 * (size_t)waypoints));
        return TLOAM_OK;
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        HIPC(c, hipMemsetAsync(Rt.out_f64.p, 0, sizeof(double) * 3 * (size_t)waypoints, c->stream));
        RoutePathsArgs A;
        memset(&A, 0, sizeof(A));
        A.f = Rt.field;
        A.voxel = grid.voxel;
        for (int a = 0; a < 3; ++a) A.origin[a] = grid.origin[a];
        A.scan = scan;
        A.posed = pose ? 1 : 0;
        A.max_cells = (long long)max_cells;
        A.status = M.scan_u8.p;
        A.n_cells = Rt.out_i32.p;
        A.cost = Rt.out_u32.p;
        A.centres = Rt.out_f64.p;
        launch_route_paths(A, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(status_out, M.scan_u8.p, n, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(n_cells_out, Rt.out_i32.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(cost_out, Rt.out_u32.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(centres_aos_out, Rt.out_f64.p, sizeof(double) * 3 * (size_t)waypoints, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
}

int tloam_closed_map_route_columns(tloam_ctx* c, double z_lo, double z_hi, int64_t min_free, const double* goals_aos, size_t n,
                                   const double* pose, double radius, uint8_t* state_out, uint16_t* d2_out, uint32_t* cost_out,
                                   size_t capacity, size_t* nx, size_t* ny, tloam_closed_map_route_info* info) {
  if (nx) *nx = 0;
  if (ny) *ny = 0;
  if (!c || c->nranks > 1 || !nx || !ny || min_free < 1 || !goals_aos || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  CmapState::FreeState& F = M.free;
  ClearState& C = F.clear;
  RouteState& Rt = C.route;
  int R = 0;
  if (!tlc::radius_cells(C.cfg.max_distance, M.cfg.voxel, &R)) return TLOAM_E_INVALID;
  int64_t z0, z1;
  if (!tlf::z_band(z_lo, z_hi, M.cfg.origin[2], M.cfg.voxel, F.grid.blo[2], F.grid.nb[2], &z0, &z1)) return TLOAM_E_INVALID;
  const size_t cx = 4 * (size_t)F.grid.nb[0], cy = 4 * (size_t)F.grid.nb[1], cols = cx * cy;   // (nb <= 2^19 each: no overflow)
  *nx = cx;
  *ny = cy;
  if (capacity < cols || !cost_out) return TLOAM_E_INVALID;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  int64_t need = 0;
  if (!tlc::need_d2(radius, M.cfg.voxel, R, &need)) return TLOAM_E_INVALID;
  if (cols > (uint64_t)C.cfg.max_bytes / 4u) return TLOAM_E_INVALID;   // the clearance's two layers, as its column call holds them
  const int64_t cells[3] = {(int64_t)cx, (int64_t)cy, 1};
  tlt::TileBox B;
  if (!tlt::make_box(cells, Rt.cfg.max_bytes, tlt::kRouteCellsBelow, &B)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (M.scan_u8.cap < cols || C.col_a.cap < cols || C.col_b.cap < cols || Rt.col_cost.cap < cols || Rt.col_flags.cap < 2 * (size_t)B.ntiles ||
      Rt.ctl.cap < (size_t)kRouteCtl || M.loc_pts.cap < 3 * n)
    HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, M.scan_u8.reserve(cols));
  HIPC(c, C.col_a.reserve(cols));
  HIPC(c, C.col_b.reserve(cols));
  HIPC(c, Rt.col_cost.reserve(cols));
  HIPC(c, Rt.col_flags.reserve(2 * (size_t)B.ntiles));
  HIPC(c, Rt.ctl.reserve(kRouteCtl));
  HIPC(c, M.loc_pts.reserve(3 * n));
  // the clearance's column call, launch for launch: the states, then the layer of d2
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
  const int lo[3] = {4 * F.grid.blo[0], 4 * F.grid.blo[1], 0};
  const TileField f = field_of(B, lo, Rt.col_cost.p);
  tloam_closed_map_route_info got;
  int rc = TLOAM_OK;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    rc = route_run(c, "tloam_closed_map_route_columns", f, B, C.col_a.p, need, true, Rt.col_flags.p, goals_aos, n, pose, &got);
    if (rc == TLOAM_OK && state_out) e = hipMemcpyAsync(state_out, M.scan_u8.p, cols, hipMemcpyDeviceToHost, c->stream);
    if (rc == TLOAM_OK && e == hipSuccess && d2_out)
      e = hipMemcpyAsync(d2_out, C.col_a.p, sizeof(uint16_t) * cols, hipMemcpyDeviceToHost, c->stream);
    if (rc == TLOAM_OK && e == hipSuccess)
      e = hipMemcpyAsync(cost_out, Rt.col_cost.p, sizeof(uint32_t) * cols, hipMemcpyDeviceToHost, c->stream);
  }
  const hipError_t waited = hipStreamSynchronize(c->stream);   // (nothing of the call stays in flight, whatever failed)
  if (rc != TLOAM_OK) return rc;
  if (e == hipSuccess) e = waited;
  if (e != hipSuccess) {
    c->last_error = std::string("tloam_closed_map_route_columns: ") + hipGetErrorString(e);
    return TLOAM_E_HIP;
  }
  got.launches += 4;   // the states, and the layer's seed | x | y
  got.waits += 1;
  if (info) *info = got;
  return TLOAM_OK;
}

}  // extern "C"
