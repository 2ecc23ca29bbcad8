// tl_api_free.hip -- C ABI of the closed map's free space (include/tloam_hip.h: tloam_closed_map_free_*, _get_free_info,
// _occupancy, _read_free; kernels in tl_free.hip; the box's arithmetic in tl_free_box.hpp).
//
// The grid is a FreeState inside the closed map's state: a reset sizes it over a box of bricks and zeroes it, an add walks rays
// into it -- the keyframes' through the pass runner the carve uses (cmap_pass, over the keyframes the grid has not seen), a live
// scan's from one origin through the scan-form runner (cmap_scan_call, as the occupancy of a scan's points) -- and the reads
// resolve occupancy against the map as it is when they run, under the one carve gate (tl_common.hpp: CarveGate).  Every call enqueues a fixed number of launches on the context's stream and waits once.  Nothing of the closed
// map, of a carve, of the surfels, of a diff or of anything else in the context is written.
#include <math.h>

#include "tl_ctx.hpp"
#include "tl_free_box.hpp"

using namespace tl;

namespace tlh {

// the context and the grid checked for a call that needs one
int free_ready(const tloam_ctx* c) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  if (!c->cmap.built || !c->cmap.free.have) return TLOAM_E_NOT_READY;
  return TLOAM_OK;
}

// ... and for a read, which resolves occupancy: the gate needs the carve's counts
int free_read_ready(const tloam_ctx* c) {
  const int rc = free_ready(c);
  if (rc != TLOAM_OK) return rc;
  return c->cmap.free.cfg.carve_gate && !c->cmap.carved ? TLOAM_E_NOT_READY : TLOAM_OK;
}

tl::FreeQuery free_query(const CmapState& M) {
  const CmapState::FreeState& F = M.free;
  FreeQuery q;
  memset(&q, 0, sizeof(q));
  q.grid = map_grid_of(M);
  q.gate = CarveGate{(const long long*)M.miss.p, F.cfg.min_count, F.cfg.min_miss, F.cfg.miss_ratio, F.cfg.carve_gate, 0};
  q.g = F.grid;
  return q;
}

}  // namespace tlh

namespace {

using FreeState = CmapState::FreeState;

bool free_config_ok(const tloam_closed_map_free_config& m) {
  return m.max_range > 0.0 && std::isfinite(m.max_range) && m.end_margin >= 0.0 && std::isfinite(m.end_margin) && m.max_bytes >= 8 &&
         m.min_count >= 1 && m.min_miss >= 0 && m.miss_ratio == m.miss_ratio && m.ray_mask >= 0 && m.ray_mask <= 0xFF &&
         (m.carve_gate == 0 || m.carve_gate == 1);
}

// what an add leaves in the info: the last add's counters, the grid's totals
void free_note_add(FreeState& F, long long rays, const unsigned long long ctl[kFreeCtl], int launches) {
  F.info.rays = (int64_t)rays;
  F.info.skipped_rays = (int64_t)ctl[0];
  F.info.cells_marked = (int64_t)ctl[1];
  F.info.cells_outside = (int64_t)ctl[2];
  F.info.free_cells = (int64_t)ctl[3];
  F.info.bricks_nonzero = (int64_t)ctl[4];
  F.info.launches = launches;
}

// an add failed with its launches possibly in flight: the stream drained (again, after cmap_scan_call), the grid (half written,
// perhaps) gone
int free_add_failed(tloam_ctx* c, int rc) {
  (void)hipStreamSynchronize(c->stream);
  c->cmap.free.drop();
  return rc;
}

}  // namespace

extern "C" {

void tloam_closed_map_free_default_config(tloam_closed_map_free_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_range = 60.0;
  cfg->end_margin = 1.0;
  cfg->max_bytes = (int64_t)1 << 30;
  cfg->min_count = 1;
  cfg->min_miss = 3;
  cfg->miss_ratio = 1.0;
  cfg->ray_mask = 0;
  cfg->carve_gate = 0;
}

int tloam_closed_map_free_configure(tloam_ctx* c, const tloam_closed_map_free_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_free_config want = cfg_or_default(cfg, tloam_closed_map_free_default_config);
  if (!free_config_ok(want)) return TLOAM_E_INVALID;
  c->cmap.free.drop();
  c->cmap.free.cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_free_info(tloam_ctx* c, tloam_closed_map_free_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.free.info;
  return TLOAM_OK;
}

int tloam_closed_map_free_reset(tloam_ctx* c, const int64_t* lo_cells, const int64_t* hi_cells) {
  if (!c || c->nranks > 1 || (lo_cells == nullptr) != (hi_cells == nullptr)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built) return TLOAM_E_NOT_READY;
  FreeState& F = M.free;
  int64_t lo[3], hi[3];
  if (lo_cells) {
    for (int a = 0; a < 3; ++a) { lo[a] = lo_cells[a]; hi[a] = hi_cells[a]; }
  } else {
    tlf::auto_box(M.poses.data(), M.poses.size() / 16, M.cfg.origin, M.cfg.voxel, F.cfg.max_range, lo, hi);
  }
  tlf::FreeBox B;
  if (!tlf::make_box(lo, hi, F.cfg.max_bytes, &B)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (F.words.cap < (size_t)B.words) HIPC(c, hipStreamSynchronize(c->stream));   // (the words replaced may still be read)
  HIPC(c, F.words.reserve((size_t)B.words));   // (a failure leaves the previous grid)
  HIPC(c, F.ctl.reserve(kFreeCtl));
  FreeGrid g;
  memset(&g, 0, sizeof(g));
  g.words = F.words.p;
  for (int a = 0; a < 3; ++a) { g.blo[a] = (int)B.blo[a]; g.nb[a] = (int)B.nb[a]; }
  g.nwords = (long long)B.words;
  // from here on the previous grid is gone, and what was built from it
  F.drop_fields();
  F.have = false;
  F.info = tloam_closed_map_free_info{};
  F.grid = g;
  const int launches = launch_free_clear(g, c->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    c->last_error = std::string("tloam_closed_map_free_reset: ") + hipGetErrorString(e);
    return free_add_failed(c, TLOAM_E_HIP);
  }
  for (int a = 0; a < 3; ++a) { F.info.lo_cells[a] = 4 * B.blo[a]; F.info.n_bricks[a] = B.nb[a]; }
  F.info.bytes = (int64_t)B.bytes;
  F.info.launches = launches;
  F.have = true;
  return TLOAM_OK;
}

int tloam_closed_map_free_add_keyframes(tloam_ctx* c, tloam_closed_map_free_info* info) {
  const int ready = free_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  if (M.detached) return TLOAM_E_NOT_READY;   // (loaded without its clouds: DESIGN.md 25)
  FreeState& F = M.free;
  const tloam_closed_map_free_config& g = F.cfg;
  F.drop_fields();   // (the clearance and the frontiers were built from the grid as it was)
  CmapPassOut R;
  const int rc = cmap_pass<FreeWork>(
      c, g.ray_mask ? g.ray_mask : M.cfg.cloud_mask, F.ctl,
      [&]() -> int {
        HIPC(c, F.ctl.reserve(kFreeCtl));
        HIPC(c, hipMemsetAsync(F.ctl.p, 0, sizeof(unsigned long long) * kFreeCtl, c->stream));
        return TLOAM_OK;
      },
      [&](FreeWork& W) {   // (W.scan stays zero: the keyframe form)
        W.max_range = g.max_range;
        W.end_margin = g.end_margin;
        W.g = F.grid;
        return launch_free_rays(W, true, c->stream);
      },
      &R, (size_t)F.info.keyframes);
  if (rc != TLOAM_OK) return free_add_failed(c, rc);
  free_note_add(F, R.n, R.ctl, R.launches);
  F.info.keyframes = (int64_t)R.K;
  if (info) *info = F.info;
  return TLOAM_OK;
}

int tloam_closed_map_free_add_scan(tloam_ctx* c, const double* points_aos, size_t n, const double* pose,
                                   tloam_closed_map_free_info* info) {
  if (!c || c->nranks > 1 || !points_aos || !pose || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const int ready = free_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (!pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  FreeState& F = M.free;
  F.drop_fields();   // (the clearance and the frontiers were built from the grid as it was)
  unsigned long long ctl[kFreeCtl];
  int launches = 0, prepared = 0;
  const int rc = cmap_scan_call(
      c, CmapScanCall{points_aos, n, pose, false, &F.ctl, kFreeCtl, ctl}, &prepared, [](auto) { return TLOAM_OK; },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        FreeWork W;
        memset(&W, 0, sizeof(W));
        W.scan = scan;
        W.grid = grid;
        W.max_range = F.cfg.max_range;
        W.end_margin = F.cfg.end_margin;
        W.g = F.grid;
        W.ctl = F.ctl.p;
        launches = launch_free_rays(W, false, c->stream);
        return TLOAM_OK;
      },
      [] { return TLOAM_OK; });
  if (rc != TLOAM_OK) return free_add_failed(c, rc);
  free_note_add(F, (long long)n, ctl, launches);
  F.info.scans += 1;
  if (info) *info = F.info;
  return TLOAM_OK;
}

int tloam_closed_map_read_free_words(tloam_ctx* c, size_t first, size_t count, uint64_t* words) {
  const int ready = free_ready(c);
  if (ready != TLOAM_OK) return ready;
  const FreeState& F = c->cmap.free;
  const size_t nw = (size_t)F.grid.nwords;
  if (first > nw || count > nw - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!words) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(words, F.grid.words + first, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_occupancy(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, uint8_t* state_out,
                               int32_t* ids_out, int64_t* counts_out) {
  if (!c || c->nranks > 1 || !points_aos || !state_out || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  unsigned long long w[4];
  int prepared = 0;
  const int rc = cmap_scan_call(
      c, CmapScanCall{points_aos, n, pose, false, &M.scan_ctl, 4, w}, &prepared,
      [&](auto room) -> int {
        HIPC(c, room(M.scan_u8, n));
        if (ids_out) HIPC(c, room(M.scan_ids, n));
        return TLOAM_OK;
      },
      [&](const MapGrid&, const ScanAt& scan) -> int {
        FreePointsArgs A;
        memset(&A, 0, sizeof(A));
        A.q = free_query(M);
        A.scan = scan;
        A.posed = pose ? 1 : 0;
        A.state = M.scan_u8.p;
        A.ids = ids_out ? M.scan_ids.p : nullptr;
        A.ctl = M.scan_ctl.p;
        launch_free_points(A, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(state_out, M.scan_u8.p, n, hipMemcpyDeviceToHost, c->stream));
        if (ids_out) HIPC(c, hipMemcpyAsync(ids_out, M.scan_ids.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
  if (rc != TLOAM_OK) return rc;
  if (counts_out)
    for (int k = 0; k < 4; ++k) counts_out[k] = (int64_t)w[k];
  return TLOAM_OK;
}

int tloam_closed_map_read_free(tloam_ctx* c, const double* lo, const double* hi, size_t capacity, size_t* n, double* centres_aos) {
  if (n) *n = 0;
  if (!c || !n || (lo == nullptr) != (hi == nullptr) || c->nranks > 1) return TLOAM_E_INVALID;
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  FreeState& F = M.free;
  const size_t most = (size_t)F.info.free_cells;   // the grid's popcount: no read gives more
  if (most == 0) return TLOAM_OK;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (the scratch may be replaced)
  const size_t blocks = ((size_t)F.grid.nwords + 255) / 256;
  HIPC(c, F.rd_c.reserve(3 * most)); HIPC(c, F.look.reserve(blocks + 1)); HIPC(c, M.scan_ctl.reserve(kDiffCtl));
  HIPC(c, hipMemsetAsync(F.look.p, 0, sizeof(unsigned long long) * (blocks + 1), c->stream));
  HIPC(c, hipMemsetAsync(M.scan_ctl.p, 0, sizeof(unsigned long long) * 8, c->stream));
  FreeCellsArgs A;
  memset(&A, 0, sizeof(A));
  A.q = free_query(M);
  A.boxed = lo ? 1 : 0;
  for (int a = 0; a < 3; ++a) { A.lo[a] = lo ? lo[a] : 0.0; A.hi[a] = hi ? hi[a] : 0.0; }
  A.out_c = F.rd_c.p;
  A.look = F.look.p;
  A.ctl = M.scan_ctl.p;
  launch_free_cells(A, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long w[3];
  HIPC(c, hipMemcpyAsync(w, M.scan_ctl.p, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (w[1]) {
    c->last_error = "closed map free space: a look-back of k_free_cells timed out";
    return TLOAM_E_HIP;
  }
  const size_t m = (size_t)w[2];
  *n = m;
  if (m == 0) return TLOAM_OK;
  if (capacity < m) return TLOAM_E_INVALID;
  if (centres_aos) {
    HIPC(c, hipMemcpyAsync(centres_aos, F.rd_c.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
  }
  return TLOAM_OK;
}

int tloam_closed_map_free_columns(tloam_ctx* c, double z_lo, double z_hi, int64_t min_free, uint8_t* state_out, size_t capacity,
                                  size_t* nx, size_t* ny) {
  if (nx) *nx = 0;
  if (ny) *ny = 0;
  if (!c || c->nranks > 1 || !nx || !ny || min_free < 1) return TLOAM_E_INVALID;
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  FreeState& F = M.free;
  int64_t z0, z1;
  if (!tlf::z_band(z_lo, z_hi, M.cfg.origin[2], M.cfg.voxel, F.grid.blo[2], F.grid.nb[2], &z0, &z1)) return TLOAM_E_INVALID;
  const size_t cx = 4 * (size_t)F.grid.nb[0], cy = 4 * (size_t)F.grid.nb[1], cols = cx * cy;   // (nb <= 2^19 each: no overflow)
  *nx = cx;
  *ny = cy;
  if (capacity < cols || !state_out) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (M.scan_u8.cap < cols) HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, M.scan_u8.reserve(cols));
  FreeColumnsArgs A;
  memset(&A, 0, sizeof(A));
  A.q = free_query(M);
  A.z0 = (int)z0;
  A.z1 = (int)z1;
  A.min_free = min_free;
  A.state = M.scan_u8.p;
  launch_free_columns(A, c->stream);
  HIPC(c, hipGetLastError());
  HIPC(c, hipMemcpyAsync(state_out, M.scan_u8.p, cols, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

}  // extern "C"
