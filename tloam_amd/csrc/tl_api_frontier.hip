// tl_api_frontier.hip -- C ABI of the closed map's frontiers (include/tloam_hip.h: tloam_closed_map_frontier_*, _get_frontier_info,
// _read_frontier, _read_frontier_cells; kernels in tl_frontier.hip; the tile, byte and table arithmetic in
// tl_tile_box.hpp).
//
// The field is a FrontierState inside the free space's FreeState, beside the clearance's: a build resolves the states of the
// grid's box as the occupancy query does (free_query: the one carve gate), marks the frontier cells, enqueues rounds_per_wait
// rounds of the tiled min-propagation between two waits and stops when a round marked no tile, counts, then gathers the clusters;
// the point query goes through the scan-form runner (cmap_scan_call); the cost join reads the route field; the column form runs
// the same launches over the layer the free space's column call computes.  Nothing of the closed map, of the free-space grid, of
// the clearance field, of the route field or of anything else in the context is written.
#include <math.h>

#include "tl_ctx.hpp"
#include "tl_free_box.hpp"

using namespace tl;

namespace {

using FreeState = CmapState::FreeState;
using FrontierState = FreeState::FrontierState;

bool frontier_config_ok(const tloam_closed_map_frontier_config& m) {
  return m.max_bytes >= 4 && m.min_cells >= 1 && m.reach >= 0 && m.reach <= 4 && m.max_rounds >= 1 && m.rounds_per_wait >= 1 &&
         m.rounds_per_wait <= kTileMaxBatch;
}

// the context, the grid and the field checked for a query of the field
int frontier_ready(const tloam_ctx* c) {
  const int rc = free_read_ready(c);
  if (rc != TLOAM_OK) return rc;
  return c->cmap.free.frontier.have ? TLOAM_OK : TLOAM_E_NOT_READY;
}

// blocks of 256 threads over n items, as the launches count them (tl_voxel.hpp's blocks_of)
size_t blocks256(size_t n) { return (n + 255) / 256; }

// What a build and a column call share, the field and the flags reserved and the seed's arguments filled but for its flags and
// control words: the states and the marks, the rounds in batches of rounds_per_wait with one wait each, the count, the cluster
// table sized from the count and gathered.  *info, *table and *kept filled on TLOAM_OK; on a failure launches may be in flight:
// the caller drains the stream.
int frontier_run(tloam_ctx* c, const char* who, FrontSeedArgs S, const tlt::TileBox& B, FrontierState::Bufs& U,
                 tloam_closed_map_frontier_info* info, FrontTable* table, std::vector<tloam_closed_map_frontier_cluster>* kept) {
  FrontierState& Fr = c->cmap.free.frontier;
  const TileField& f = S.f;
  unsigned long long* ctl = Fr.ctl.p;
  const size_t ntiles = (size_t)B.ntiles;
  HIPC(c, hipMemsetAsync(U.flags.p, 0, sizeof(unsigned) * 2 * ntiles, c->stream));
  HIPC(c, hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * kFrontCtl, c->stream));
  S.next = U.flags.p;
  S.ctl = ctl;
  int launches = launch_front_seed(S, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long head[2] = {0ull, 0ull};   // the frontier cells' marks are the first round's tiles
  TileRounds r;
  const int rc = tile_rounds(c, who, "labels", Fr.cfg.max_rounds, Fr.cfg.rounds_per_wait, f, U.flags.p, ntiles, ctl + kFrontRounds0,
                             launch_front_round, ctl, head, 2, &r);
  if (rc != TLOAM_OK) return rc;
  int waits = r.waits;
  launches += (int)r.enqueued;
  launch_front_count(f, ctl, c->stream);
  ++launches;
  HIPC(c, hipGetLastError());
  unsigned long long w[5];   // free, unknown, occupied, frontier cells, roots
  HIPC(c, hipMemcpyAsync(w, ctl + 2, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  ++waits;
  const size_t nroots = (size_t)w[4];
  uint64_t table_bytes = 0;
  if (!tlt::table_room(nroots, B.bytes, Fr.cfg.max_bytes, &table_bytes)) {
    c->last_error = std::string(who) + ": the table of " + std::to_string(nroots) + " clusters does not fit under max_bytes = " +
                    std::to_string(Fr.cfg.max_bytes) + " beside the field";
    return TLOAM_E_HIP;
  }
  unsigned long long g[9] = {0ull};   // [8 .. 16]: tickets, fault, written of the roots and of the kept list, cells kept, largest
  kept->clear();
  *table = FrontTable{};
  if (nroots) {
    const size_t nb = blocks256((size_t)(f.cells >> 2)), kb = blocks256(nroots);
    HIPC(c, U.roots.reserve(nroots));   // (the stream is idle: the wait above)
    HIPC(c, U.rec.reserve(nroots));
    HIPC(c, U.kept_rec.reserve(nroots));
    HIPC(c, U.kept_of.reserve(nroots));
    HIPC(c, U.look.reserve(nb + 1 + kb + 1));
    HIPC(c, hipMemsetAsync(U.look.p, 0, sizeof(unsigned long long) * (nb + 1 + kb + 1), c->stream));
    FrontGatherArgs G;
    memset(&G, 0, sizeof(G));
    G.f = f;
    G.roots = U.roots.p;
    G.rec = U.rec.p;
    G.kept_rec = U.kept_rec.p;
    G.kept_of = U.kept_of.p;
    G.nroots = (long long)nroots;
    G.min_cells = (unsigned)Fr.cfg.min_cells;
    G.look = U.look.p;
    G.ctl = ctl;
    launches += launch_front_gather(G, c->stream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(g, ctl + 8, sizeof(g), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    ++waits;
    if (g[1] || g[5]) {
      c->last_error = std::string(who) + ": a look-back of the cluster table timed out";
      return TLOAM_E_HIP;
    }
    if (g[2] != nroots || g[6] > nroots) {
      c->last_error = std::string(who) + ": the roots written do not match the roots counted";
      return TLOAM_E_HIP;
    }
    kept->resize((size_t)g[6]);
    if (g[6]) {
      HIPC(c, hipMemcpyAsync(kept->data(), U.kept_rec.p, sizeof(tloam_closed_map_frontier_cluster) * (size_t)g[6], hipMemcpyDeviceToHost,
                             c->stream));
      HIPC(c, hipStreamSynchronize(c->stream));
      ++waits;
    }
    table->roots = U.roots.p;
    table->kept_of = U.kept_of.p;
    table->nroots = (long long)nroots;
  }
  *info = tloam_closed_map_frontier_info{};
  for (int a = 0; a < 3; ++a) { info->lo_cells[a] = f.lo[a]; info->n_cells[a] = B.n[a]; }
  info->bytes = (int64_t)B.bytes;
  info->free_cells = (int64_t)w[0];
  info->unknown_cells = (int64_t)w[1];
  info->occupied_cells = (int64_t)w[2];
  info->frontier_cells = (int64_t)w[3];
  info->clusters = (int64_t)nroots;
  info->clusters_kept = (int64_t)g[6];
  info->cells_kept = (int64_t)g[7];
  info->largest = (int64_t)g[8];
  info->unknown_faces = (int64_t)head[1];
  info->tile_updates = (int64_t)head[0] + r.updates;
  info->rounds = (int32_t)r.rounds;
  info->launches = launches;
  info->waits = waits;
  return TLOAM_OK;
}

// the kept list by tloam_closed_map_read_box's capacity convention
int give_clusters(const std::vector<tloam_closed_map_frontier_cluster>& kept, size_t capacity, tloam_closed_map_frontier_cluster* out,
                  size_t* n_out) {
  *n_out = kept.size();
  if (kept.empty()) return TLOAM_OK;
  if (capacity < kept.size()) return TLOAM_E_INVALID;
  if (out) memcpy(out, kept.data(), sizeof(tloam_closed_map_frontier_cluster) * kept.size());
  return TLOAM_OK;
}

}  // namespace

extern "C" {

void tloam_closed_map_frontier_default_config(tloam_closed_map_frontier_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_bytes = (int64_t)1 << 30;
  cfg->min_cells = 8;
  cfg->reach = 2;
  cfg->max_rounds = 65536;
  cfg->rounds_per_wait = 16;
}

int tloam_closed_map_frontier_configure(tloam_ctx* c, const tloam_closed_map_frontier_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_frontier_config want = cfg_or_default(cfg, tloam_closed_map_frontier_default_config);
  if (!frontier_config_ok(want)) return TLOAM_E_INVALID;
  FrontierState& Fr = c->cmap.free.frontier;
  Fr.drop();
  Fr.cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_frontier_info(tloam_ctx* c, tloam_closed_map_frontier_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.free.frontier.info;
  return TLOAM_OK;
}

int tloam_closed_map_frontier_build(tloam_ctx* c, tloam_closed_map_frontier_info* info) {
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  FreeState& F = M.free;
  FrontierState& Fr = F.frontier;
  const int64_t cells[3] = {4 * (int64_t)F.grid.nb[0], 4 * (int64_t)F.grid.nb[1], 4 * (int64_t)F.grid.nb[2]};
  tlt::TileBox B;
  if (!tlt::make_box(cells, Fr.cfg.max_bytes, tlt::kFrontCellsBelow, &B)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (Fr.own.label.cap < (size_t)B.cells || Fr.own.flags.cap < 2 * (size_t)B.ntiles || Fr.ctl.cap < (size_t)kFrontCtl)
    HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, Fr.own.label.reserve((size_t)B.cells));   // (a failure leaves the previous field: the same box has the same size)
  HIPC(c, Fr.own.flags.reserve(2 * (size_t)B.ntiles));
  HIPC(c, Fr.ctl.reserve(kFrontCtl));
  const int lo[3] = {4 * F.grid.blo[0], 4 * F.grid.blo[1], 4 * F.grid.blo[2]};
  FrontSeedArgs S;
  memset(&S, 0, sizeof(S));
  S.q = free_query(M);
  S.f = field_of(B, lo, Fr.own.label.p);
  // from here on the previous field is gone
  Fr.have = false;
  Fr.info = tloam_closed_map_frontier_info{};
  Fr.view.info = tloam_closed_map_view_info{};   // (the last view call was of that field)
  Fr.field = TileField{};
  Fr.table = FrontTable{};
  Fr.kept.clear();
  tloam_closed_map_frontier_info got;
  FrontTable table;
  const int rc = frontier_run(c, "tloam_closed_map_frontier_build", S, B, Fr.own, &got, &table, &Fr.kept);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);   // the stream drained, the field (half labelled, perhaps) gone
    Fr.drop();
    return rc;
  }
  Fr.field = S.f;
  Fr.table = table;
  Fr.info = got;
  Fr.have = true;
  if (info) *info = got;
  return TLOAM_OK;
}

int tloam_closed_map_read_frontier(tloam_ctx* c, size_t first, size_t count, uint32_t* label) {
  const int ready = frontier_ready(c);
  if (ready != TLOAM_OK) return ready;
  const FrontierState& Fr = c->cmap.free.frontier;
  const size_t cells = (size_t)Fr.field.cells;
  if (first > cells || count > cells - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!label) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(label, Fr.field.v + first, sizeof(uint32_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_frontier_clusters(tloam_ctx* c, size_t capacity, tloam_closed_map_frontier_cluster* clusters_out, size_t* n_out) {
  if (n_out) *n_out = 0;
  if (!c || !n_out || c->nranks > 1) return TLOAM_E_INVALID;
  const int ready = frontier_ready(c);
  if (ready != TLOAM_OK) return ready;
  return give_clusters(c->cmap.free.frontier.kept, capacity, clusters_out, n_out);
}

int tloam_closed_map_read_frontier_cells(tloam_ctx* c, uint32_t root_or_all, size_t capacity, double* centres_aos_out,
                                         uint32_t* roots_out, size_t* n_out) {
  if (n_out) *n_out = 0;
  if (!c || !n_out || c->nranks > 1) return TLOAM_E_INVALID;
  const int ready = frontier_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  FrontierState& Fr = M.free.frontier;
  size_t m = (size_t)Fr.info.cells_kept;
  if (root_or_all != TLOAM_FRONTIER_ALL) {   // the kept list ascends in root
    const auto it = std::lower_bound(Fr.kept.begin(), Fr.kept.end(), root_or_all,
                                     [](const tloam_closed_map_frontier_cluster& r, uint32_t v) { return r.root < v; });
    m = it != Fr.kept.end() && it->root == root_or_all ? (size_t)it->cells : 0;
  }
  *n_out = m;
  if (m == 0) return TLOAM_OK;
  if (capacity < m) return TLOAM_E_INVALID;
  if (!centres_aos_out && !roots_out) return TLOAM_OK;
  HIPC(c, hipSetDevice(c->device));
  const size_t nb = blocks256((size_t)(Fr.field.cells >> 2));
  if (Fr.out_f64.cap < 3 * m || Fr.out_u32.cap < m || Fr.own.look.cap < nb + 1) HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, Fr.out_f64.reserve(3 * m));
  HIPC(c, Fr.out_u32.reserve(m));
  HIPC(c, Fr.own.look.reserve(nb + 1));
  HIPC(c, hipMemsetAsync(Fr.own.look.p, 0, sizeof(unsigned long long) * (nb + 1), c->stream));
  HIPC(c, hipMemsetAsync(Fr.ctl.p + 20, 0, sizeof(unsigned long long) * 4, c->stream));
  FrontCellsArgs A;
  memset(&A, 0, sizeof(A));
  A.f = Fr.field;
  A.t = Fr.table;
  A.root = root_or_all;
  A.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) A.origin[a] = M.cfg.origin[a];
  A.m = (long long)m;
  A.centres = Fr.out_f64.p;
  A.roots_out = Fr.out_u32.p;
  A.look = Fr.own.look.p;
  A.ctl = Fr.ctl.p;
  launch_front_cells(A, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long w[3];
  HIPC(c, hipMemcpyAsync(w, Fr.ctl.p + 20, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  if (centres_aos_out) HIPC(c, hipMemcpyAsync(centres_aos_out, Fr.out_f64.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, c->stream));
  if (roots_out) HIPC(c, hipMemcpyAsync(roots_out, Fr.out_u32.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (w[1] || w[2] != m) {
    c->last_error = "closed map frontiers: a look-back of k_front_cells timed out";
    return TLOAM_E_HIP;
  }
  return TLOAM_OK;
}

int tloam_closed_map_frontier_points(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, uint32_t* label_out,
                                     int32_t* cluster_out, int64_t* counts_out) {
  if (!c || c->nranks > 1 || !points_aos || !label_out || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const int ready = frontier_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (pose && !pose_finite_rigid(pose)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  FrontierState& Fr = M.free.frontier;
  unsigned long long w[5];
  int prepared = 0;
  const int rc = cmap_scan_call(
      c, CmapScanCall{points_aos, n, pose, false, &M.scan_ctl, 5, w}, &prepared,
      [&](auto room) -> int {
        HIPC(c, room(Fr.out_u32, n));
        if (cluster_out) HIPC(c, room(Fr.out_i32, n));
        return TLOAM_OK;
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        FrontPointsArgs A;
        memset(&A, 0, sizeof(A));
        A.f = Fr.field;
        A.t = Fr.table;
        A.voxel = grid.voxel;
        for (int a = 0; a < 3; ++a) A.origin[a] = grid.origin[a];
        A.scan = scan;
        A.posed = pose ? 1 : 0;
        A.label = Fr.out_u32.p;
        A.cluster = cluster_out ? Fr.out_i32.p : nullptr;
        A.ctl = M.scan_ctl.p;
        launch_front_points(A, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(label_out, Fr.out_u32.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (cluster_out) HIPC(c, hipMemcpyAsync(cluster_out, Fr.out_i32.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
  if (rc != TLOAM_OK) return rc;
  if (counts_out)
    for (int k = 0; k < 5; ++k) counts_out[k] = (int64_t)w[k];
  return TLOAM_OK;
}

int tloam_closed_map_frontier_costs(tloam_ctx* c, size_t capacity, uint32_t* cost_out, double* approach_aos_out, size_t* n_out) {
  if (n_out) *n_out = 0;
  if (!c || !n_out || c->nranks > 1) return TLOAM_E_INVALID;
  const int ready = frontier_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  FreeState& F = M.free;
  FrontierState& Fr = F.frontier;
  if (!F.clear.have || !F.clear.route.have) return TLOAM_E_NOT_READY;
  const TileField& R = F.clear.route.field;
  const TileField& f = Fr.field;
  // both fields lie over the grid's box as it is: whatever changes the grid drops both
  if (R.cells != f.cells || R.lo[0] != f.lo[0] || R.lo[1] != f.lo[1] || R.lo[2] != f.lo[2] || R.n[0] != f.n[0] || R.n[1] != f.n[1] ||
      R.n[2] != f.n[2]) {
    c->last_error = "tloam_closed_map_frontier_costs: the route field and the frontier field lie over different boxes";
    return TLOAM_E_INVALID;
  }
  const size_t m = Fr.kept.size();
  *n_out = m;
  if (m == 0) return TLOAM_OK;
  if (capacity < m) return TLOAM_E_INVALID;
  if (!cost_out && !approach_aos_out) return TLOAM_OK;
  HIPC(c, hipSetDevice(c->device));
  if (Fr.keys.cap < m) HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, Fr.keys.reserve(m));
  HIPC(c, hipMemsetAsync(Fr.keys.p, 0xFF, sizeof(unsigned long long) * m, c->stream));
  FrontCostsArgs A;
  memset(&A, 0, sizeof(A));
  A.f = f;
  A.t = Fr.table;
  A.cost = R.v;
  A.reach = Fr.cfg.reach;
  A.keys = Fr.keys.p;
  launch_front_costs(A, c->stream);
  HIPC(c, hipGetLastError());
  std::vector<unsigned long long> keys(m);
  HIPC(c, hipMemcpyAsync(keys.data(), Fr.keys.p, sizeof(unsigned long long) * m, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  const double v = M.cfg.voxel;
  for (size_t k = 0; k < m; ++k) {
    const bool none = keys[k] == ~0ull;
    if (cost_out) cost_out[k] = none ? TLOAM_ROUTE_UNREACHED : (uint32_t)(keys[k] >> 32);
    if (!approach_aos_out) continue;
    if (none) {
      for (int a = 0; a < 3; ++a) approach_aos_out[3 * k + a] = NAN;
      continue;
    }
    const long long idx = (long long)(keys[k] & 0xFFFFFFFFull), row = idx / f.n[0];
    const long long cell[3] = {idx - row * f.n[0], row % f.n[1], row / f.n[1]};
    for (int a = 0; a < 3; ++a) approach_aos_out[3 * k + a] = M.cfg.origin[a] + ((double)(f.lo[a] + cell[a]) + 0.5) * v;
  }
  return TLOAM_OK;
}

int tloam_closed_map_frontier_columns(tloam_ctx* c, double z_lo, double z_hi, int64_t min_free, uint32_t* label_out, size_t capacity,
                                      tloam_closed_map_frontier_cluster* clusters_out, size_t* n_out,
                                      tloam_closed_map_frontier_info* info) {
  if (n_out) *n_out = 0;
  if (!c || c->nranks > 1 || !n_out || min_free < 1) return TLOAM_E_INVALID;
  const int ready = free_read_ready(c);
  if (ready != TLOAM_OK) return ready;
  CmapState& M = c->cmap;
  FreeState& F = M.free;
  FrontierState& Fr = F.frontier;
  int64_t z0, z1;
  if (!tlf::z_band(z_lo, z_hi, M.cfg.origin[2], M.cfg.voxel, F.grid.blo[2], F.grid.nb[2], &z0, &z1)) return TLOAM_E_INVALID;
  const size_t cx = 4 * (size_t)F.grid.nb[0], cy = 4 * (size_t)F.grid.nb[1], cols = cx * cy;   // (nb <= 2^19 each: no overflow)
  const int64_t cells[3] = {(int64_t)cx, (int64_t)cy, 1};
  tlt::TileBox B;
  if (!tlt::make_box(cells, Fr.cfg.max_bytes, tlt::kFrontCellsBelow, &B)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (M.scan_u8.cap < cols || Fr.col.label.cap < cols || Fr.col.flags.cap < 2 * (size_t)B.ntiles || Fr.ctl.cap < (size_t)kFrontCtl)
    HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, M.scan_u8.reserve(cols));
  HIPC(c, Fr.col.label.reserve(cols));
  HIPC(c, Fr.col.flags.reserve(2 * (size_t)B.ntiles));
  HIPC(c, Fr.ctl.reserve(kFrontCtl));
  // the free space's column call, launch for launch: the states
  FreeColumnsArgs Q;
  memset(&Q, 0, sizeof(Q));
  Q.q = free_query(M);
  Q.z0 = (int)z0;
  Q.z1 = (int)z1;
  Q.min_free = min_free;
  Q.state = M.scan_u8.p;
  launch_free_columns(Q, c->stream);
  const int lo[3] = {4 * F.grid.blo[0], 4 * F.grid.blo[1], 4 * F.grid.blo[2]};
  FrontSeedArgs S;
  memset(&S, 0, sizeof(S));
  S.state = M.scan_u8.p;
  S.f = field_of(B, lo, Fr.col.label.p);
  tloam_closed_map_frontier_info got;
  FrontTable table;
  std::vector<tloam_closed_map_frontier_cluster> kept;
  int rc = TLOAM_OK;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    rc = frontier_run(c, "tloam_closed_map_frontier_columns", S, B, Fr.col, &got, &table, &kept);
    if (rc == TLOAM_OK && label_out) e = hipMemcpyAsync(label_out, Fr.col.label.p, sizeof(uint32_t) * cols, hipMemcpyDeviceToHost, c->stream);
  }
  const hipError_t waited = hipStreamSynchronize(c->stream);   // (nothing of the call stays in flight, whatever failed)
  if (rc != TLOAM_OK) return rc;
  if (e == hipSuccess) e = waited;
  if (e != hipSuccess) {
    c->last_error = std::string("tloam_closed_map_frontier_columns: ") + hipGetErrorString(e);
    return TLOAM_E_HIP;
  }
  got.launches += 1;   // the states
  got.waits += 1;
  if (info) *info = got;
  return give_clusters(kept, capacity, clusters_out, n_out);
}

}  // extern "C"
