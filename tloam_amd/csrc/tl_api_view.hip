// tl_api_view.hip -- C ABI of the closed map's view gain (include/tloam_hip.h: tloam_closed_map_view_*, _frontier_gains,
// _get_view_info; kernels in tl_view.hip; the window, form and chunk arithmetic in tl_view_box.hpp).
//
// The state is a ViewState inside the frontiers' FrontierState: the configuration, grow-only scratch and the last info.  A call
// reads the built frontier field as the dense state array of the box and goes through the scan-form runner (cmap_scan_call): the
// ends are the scan, the poses have a room of their own and are uploaded in fill_and_launch; the LDS form is one launch, the
// global form per chunk of views a memset of its windows and counters and two launches; the records and the views' beyond-window
// counts are read back with the one wait.  Nothing of the frontier field, of the closed map, of the free-space grid, of the
// clearance, of the route or of anything else in the context is written.
#include <math.h>
#include <stdlib.h>

#include "tl_ctx.hpp"
#include "tl_view_box.hpp"

using namespace tl;

namespace {

using FrontierState = CmapState::FreeState::FrontierState;
using ViewState = FrontierState::ViewState;

// the context, the grid and the field checked for a call that reads the field
int view_ready(const tloam_ctx* c) {
  const int rc = free_read_ready(c);
  if (rc != TLOAM_OK) return rc;
  return c->cmap.free.frontier.have ? TLOAM_OK : TLOAM_E_NOT_READY;
}

// the largest lds_bytes the device takes: what it reports as a block's most shared memory less the LDS form's static use
int view_lds_limit(tloam_ctx* c, int64_t* limit) {
  HIPC(c, hipSetDevice(c->device));
  int most = 0;
  HIPC(c, hipDeviceGetAttribute(&most, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
  *limit = std::max<int64_t>((int64_t)most - (int64_t)view_lds_static(), 0);
  return TLOAM_OK;
}

// the blocks a view's rays are split over in the global form: enough for every ray to have a thread, held to about 2048 blocks a
// launch (eight a CU); TLOAM_VIEW_BLOCKS (development aid: A/B, tests) overrides it
uint64_t view_blocks_wanted(uint64_t rays, uint64_t views_in_chunk) {
  if (const char* e = getenv("TLOAM_VIEW_BLOCKS")) {
    const long v = strtol(e, nullptr, 10);
    if (v >= 1) return (uint64_t)v;
  }
  const uint64_t fill = (rays + kViewThreads - 1) / kViewThreads, room = std::max<uint64_t>(2048u / views_in_chunk, 1u);
  return std::min(fill, room);
}

struct ViewCall {
  const double* poses;   // [16 views] host
  size_t views;
  const double* ends;    // [3 rays] host
  size_t rays;
  bool cells;            // the cells form (views == 1): the centres compacted into ViewState::out_f64 ...
  size_t capacity;       // ... at most this many
  int launches0, waits0; // what the caller has spent already
};

// One call: checked, planned (tl_view_box.hpp), run.  rec [views] and *info filled on TLOAM_OK, and the info kept as the last.
int view_run(tloam_ctx* c, const ViewCall& q, std::vector<tloam_closed_map_view_record>* rec, tloam_closed_map_view_info* info) {
  CmapState& M = c->cmap;
  FrontierState& Fr = M.free.frontier;
  ViewState& Vs = Fr.view;
  tlv::Window win;
  uint64_t total = 0;
  if (!tlv::make_window(Vs.cfg.max_range, M.cfg.voxel, &win)) return TLOAM_E_INVALID;
  if (!tlv::ray_count(q.views, q.rays, &total) || q.rays > kMaxPoints || q.views > tlv::kMostBlocks) return TLOAM_E_INVALID;
  int form = 0;
  if (!tlv::choose_form(Vs.cfg.form, win.bytes, Vs.cfg.lds_bytes, &form)) return TLOAM_E_INVALID;
  uint64_t per = q.views, chunks = 1, bpv = 1;
  if (form == tlv::kFormGlobal) {
    if (!tlv::make_chunks(q.views, win.bytes, Vs.cfg.max_bytes, &per, &chunks)) return TLOAM_E_INVALID;
    bpv = tlv::blocks_per_view(per, view_blocks_wanted(q.rays, per));
  }
  const size_t V = q.views, cap_dev = q.cells ? (size_t)std::min<uint64_t>(q.capacity, win.bits) : 0;
  rec->resize(V);
  std::vector<unsigned long long> beyond(V);
  int launches = q.launches0;
  int prepared = 0;
  const int rc = cmap_scan_call(
      c, CmapScanCall{q.ends, q.rays, nullptr, false, nullptr, 0, nullptr}, &prepared,
      [&](auto room) -> int {
        HIPC(c, room(Vs.poses, 16 * V));
        HIPC(c, room(Vs.rec, V));
        HIPC(c, room(Vs.beyond, V));
        if (form == tlv::kFormGlobal) {
          HIPC(c, room(Vs.win, (size_t)(per * win.words)));   // (per * bytes <= max_bytes: tlv::make_chunks)
          HIPC(c, room(Vs.cnt, (size_t)per * kViewCounters));
        }
        if (cap_dev) HIPC(c, room(Vs.out_f64, 3 * cap_dev));
        return TLOAM_OK;
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        HIPC(c, hipMemcpyAsync(Vs.poses.p, q.poses, sizeof(double) * 16 * V, hipMemcpyHostToDevice, c->stream));
        ViewArgs A;
        memset(&A, 0, sizeof(A));
        A.f = Fr.field;
        A.grid = grid;
        A.max_range = Vs.cfg.max_range;
        A.poses = Vs.poses.p;
        A.ends = scan.pts;
        A.rays = scan.n;
        A.words = (long long)win.words;
        A.W = (int)win.W;
        A.S = (int)win.S;
        A.bpv = (int)bpv;
        A.out = Vs.rec.p;
        A.beyond = Vs.beyond.p;
        A.centres = cap_dev ? Vs.out_f64.p : nullptr;
        A.capacity = (long long)cap_dev;
        if (form == tlv::kFormLds) {
          HIPC(c, launch_view_lds(A, (long long)V, q.cells, c->stream));
          ++launches;
          return TLOAM_OK;
        }
        A.win = Vs.win.p;
        A.cnt = Vs.cnt.p;
        for (uint64_t k = 0; k < chunks; ++k) {
          const uint64_t first = k * per, n = std::min<uint64_t>(per, V - first);
          HIPC(c, hipMemsetAsync(Vs.win.p, 0, sizeof(unsigned) * (size_t)(n * win.words), c->stream));
          HIPC(c, hipMemsetAsync(Vs.cnt.p, 0, sizeof(unsigned long long) * (size_t)n * kViewCounters, c->stream));
          A.view0 = (long long)first;
          launch_view_rays(A, (long long)n, c->stream);
          launch_view_count(A, (long long)n, q.cells, c->stream);
          launches += 2;
        }
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(rec->data(), Vs.rec.p, sizeof(tloam_closed_map_view_record) * V, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(beyond.data(), Vs.beyond.p, sizeof(unsigned long long) * V, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
  if (rc != TLOAM_OK) return rc;
  tloam_closed_map_view_info got{};
  got.views = (int64_t)V;
  got.rays = (int64_t)q.rays;
  got.window_side = win.S;
  got.window_bytes = (int64_t)win.bytes;
  got.chunks = (int64_t)chunks;
  for (size_t v = 0; v < V; ++v) {
    got.steps += (*rec)[v].steps;
    got.unknown_visits += (*rec)[v].unknown_visits;
    got.unknown_cells += (*rec)[v].unknown_cells;
    got.beyond_window += (int64_t)beyond[v];
  }
  got.form = form;
  got.blocks_per_view = (int32_t)bpv;
  got.launches = launches;
  got.waits = q.waits0 + 1;
  Vs.info = got;
  *info = got;
  return TLOAM_OK;
}

bool poses_rigid(const double* poses, size_t n) {
  for (size_t v = 0; v < n; ++v)
    if (!pose_finite_rigid(poses + 16 * v)) return false;
  return true;
}

}  // namespace

extern "C" {

void tloam_closed_map_view_default_config(tloam_closed_map_view_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_range = 20.0;
  cfg->max_bytes = (int64_t)256 << 20;
  cfg->lds_bytes = 131072;
  cfg->form = tlv::kFormAuto;
}

int tloam_closed_map_view_configure(tloam_ctx* c, const tloam_closed_map_view_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_closed_map_view_config want = cfg_or_default(cfg, tloam_closed_map_view_default_config);
  if (!(want.max_range > 0.0) || !isfinite(want.max_range) || want.max_bytes < 4 || want.lds_bytes < 0 || want.form < tlv::kFormAuto ||
      want.form > tlv::kFormGlobal)
    return TLOAM_E_INVALID;
  int64_t limit = 0;
  const int rc = view_lds_limit(c, &limit);
  if (rc != TLOAM_OK) return rc;
  if ((int64_t)want.lds_bytes > limit) return TLOAM_E_INVALID;
  ViewState& Vs = c->cmap.free.frontier.view;
  Vs.cfg = want;
  Vs.info = tloam_closed_map_view_info{};
  return TLOAM_OK;
}

int tloam_closed_map_get_view_info(tloam_ctx* c, tloam_closed_map_view_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.free.frontier.view.info;
  return TLOAM_OK;
}

int tloam_closed_map_view_gain(tloam_ctx* c, const double* poses_colmajor, size_t n_views, const double* ends_aos, size_t n_rays,
                               tloam_closed_map_view_record* gain_out, tloam_closed_map_view_info* info) {
  if (!c || c->nranks > 1 || !poses_colmajor || !ends_aos || !gain_out || n_views == 0 || n_rays == 0) return TLOAM_E_INVALID;
  uint64_t total = 0;
  if (!tlv::ray_count(n_views, n_rays, &total)) return TLOAM_E_INVALID;   // (before the poses are walked)
  const int ready = view_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (!poses_rigid(poses_colmajor, n_views)) return TLOAM_E_INVALID;
  std::vector<tloam_closed_map_view_record> rec;
  tloam_closed_map_view_info got;
  const int rc = view_run(c, ViewCall{poses_colmajor, n_views, ends_aos, n_rays, false, 0, 0, 0}, &rec, &got);
  if (rc != TLOAM_OK) return rc;
  memcpy(gain_out, rec.data(), sizeof(tloam_closed_map_view_record) * n_views);
  if (info) *info = got;
  return TLOAM_OK;
}

int tloam_closed_map_view_cells(tloam_ctx* c, const double* pose_colmajor, const double* ends_aos, size_t n_rays, size_t capacity,
                                double* centres_aos_out, size_t* n_out, tloam_closed_map_view_record* gain_out) {
  if (n_out) *n_out = 0;
  if (!c || c->nranks > 1 || !pose_colmajor || !ends_aos || !n_out || n_rays == 0) return TLOAM_E_INVALID;
  const int ready = view_ready(c);
  if (ready != TLOAM_OK) return ready;
  if (!pose_finite_rigid(pose_colmajor)) return TLOAM_E_INVALID;
  std::vector<tloam_closed_map_view_record> rec;
  tloam_closed_map_view_info got;
  const bool fetch = centres_aos_out != nullptr && capacity > 0;
  const int rc = view_run(c, ViewCall{pose_colmajor, 1, ends_aos, n_rays, fetch, capacity, 0, 0}, &rec, &got);
  if (rc != TLOAM_OK) return rc;
  const size_t m = (size_t)rec[0].unknown_cells;
  *n_out = m;
  if (m == 0) {
    if (gain_out) *gain_out = rec[0];
    return TLOAM_OK;
  }
  if (capacity < m) return TLOAM_E_INVALID;
  if (centres_aos_out) {
    ViewState& Vs = c->cmap.free.frontier.view;
    HIPC(c, hipMemcpyAsync(centres_aos_out, Vs.out_f64.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    Vs.info.waits += 1;
  }
  if (gain_out) *gain_out = rec[0];
  return TLOAM_OK;
}

int tloam_closed_map_frontier_gains(tloam_ctx* c, const double* ends_aos, size_t n_rays, size_t capacity,
                                    tloam_closed_map_view_record* gain_out, uint32_t* cost_out, double* approach_aos_out, size_t* n_out) {
  if (n_out) *n_out = 0;
  if (!c || c->nranks > 1 || !ends_aos || !n_out || n_rays == 0) return TLOAM_E_INVALID;
  size_t m = 0;
  int rc = tloam_closed_map_frontier_costs(c, 0, nullptr, nullptr, &m);   // readiness and the number, as the cost join has them
  if (rc != TLOAM_OK && m == 0) return rc;
  *n_out = m;
  if (m == 0) return TLOAM_OK;
  if (capacity < m) return TLOAM_E_INVALID;
  if (!gain_out && !cost_out && !approach_aos_out) return TLOAM_OK;
  std::vector<uint32_t> cost(m);
  std::vector<double> approach(3 * m), poses(16 * m, 0.0);
  rc = tloam_closed_map_frontier_costs(c, m, cost.data(), approach.data(), &m);   // one launch, one wait
  if (rc != TLOAM_OK) return rc;
  for (size_t k = 0; k < m; ++k) {   // the identity rotation at the approach point (three NaN: every ray skipped)
    double* P = poses.data() + 16 * k;
    P[0] = P[5] = P[10] = P[15] = 1.0;
    for (int a = 0; a < 3; ++a) P[12 + a] = approach[3 * k + a];
  }
  std::vector<tloam_closed_map_view_record> rec;
  tloam_closed_map_view_info got;
  rc = view_run(c, ViewCall{poses.data(), m, ends_aos, n_rays, false, 0, 1, 1}, &rec, &got);
  if (rc != TLOAM_OK) return rc;
  if (gain_out) memcpy(gain_out, rec.data(), sizeof(tloam_closed_map_view_record) * m);
  if (cost_out) memcpy(cost_out, cost.data(), sizeof(uint32_t) * m);
  if (approach_aos_out) memcpy(approach_aos_out, approach.data(), sizeof(double) * 3 * m);
  return TLOAM_OK;
}

}  // extern "C"
