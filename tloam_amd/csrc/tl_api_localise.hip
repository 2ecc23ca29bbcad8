// tl_api_localise.hip -- C ABI of the localisation of a scan in the closed map (include/tloam_hip.h: tloam_closed_map_localise*,
// _linearise; kernels in tl_localise.hip).
//
// A call takes the built closed map with its surfels (CmapState), uploads the scan and the stage's state words, enqueues the
// voxel records' rebuild when they are stale and max_iterations pairs of (sweep, step) on the context's stream, and waits once.
// A pair behind the last executed iteration returns on entry, so the launches are the same for every input.  Nothing of the
// closed map, of a carve's counts, of the surfels or of anything else in the context is written.
// Compiled with -ffp-contract=off: the prior's quaternion and its matrix are formed here as the restatement forms them.
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

bool config_ok(const tloam_closed_map_localise_config& w) {
  return w.max_residual0 > 0.0 && w.max_residual0 < HUGE_VAL && w.shrink > 0.0 && w.shrink <= 1.0 && w.min_residual >= 0.0 &&
         w.min_residual < HUGE_VAL && w.max_sigma >= 0.0 && w.min_planarity - w.min_planarity == 0.0 && w.step_tol_t >= 0.0 &&
         w.step_tol_t < HUGE_VAL && w.step_tol_r >= 0.0 && w.step_tol_r < HUGE_VAL && w.min_pivot_ratio >= 0.0 &&
         w.min_pivot_ratio < 1.0 && w.max_iterations >= 1 && w.max_iterations <= kLocMaxIterations && w.min_matches >= 1;
}

// what both calls check before anything is touched
int loc_check(const tloam_ctx* c, const double* points_aos, size_t n, const double* pose, Pose* T) {
  if (!c || c->nranks > 1 || !points_aos || !pose || n == 0 || n > kMaxPoints) return TLOAM_E_INVALID;
  const CmapState& M = c->cmap;
  if (!M.built || !M.surfeled) return TLOAM_E_NOT_READY;
  for (int i = 0; i < 16; ++i)
    if (!(pose[i] - pose[i] == 0.0)) return TLOAM_E_INVALID;
  if (!pose_from_matrix(pose, T)) return TLOAM_E_INVALID;
  return TLOAM_OK;
}

// the buffers sized, the scan uploaded and the records rebuilt when stale (*prepared); ids, res: a linearise's per-point outputs are asked for
int loc_begin(tloam_ctx* c, const double* points_aos, size_t n, bool ids, bool res, int* prepared) {
  CmapState& M = c->cmap;
  const size_t nv = (size_t)M.info.n_voxels, cap = std::max<size_t>(M.rows.cap, 1);
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, M.loc_rec.reserve(cap)); HIPC(c, M.loc_pts.reserve(3 * n));
  HIPC(c, M.loc_partial.reserve((size_t)loc_blocks((long long)n) * kLocRow));
  HIPC(c, M.loc_state.reserve(1)); HIPC(c, M.loc_log.reserve(kLocMaxIterations));
  if (ids) HIPC(c, M.loc_ids.reserve(n));
  if (res) HIPC(c, M.loc_res.reserve(n));
  HIPC(c, hipMemcpyAsync(M.loc_pts.p, points_aos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  *prepared = 0;
  if (!M.loc_ready) {
    LocPrepArgs A;
    memset(&A, 0, sizeof(A));
    A.pkey = M.rows.key.p; A.pn = M.rows.n.p; A.pqx = M.rows.qx.p; A.pqy = M.rows.qy.p; A.pqz = M.rows.qz.p;
    A.sums = M.surfel_sums.p; A.normal = M.surfel_nrm.p; A.eval = M.surfel_ev.p;
    A.nv = (long long)nv;
    A.voxel = M.cfg.voxel;
    for (int a = 0; a < 3; ++a) A.origin[a] = M.cfg.origin[a];
    A.min_points = M.surfel_cfg.min_points;
    A.max_sigma2 = M.loc_cfg.max_sigma * M.loc_cfg.max_sigma;
    A.min_planarity = M.loc_cfg.min_planarity;
    A.rec = M.loc_rec.p;
    launch_loc_prepare(A, c->stream);
    HIPC(c, hipGetLastError());
    *prepared = 1;
  }
  return TLOAM_OK;
}

LocSweepArgs sweep_args(const CmapState& M, size_t n, int* ids, double* res) {
  LocSweepArgs W;
  memset(&W, 0, sizeof(W));
  W.pts = M.loc_pts.p;
  W.n = (long long)n;
  W.st = M.loc_state.p;
  W.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) W.origin[a] = M.cfg.origin[a];
  const VmapTable T = M.rows.table();
  W.pmask = T.pmask; W.ptab = T.ptab; W.pkey = T.pkey;
  W.nv = (long long)M.info.n_voxels;
  W.rec = M.loc_rec.p;
  W.partial = M.loc_partial.p;
  W.ids = ids;
  W.res = res;
  return W;
}

LocStepArgs step_args(const CmapState& M, size_t n, int k) {
  const tloam_closed_map_localise_config& g = M.loc_cfg;
  LocStepArgs A;
  memset(&A, 0, sizeof(A));
  A.st = M.loc_state.p;
  A.partial = M.loc_partial.p;
  A.nblocks = loc_blocks((long long)n);
  A.k = k;
  A.max_iterations = g.max_iterations; A.min_matches = g.min_matches;
  A.shrink = g.shrink; A.min_residual = g.min_residual;
  A.step_tol_t = g.step_tol_t; A.step_tol_r = g.step_tol_r; A.min_pivot_ratio = g.min_pivot_ratio;
  A.log = M.loc_log.p;
  return A;
}

// a failed enqueue or wait: nothing of the call stays in flight, and the records are rebuilt by the next call
int loc_failed(tloam_ctx* c, int rc) {
  (void)hipStreamSynchronize(c->stream);
  c->cmap.loc_ready = false;
  return rc;
}

int localise_body(tloam_ctx* c, const double* points_aos, size_t n, const Pose& T0, LocState* st, tloam_closed_map_localise_info* I) {
  CmapState& M = c->cmap;
  const tloam_closed_map_localise_config& g = M.loc_cfg;
  int rc = loc_begin(c, points_aos, n, false, false, &I->prepared);
  if (rc != TLOAM_OK) return rc;
  memset(st, 0, sizeof(*st));
  st->T = T0;
  pose_to_matrix(T0, st->M);
  st->pw = g.max_residual0;
  st->tau = fmax(g.min_residual, st->pw);
  st->status = TLOAM_LOCALISE_MAX_ITERATIONS;
  HIPC(c, hipMemcpyAsync(M.loc_state.p, st, sizeof(*st), hipMemcpyHostToDevice, c->stream));
  const LocSweepArgs W = sweep_args(M, n, nullptr, nullptr);
  for (int k = 0; k < g.max_iterations; ++k) {
    launch_loc_sweep(W, c->stream);
    launch_loc_step(step_args(M, n, k), c->stream);
    I->launches += 2;
  }
  HIPC(c, hipGetLastError());
  HIPC(c, hipMemcpyAsync(st, M.loc_state.p, sizeof(*st), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

}  // namespace

extern "C" {

void tloam_closed_map_localise_default_config(tloam_closed_map_localise_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_residual0 = 1.0; cfg->shrink = 0.7; cfg->min_residual = 0.1;
  cfg->max_sigma = HUGE_VAL; cfg->min_planarity = 0.05;
  cfg->step_tol_t = 1e-6; cfg->step_tol_r = 1e-7; cfg->min_pivot_ratio = 1e-9;
  cfg->max_iterations = 20; cfg->min_matches = 50;
}

int tloam_closed_map_localise_configure(tloam_ctx* c, const tloam_closed_map_localise_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  tloam_closed_map_localise_config want;
  if (cfg) want = *cfg;
  else tloam_closed_map_localise_default_config(&want);
  if (!config_ok(want)) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (want.max_sigma != M.loc_cfg.max_sigma || want.min_planarity != M.loc_cfg.min_planarity) M.loc_ready = false;   // the gate
  M.loc_cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_localise(tloam_ctx* c, const double* points_aos, size_t n, const double* prior, double* pose_out,
                              tloam_closed_map_localise_info* info) {
  Pose T0;
  const int rc0 = pose_out ? loc_check(c, points_aos, n, prior, &T0) : TLOAM_E_INVALID;
  if (rc0 != TLOAM_OK) return rc0;
  CmapState& M = c->cmap;
  tloam_closed_map_localise_info I;
  memset(&I, 0, sizeof(I));
  LocState st;
  const int rc = localise_body(c, points_aos, n, T0, &st, &I);
  if (rc != TLOAM_OK) return loc_failed(c, rc);
  M.loc_ready = true;
  const int it = std::min(std::max(st.iterations, 0), M.loc_cfg.max_iterations);
  std::vector<LocLog> log((size_t)it);
  auto read_log = [&]() -> int {
    HIPC(c, hipMemcpyAsync(log.data(), M.loc_log.p, sizeof(LocLog) * (size_t)it, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return TLOAM_OK;
  };
  if (it && read_log() != TLOAM_OK) return loc_failed(c, TLOAM_E_HIP);
  M.loc_records.assign((size_t)it, tloam_closed_map_localise_record{});
  static_assert(sizeof(LocLog) == sizeof(tloam_closed_map_localise_record), "the log is read back as it is");
  if (it) memcpy(M.loc_records.data(), log.data(), sizeof(LocLog) * (size_t)it);
  I.status = st.status;
  I.iterations = it;
  I.matched = (int64_t)st.sums[kLocTerms];
  I.used = (int64_t)st.sums[kLocTerms + 1];
  I.rms = I.used > 0 ? sqrt(2.0 * st.sums[27] / (double)I.used) : 0.0;
  if (st.status == TLOAM_LOCALISE_DEGENERATE) memcpy(pose_out, prior, sizeof(double) * 16);
  else pose_to_matrix(st.T, pose_out);
  if (info) *info = I;
  return TLOAM_OK;
}

int tloam_closed_map_localise_log(tloam_ctx* c, size_t capacity, size_t* n, tloam_closed_map_localise_record* records) {
  if (n) *n = 0;
  if (!c || !n || c->nranks > 1) return TLOAM_E_INVALID;
  const std::vector<tloam_closed_map_localise_record>& R = c->cmap.loc_records;
  *n = R.size();
  if (!records || R.empty()) return TLOAM_OK;
  if (capacity < R.size()) return TLOAM_E_INVALID;
  memcpy(records, R.data(), sizeof(R[0]) * R.size());
  return TLOAM_OK;
}

int tloam_closed_map_linearise(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, double tau, int32_t* ids,
                               double* residuals, double* out28, int64_t* counts2) {
  Pose rigid;   // (only the check that `pose` is a rigid transform: the sweep runs at the matrix as it stands)
  const int rc0 = (out28 && counts2 && tau >= 0.0) ? loc_check(c, points_aos, n, pose, &rigid) : TLOAM_E_INVALID;
  if (rc0 != TLOAM_OK) return rc0;
  CmapState& M = c->cmap;
  int prepared = 0;
  int rc = loc_begin(c, points_aos, n, ids != nullptr, residuals != nullptr, &prepared);
  if (rc != TLOAM_OK) return loc_failed(c, rc);
  LocState st;
  memset(&st, 0, sizeof(st));
  memcpy(st.M, pose, sizeof(double) * 16);   // the matrix as it stands
  st.tau = tau;
  auto body = [&]() -> int {
    HIPC(c, hipMemcpyAsync(M.loc_state.p, &st, sizeof(st), hipMemcpyHostToDevice, c->stream));
    launch_loc_sweep(sweep_args(M, n, ids ? M.loc_ids.p : nullptr, residuals ? M.loc_res.p : nullptr), c->stream);
    launch_loc_step(step_args(M, n, -1), c->stream);
    HIPC(c, hipGetLastError());
    HIPC(c, hipMemcpyAsync(&st, M.loc_state.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    if (ids) HIPC(c, hipMemcpyAsync(ids, M.loc_ids.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (residuals) HIPC(c, hipMemcpyAsync(residuals, M.loc_res.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    return TLOAM_OK;
  };
  rc = body();
  if (rc != TLOAM_OK) return loc_failed(c, rc);
  M.loc_ready = true;
  memcpy(out28, st.sums, sizeof(double) * kLocTerms);
  counts2[0] = (int64_t)st.sums[kLocTerms];
  counts2[1] = (int64_t)st.sums[kLocTerms + 1];
  return TLOAM_OK;
}

}  // extern "C"
