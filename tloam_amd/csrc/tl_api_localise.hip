// tl_api_localise.hip -- C ABI of the localisation of a scan in the closed map (include/tloam_hip.h: tloam_closed_map_localise*,
// _linearise; kernels in tl_localise.hip).
//
// A call takes the built closed map with its surfels (CmapState) and goes through loc_run, a caller of the scan-form runner
// (tl_ctx.hpp: cmap_scan_call, as the linearise is): the scan uploaded, the voxel records' rebuild enqueued when they are stale,
// the B states seeded (uploaded as the host forms them from the priors, or formed on the
// device by the relocalisation's launches), max_iterations pairs of (sweep, step) over the B hypotheses on the context's stream,
// the states and the logs read back, one wait.  The single call is B = 1.
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
  return pose_finite_rigid(pose, T) ? TLOAM_OK : TLOAM_E_INVALID;
}

// the runner's call of a localiser: no pose (the states carry it), the records, no control words
CmapScanCall loc_call(const double* points_aos, size_t n) { return CmapScanCall{points_aos, n, nullptr, true, nullptr, 0, nullptr}; }

// the localiser's own buffers sized for B hypotheses of n points, through the runner's room(buffer, elements)
template <class Room>
int loc_rooms(tloam_ctx* c, Room room, size_t n, size_t B) {
  CmapState& M = c->cmap;
  HIPC(c, room(M.loc_partial, B * (size_t)loc_blocks((long long)n) * kLocRow));
  HIPC(c, room(M.loc_state, B)); HIPC(c, room(M.loc_log, B * kLocMaxIterations));
  return TLOAM_OK;
}

LocSweepArgs sweep_args(const CmapState& M, const MapGrid& grid, const ScanAt& scan, int* ids, double* res) {
  LocSweepArgs W;
  memset(&W, 0, sizeof(W));
  W.pts = scan.pts;
  W.n = scan.n;
  W.st = M.loc_state.p;
  W.grid = grid;
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

// the state words a localisation starts from
void loc_state0(const tloam_closed_map_localise_config& g, const Pose& T0, LocState* st) {
  memset(st, 0, sizeof(*st));
  st->T = T0;
  pose_to_matrix(T0, st->M);
  st->pw = g.max_residual0;
  st->tau = fmax(g.min_residual, st->pw);
  st->status = TLOAM_LOCALISE_MAX_ITERATIONS;
}

// One run of the localiser over B hypotheses of one scan.  seed() leaves the B states on the device -- upload_states, or the
// launches that form them there, counted into `launches`; more_reads() enqueues what else the caller reads back with the wait
struct LocRun {
  std::vector<LocState> st;    // [B] as seeded by the host (upload_states), then as the run left them
  std::vector<LocLog> log;     // [B][kLocMaxIterations]
  int prepared = 0, launches = 0;
  explicit LocRun(size_t B) : st(B), log(B * kLocMaxIterations) {}
};
int upload_states(tloam_ctx* c, const LocRun& R) {
  HIPC(c, hipMemcpyAsync(c->cmap.loc_state.p, R.st.data(), sizeof(LocState) * R.st.size(), hipMemcpyHostToDevice, c->stream));
  return TLOAM_OK;
}
int no_reads() { return TLOAM_OK; }
template <class Seed, class Reads>
int loc_run(tloam_ctx* c, const double* points_aos, size_t n, LocRun& R, Seed seed, Reads more_reads) {
  CmapState& M = c->cmap;
  const int B = (int)R.st.size();
  return cmap_scan_call(
      c, loc_call(points_aos, n), &R.prepared, [&](auto room) { return loc_rooms(c, room, n, (size_t)B); },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        const int rc = seed();
        if (rc != TLOAM_OK) return rc;
        const LocSweepArgs W = sweep_args(M, grid, scan, nullptr, nullptr);
        for (int k = 0; k < M.loc_cfg.max_iterations; ++k) {
          launch_loc_sweep(W, B, c->stream);
          launch_loc_step(step_args(M, n, k), B, c->stream);
          R.launches += 2;
        }
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(R.st.data(), M.loc_state.p, sizeof(LocState) * R.st.size(), hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipMemcpyAsync(R.log.data(), M.loc_log.p, sizeof(LocLog) * R.log.size(), hipMemcpyDeviceToHost, c->stream));
        return more_reads();
      });
}

// what a hypothesis's state words and log say, as the single call reports them (info.launches and .prepared are the caller's)
void loc_report(const CmapState& M, const LocState& st, const LocLog* log, const double* prior, double* pose_out,
                tloam_closed_map_localise_info* I, std::vector<tloam_closed_map_localise_record>* records) {
  static_assert(sizeof(LocLog) == sizeof(tloam_closed_map_localise_record), "the log is read back as it is");
  const int it = std::min(std::max(st.iterations, 0), M.loc_cfg.max_iterations);
  records->assign((size_t)it, tloam_closed_map_localise_record{});
  if (it) memcpy(records->data(), log, sizeof(LocLog) * (size_t)it);
  I->status = st.status;
  I->iterations = it;
  I->matched = (int64_t)st.sums[kLocTerms];
  I->used = (int64_t)st.sums[kLocTerms + 1];
  I->rms = I->used > 0 ? sqrt(2.0 * st.sums[27] / (double)I->used) : 0.0;
  if (st.status == TLOAM_LOCALISE_DEGENERATE) memcpy(pose_out, prior, sizeof(double) * 16);
  else pose_to_matrix(st.T, pose_out);
}

// the pick among hypotheses (skip[h] set: left out): not DEGENERATE, the largest used, then the smaller cost of the last executed
// sweep, then the lower index; -1: none
int loc_pick(const LocState* st, const int* skip, int B) {
  int best = -1;
  for (int h = 0; h < B; ++h) {
    if ((skip && skip[h]) || st[h].status == TLOAM_LOCALISE_DEGENERATE) continue;
    if (best < 0) { best = h; continue; }
    const long long u = (long long)st[h].sums[kLocTerms + 1], ub = (long long)st[best].sums[kLocTerms + 1];
    if (u > ub || (u == ub && st[h].sums[27] < st[best].sums[27])) best = h;
  }
  return best;
}

bool reloc_config_ok(const tloam_closed_map_relocalise_config& w) {
  return w.num_candidates >= 1 && w.num_candidates <= kLocMaxBatch && w.max_dist > 0.0 && w.min_used_ratio >= 0.0 &&
         w.min_used_ratio <= 1.0 && w.max_rms > 0.0;
}

}  // namespace

namespace tlh {
int loc_records_prepare(tloam_ctx* c, int* prepared) {
  CmapState& M = c->cmap;
  HIPC(c, M.loc_rec.reserve(std::max<size_t>(M.rows.cap, 1)));
  *prepared = 0;
  if (M.loc_ready) return TLOAM_OK;
  LocPrepArgs A;
  memset(&A, 0, sizeof(A));
  A.grid = map_grid_of(M);
  A.sums = M.surfel_sums.p; A.normal = M.surfel_nrm.p; A.eval = M.surfel_ev.p;
  A.min_points = M.surfel_cfg.min_points;
  A.max_sigma2 = M.loc_cfg.max_sigma * M.loc_cfg.max_sigma;
  A.min_planarity = M.loc_cfg.min_planarity;
  A.rec = M.loc_rec.p;
  launch_loc_prepare(A, c->stream);
  HIPC(c, hipGetLastError());
  *prepared = 1;
  return TLOAM_OK;
}
}  // namespace tlh

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
  const tloam_closed_map_localise_config want = cfg_or_default(cfg, tloam_closed_map_localise_default_config);
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
  LocRun R(1);
  loc_state0(M.loc_cfg, T0, &R.st[0]);
  const int rc = loc_run(c, points_aos, n, R, [&] { return upload_states(c, R); }, no_reads);
  if (rc != TLOAM_OK) return rc;
  tloam_closed_map_localise_info I;
  memset(&I, 0, sizeof(I));
  loc_report(M, R.st[0], R.log.data(), prior, pose_out, &I, &M.loc_records);
  I.launches = R.launches;
  I.prepared = R.prepared;
  if (info) *info = I;
  return TLOAM_OK;
}

int tloam_closed_map_localise_log(tloam_ctx* c, size_t capacity, size_t* n, tloam_closed_map_localise_record* records) {
  if (n) *n = 0;
  if (!c || !n || c->nranks > 1) return TLOAM_E_INVALID;
  return copy_list(c->cmap.loc_records, capacity, n, records);
}

int tloam_closed_map_linearise(tloam_ctx* c, const double* points_aos, size_t n, const double* pose, double tau, int32_t* ids,
                               double* residuals, double* out28, int64_t* counts2) {
  Pose rigid;   // (only the check that `pose` is a rigid transform: the sweep runs at the matrix as it stands)
  const int rc0 = (out28 && counts2 && tau >= 0.0) ? loc_check(c, points_aos, n, pose, &rigid) : TLOAM_E_INVALID;
  if (rc0 != TLOAM_OK) return rc0;
  CmapState& M = c->cmap;
  int prepared = 0;
  LocState st;
  memset(&st, 0, sizeof(st));
  memcpy(st.M, pose, sizeof(double) * 16);   // the matrix as it stands
  st.tau = tau;
  const int rc = cmap_scan_call(
      c, loc_call(points_aos, n), &prepared,
      [&](auto room) -> int {
        if (ids) HIPC(c, room(M.scan_ids, n));
        if (residuals) HIPC(c, room(M.loc_res, n));
        return loc_rooms(c, room, n, 1);
      },
      [&](const MapGrid& grid, const ScanAt& scan) -> int {
        HIPC(c, hipMemcpyAsync(M.loc_state.p, &st, sizeof(st), hipMemcpyHostToDevice, c->stream));
        launch_loc_sweep(sweep_args(M, grid, scan, ids ? M.scan_ids.p : nullptr, residuals ? M.loc_res.p : nullptr), 1, c->stream);
        launch_loc_step(step_args(M, n, -1), 1, c->stream);
        return TLOAM_OK;
      },
      [&]() -> int {
        HIPC(c, hipMemcpyAsync(&st, M.loc_state.p, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        if (ids) HIPC(c, hipMemcpyAsync(ids, M.scan_ids.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (residuals) HIPC(c, hipMemcpyAsync(residuals, M.loc_res.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        return TLOAM_OK;
      });
  if (rc != TLOAM_OK) return rc;
  memcpy(out28, st.sums, sizeof(double) * kLocTerms);
  counts2[0] = (int64_t)st.sums[kLocTerms];
  counts2[1] = (int64_t)st.sums[kLocTerms + 1];
  return TLOAM_OK;
}

int tloam_closed_map_localise_batch(tloam_ctx* c, const double* points_aos, size_t n, const double* priors, size_t B,
                                    double* poses_out, tloam_closed_map_localise_info* infos, int32_t* best_out) {
  if (!priors || !poses_out || !infos || !best_out || B == 0 || B > (size_t)kLocMaxBatch) return TLOAM_E_INVALID;
  LocRun R(B);
  Pose T0;
  for (size_t h = 0; h < B; ++h) {   // every prior before anything is touched
    const int rc0 = loc_check(c, points_aos, n, priors + 16 * h, &T0);
    if (rc0 != TLOAM_OK) return rc0;
    loc_state0(c->cmap.loc_cfg, T0, &R.st[h]);
  }
  CmapState& M = c->cmap;
  const int rc = loc_run(c, points_aos, n, R, [&] { return upload_states(c, R); }, no_reads);
  if (rc != TLOAM_OK) return rc;
  M.loc_batch_records.resize(B);
  for (size_t h = 0; h < B; ++h) {
    memset(&infos[h], 0, sizeof(infos[h]));
    loc_report(M, R.st[h], R.log.data() + h * kLocMaxIterations, priors + 16 * h, poses_out + 16 * h, &infos[h],
               &M.loc_batch_records[h]);
    infos[h].launches = R.launches;
    infos[h].prepared = R.prepared;
  }
  *best_out = loc_pick(R.st.data(), nullptr, (int)B);
  return TLOAM_OK;
}

int tloam_closed_map_localise_batch_log(tloam_ctx* c, size_t hypothesis, size_t capacity, size_t* n,
                                        tloam_closed_map_localise_record* records) {
  if (n) *n = 0;
  if (!c || !n || c->nranks > 1 || hypothesis >= c->cmap.loc_batch_records.size()) return TLOAM_E_INVALID;
  return copy_list(c->cmap.loc_batch_records[hypothesis], capacity, n, records);
}

void tloam_closed_map_relocalise_default_config(tloam_closed_map_relocalise_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->num_candidates = 8;
  cfg->max_dist = HUGE_VAL; cfg->min_used_ratio = 0.5; cfg->max_rms = HUGE_VAL;
}

int tloam_closed_map_relocalise_configure(tloam_ctx* c, const tloam_closed_map_relocalise_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  tloam_closed_map_relocalise_config want = cfg_or_default(cfg, tloam_closed_map_relocalise_default_config);
  if (!reloc_config_ok(want)) return TLOAM_E_INVALID;
  want.reserved0 = 0;
  c->cmap.reloc_cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_relocalise(tloam_ctx* c, const double* points_aos, size_t n, double* pose_out,
                                tloam_closed_map_relocalise_info* info) {
  if (!c || c->nranks > 1 || !points_aos || !pose_out || n == 0 || n > kMaxPoints || n > (size_t)INT32_MAX / 3)
    return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  PlaceState& P = c->place;
  const int64_t K = M.info.n_keyframes;
  if (!P.cfg.enabled || !M.built || !M.surfeled || K < 1 || K > P.n_kf || M.poses.size() != 16 * (size_t)K)
    return TLOAM_E_NOT_READY;
  const tloam_closed_map_relocalise_config& r = M.reloc_cfg;
  const tloam_place_config& g = P.cfg;
  const int B = (int)std::min<int64_t>(r.num_candidates, K);
  const size_t R = (size_t)g.n_rings, S = (size_t)g.n_sectors;
  LocRun run((size_t)B);
  std::vector<RelocHyp> hyp((size_t)B);
  auto seed = [&]() -> int {   // the place search's candidates made the B states, on the device
    HIPC(c, P.s_desc.reserve(R * S)); HIPC(c, P.s_rkey.reserve(R)); HIPC(c, P.s_skey.reserve(S));
    HIPC(c, M.reloc_cand.reserve(kLocMaxBatch)); HIPC(c, M.reloc_hyp.reserve(kLocMaxBatch));
    HIPC(c, M.reloc_poses.reserve(16 * (size_t)K));
    HIPC(c, hipMemcpyAsync(M.reloc_poses.p, M.poses.data(), sizeof(double) * 16 * (size_t)K, hipMemcpyHostToDevice, c->stream));
    PlaceDescArgs D;   // the scan's descriptor and ring key, as tloam_place_describe forms them, from the uploaded scan
    memset(&D, 0, sizeof(D));
    D.aos = M.loc_pts.p; D.n = (long long)n;
    D.bins = P.bins.p; D.desc = P.s_desc.p; D.ring_key = P.s_rkey.p; D.sector_key = P.s_skey.p;
    D.R = g.n_rings; D.S = g.n_sectors;
    D.max_radius = g.max_radius; D.height_offset = g.height_offset;
    launch_place_describe(D, c->stream);
    PlaceSearchArgs A;   // keyframes 0 .. K-1 ranked by ring key, each candidate's best shift; no loop record
    memset(&A, 0, sizeof(A));
    A.desc = P.desc.p; A.ring_key = P.rkey.p;
    A.q_desc = P.s_desc.p; A.q_ring_key = P.s_rkey.p;
    A.kdist = P.kdist.p; A.taken = P.taken.p; A.cand = M.reloc_cand.p;
    A.m = (int)K; A.ncand = B;
    A.R = g.n_rings; A.S = g.n_sectors;
    launch_place_candidates(A, c->stream);
    RelocPriorArgs Q;
    memset(&Q, 0, sizeof(Q));
    Q.cand = M.reloc_cand.p; Q.poses = M.reloc_poses.p;
    Q.B = B; Q.S = g.n_sectors;
    Q.max_dist = r.max_dist;
    Q.max_residual0 = M.loc_cfg.max_residual0; Q.min_residual = M.loc_cfg.min_residual;
    Q.hyp = M.reloc_hyp.p; Q.st = M.loc_state.p;
    launch_reloc_priors(Q, c->stream);
    run.launches += 5;
    return TLOAM_OK;
  };
  const int rc = loc_run(c, points_aos, n, run, seed, [&]() -> int {
    HIPC(c, hipMemcpyAsync(hyp.data(), M.reloc_hyp.p, sizeof(RelocHyp) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    return TLOAM_OK;
  });
  if (rc != TLOAM_OK) return rc;
  M.reloc_hyps.assign((size_t)B, tloam_closed_map_relocalise_hypothesis{});
  M.loc_batch_records.resize((size_t)B);
  std::vector<int> skip((size_t)B);
  double finite = 0.0;
  bool have_finite = false;
  for (int h = 0; h < B; ++h) {
    tloam_closed_map_relocalise_hypothesis& H = M.reloc_hyps[(size_t)h];
    const RelocHyp& d = hyp[(size_t)h];
    H.keyframe = d.keyframe; H.shift = d.shift; H.skipped = d.skipped;
    H.dist = d.d; H.yaw = d.yaw;
    memcpy(H.prior_colmajor, d.prior, sizeof(d.prior));
    skip[(size_t)h] = d.skipped;
    if (d.skipped) {   // never swept: the pose is the prior
      memcpy(H.pose_colmajor, d.prior, sizeof(d.prior));
      H.localise.status = TLOAM_LOCALISE_DEGENERATE;
      M.loc_batch_records[(size_t)h].clear();
    } else {
      loc_report(M, run.st[(size_t)h], run.log.data() + (size_t)h * kLocMaxIterations, d.prior, H.pose_colmajor, &H.localise,
                 &M.loc_batch_records[(size_t)h]);
      if (!have_finite) { finite = run.st[(size_t)h].sums[kLocFinite]; have_finite = true; }
    }
    H.localise.launches = 2 * M.loc_cfg.max_iterations;
    H.localise.prepared = run.prepared;
  }
  int best = loc_pick(run.st.data(), skip.data(), B);
  if (best >= 0) {
    const tloam_closed_map_localise_info& L = M.reloc_hyps[(size_t)best].localise;
    if (!((double)L.used >= r.min_used_ratio * finite && L.rms <= r.max_rms)) best = -1;
  }
  tloam_closed_map_relocalise_info I;
  memset(&I, 0, sizeof(I));
  I.status = best >= 0 ? TLOAM_RELOCALISE_FOUND : TLOAM_RELOCALISE_NOT_FOUND;
  I.n_hypotheses = B;
  I.best = best;
  I.launches = run.launches;
  I.keyframe = -1;
  if (best >= 0) {
    const tloam_closed_map_relocalise_hypothesis& H = M.reloc_hyps[(size_t)best];
    I.keyframe = H.keyframe; I.shift = H.shift; I.dist = H.dist; I.yaw = H.yaw;
    I.localise = H.localise;
    memcpy(pose_out, H.pose_colmajor, sizeof(H.pose_colmajor));
  }
  if (info) *info = I;
  return TLOAM_OK;
}

int tloam_closed_map_relocalise_hypotheses(tloam_ctx* c, size_t capacity, size_t* n,
                                           tloam_closed_map_relocalise_hypothesis* hypotheses) {
  if (n) *n = 0;
  if (!c || !n || c->nranks > 1) return TLOAM_E_INVALID;
  return copy_list(c->cmap.reloc_hyps, capacity, n, hypotheses);
}

}  // extern "C"
