// tl_api_graph.hip -- C ABI of the keyframe pose-graph optimisation (include/tloam_hip.h: tloam_graph_*; DESIGN.md section 18;
// the kernel in tl_graph.hip).
//
// A solve checks the caller's graph, turns poses and measurements into (unit quaternion, translation) on the host -- the form the
// device's exp / log / compose of tl_se3.hpp work on --, builds the table of every node's edge ends in edge order, uploads, and
// runs one launch per Gauss-Newton iteration, reading one small record back after each: the host only decides whether to go on.
// tloam_graph_optimize puts the context's graph together from the host's keyframe table and the verified constraints and runs the
// same solve; nothing else in the context is read or written.
// The robust mode wraps that Gauss-Newton run in an outer loop the host drives the same way: one
// k_graph_reweight launch and one small record per outer iteration, then the k_graph_step sequence from the current poses.  With
// the mode off none of it is reserved, uploaded or launched.
#include <float.h>
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

constexpr size_t kGraphMaxNodes = (size_t)1 << 22;   // rows and table entries are 32-bit integers: 12 * edges stays inside them
constexpr size_t kGraphMaxEdges = (size_t)1 << 24;

bool graph_config_ok(const tloam_graph_config& g) {
  auto sigma = [](double v) { return v > 0.0 && v <= DBL_MAX; };
  auto tol = [](double v) { return v >= 0.0 && v <= DBL_MAX; };
  return g.max_iterations >= 1 && g.max_iterations <= 1000 && g.max_cg_iterations >= 1 && g.max_cg_iterations <= 1000000 &&
         tol(g.step_tol) && tol(g.cg_tol) && sigma(g.odom_sigma_t) && sigma(g.odom_sigma_r) && sigma(g.loop_sigma_t) &&
         sigma(g.loop_sigma_r);
}

Pose pose_inverse(const Pose& T) {
  Pose I;
  I.qw = T.qw; I.qx = -T.qx; I.qy = -T.qy; I.qz = -T.qz;
  const Vec3 t = rotate(I, Vec3{T.tx, T.ty, T.tz});
  I.tx = -t.x; I.ty = -t.y; I.tz = -t.z;
  return I;
}

bool robust_config_ok(const tloam_graph_robust_config& r) {
  return r.max_outer >= 1 && r.max_outer <= 10000 && r.noise_chi2 > 0.0 && r.noise_chi2 <= DBL_MAX && r.mu_factor > 1.0 &&
         r.mu_factor <= DBL_MAX;
}

// what a solve reports of the robust mode: the loop edges' final scales and statistics beside the info
struct RobustOut {
  tloam_graph_robust_info info;
  std::vector<double> scale, chi2;
};

void sigma_weights(double st, double sr, double w[6]) {
  for (int a = 0; a < 6; ++a) w[a] = a < 3 ? 1.0 / (st * st) : 1.0 / (sr * sr);
}

// the checked solve behind tloam_graph_solve, tloam_graph_solve_robust and tloam_graph_optimize; robust.enabled == 0: the plain solve
int graph_solve(tloam_ctx* c, const tloam_graph_config& cfg, const tloam_graph_robust_config& robust, size_t n, const double* poses_in,
                size_t m, const tloam_graph_edge* edges, double* poses_out, tloam_graph_info* info, RobustOut* rout) {
  if (n < 1 || n > kGraphMaxNodes || m > kGraphMaxEdges || !poses_in || !poses_out || m < n - 1 || (m > 0 && !edges))
    return TLOAM_E_INVALID;
  std::vector<Pose> P(n), Zinv(m);
  for (size_t k = 0; k < n; ++k)
    if (!pose_from_matrix(poses_in + 16 * k, &P[k])) return TLOAM_E_INVALID;
  for (size_t e = 0; e < m; ++e) {
    const tloam_graph_edge& E = edges[e];
    if (e < n - 1 ? (E.i != (int64_t)e || E.j != (int64_t)e + 1) : (E.i < 0 || E.j < 0 || E.i >= (int64_t)n || E.j >= (int64_t)n || E.i == E.j))
      return TLOAM_E_INVALID;
    for (int a = 0; a < 6; ++a)
      if (!(E.weight[a] >= 0.0 && E.weight[a] <= DBL_MAX) || (e < n - 1 && E.weight[a] == 0.0)) return TLOAM_E_INVALID;
    Pose Z;
    if (!pose_from_matrix(E.rel_pose_colmajor, &Z)) return TLOAM_E_INVALID;
    Zinv[e] = pose_inverse(Z);
  }
  tloam_graph_info I;
  memset(&I, 0, sizeof(I));
  I.n_nodes = (int64_t)n;
  I.n_edges = (int64_t)m;
  I.n_loop_edges = (int64_t)(m - (n - 1));
  I.stop_reason = TLOAM_GRAPH_STOP_NOT_RUN;
  const bool rb = robust.enabled != 0;
  const size_t nl = m - (n - 1);   // loop edges
  RobustOut RO;
  memset(&RO.info, 0, sizeof(RO.info));
  RO.info.stop_reason = rb ? TLOAM_GRAPH_ROBUST_STOP_ALL_INLIERS : TLOAM_GRAPH_ROBUST_STOP_OFF;
  RO.info.kept = (int64_t)nl;
  RO.scale.assign(nl, 1.0);
  RO.chi2.assign(nl, NAN);   // (the plain solve computes no r)
  if (n < 2 || m == n - 1) {   // the chain alone carries no correction: the input's bits
    memmove(poses_out, poses_in, sizeof(double) * 16 * n);
    if (info) *info = I;
    if (rout) *rout = std::move(RO);
    return TLOAM_OK;
  }
  // every node's edge ends, in edge order
  std::vector<int> ints(2 * m + (n + 1) + 2 * m);
  int* ij = ints.data();
  int* start = ij + 2 * m;
  int* ent = start + (n + 1);
  std::vector<double> w(6 * m);
  for (size_t k = 0; k <= n; ++k) start[k] = 0;
  for (size_t e = 0; e < m; ++e) {
    ij[2 * e] = (int)edges[e].i;
    ij[2 * e + 1] = (int)edges[e].j;
    start[edges[e].i + 1]++;
    start[edges[e].j + 1]++;
    memcpy(&w[6 * e], edges[e].weight, sizeof(double) * 6);
  }
  for (size_t k = 0; k < n; ++k) start[k + 1] += start[k];
  {
    std::vector<int> fill(start, start + n);
    for (size_t e = 0; e < m; ++e) {
      ent[fill[edges[e].j]++] = (int)(2 * e);
      ent[fill[edges[e].i]++] = (int)(2 * e + 1);
    }
  }
  // device storage, carved from the context's two grow-only buffers
  GraphState& G = c->graph;
  constexpr size_t kPose = sizeof(Pose) / sizeof(double), kRt = sizeof(Rt) / sizeof(double);
  static_assert(sizeof(Pose) == 7 * sizeof(double) && sizeof(Rt) == 12 * sizeof(double), "carved as doubles");
  const size_t doubles = 2 * kPose * n + kPose * m + 6 * m + kRt * m + 12 * m + 2 * kRt * n + 36 * n + (rb ? 6 * m + 2 * nl : 0);
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (an earlier solve's storage may be replaced below)
  HIPC(c, G.dws.reserve(doubles));
  HIPC(c, G.iws.reserve(ints.size()));
  HIPC(c, G.rec.reserve(1));
  if (rb) HIPC(c, G.rrec.reserve(1));
  double* d = G.dws.p;
  auto take = [&d](size_t count) { double* p = d; d += count; return p; };
  Pose* dP[2] = {(Pose*)take(kPose * n), (Pose*)take(kPose * n)};
  GraphArgs A;
  memset(&A, 0, sizeof(A));
  A.n = (int)n;
  A.m = (int)m;
  A.chunk = (int)((n - 1 + kGraphThreads - 1) / kGraphThreads);
  A.max_cg = cfg.max_cg_iterations;
  A.cg_tol2 = cfg.cg_tol * cfg.cg_tol;
  double* dZ = take(kPose * m);
  double* dw = take(6 * m);
  A.Zinv = (const Pose*)dZ;
  A.w = dw;
  A.A = (Rt*)take(kRt * m);
  A.contrib = take(12 * m);
  A.Q = (Rt*)take(kRt * n);
  A.Qi = (Rt*)take(kRt * n);
  A.x = take(6 * n); A.r = take(6 * n); A.z = take(6 * n); A.p = take(6 * n); A.ap = take(6 * n); A.tmp = take(6 * n);
  A.ij = (const int2*)G.iws.p;
  A.node_start = G.iws.p + 2 * m;
  A.node_ent = G.iws.p + 2 * m + (n + 1);
  A.rec = G.rec.p;
  GraphReweightArgs W;
  memset(&W, 0, sizeof(W));
  if (rb) {   // the base weights, the scales and the statistics: behind the plain solve's arrays
    double* dw0 = take(6 * m);
    W.c2 = robust.noise_chi2;
    W.w0 = dw0;
    W.w = dw;
    W.s = take(nl);
    W.r = take(nl);
    W.rec = G.rrec.p;
  }
  const hipMemcpyKind H2D = hipMemcpyHostToDevice, D2H = hipMemcpyDeviceToHost;
  HIPC(c, hipMemcpyAsync(dP[0], P.data(), sizeof(Pose) * n, H2D, c->stream));
  HIPC(c, hipMemcpyAsync(dZ, Zinv.data(), sizeof(Pose) * m, H2D, c->stream));
  HIPC(c, hipMemcpyAsync(dw, w.data(), sizeof(double) * 6 * m, H2D, c->stream));
  HIPC(c, hipMemcpyAsync(G.iws.p, ints.data(), sizeof(int) * ints.size(), H2D, c->stream));
  if (rb) HIPC(c, hipMemcpyAsync((double*)W.w0, w.data(), sizeof(double) * 6 * m, H2D, c->stream));
  int cur = 0;
  // Gauss-Newton from dP[cur] with the weights in dw: one launch and one record per iteration
  auto gauss_newton = [&]() -> int {
    double cost = 0.0;
    bool limit = false;
    I.iterations = 0;
    I.reverted = 0;
    I.cg_iterations = 0;
    I.stop_reason = TLOAM_GRAPH_STOP_ITERATIONS;
    for (int it = 0; it < cfg.max_iterations; ++it) {
      A.P = dP[cur];
      A.Pn = dP[cur ^ 1];
      launch_graph_step(A, c->stream);
      HIPC(c, hipGetLastError());
      GraphRecord R;
      HIPC(c, hipMemcpyAsync(&R, G.rec.p, sizeof(R), D2H, c->stream));
      HIPC(c, hipStreamSynchronize(c->stream));
      if (it == 0) I.initial_cost = cost = R.cost_before;
      I.iterations = it + 1;
      I.cg_iterations += R.cg_iterations;
      I.last_step = R.max_step;
      I.last_cg_residual = R.cg_residual;
      limit = R.cg_limit != 0;
      const bool small = R.max_step < cfg.step_tol;   // (a step below step_tol is kept on its size: the cost no longer resolves it)
      if (!std::isfinite(R.cost_after) || (R.cost_after > cost && !small)) {
        I.stop_reason = TLOAM_GRAPH_STOP_COST;
        I.reverted = 1;
        break;
      }
      cur ^= 1;
      cost = R.cost_after;
      if (small) {
        I.stop_reason = TLOAM_GRAPH_STOP_STEP;
        break;
      }
    }
    if (limit && I.stop_reason != TLOAM_GRAPH_STOP_COST) I.stop_reason = TLOAM_GRAPH_STOP_CG_LIMIT;
    I.final_cost = cost;
    return TLOAM_OK;
  };
  int rc = gauss_newton();
  if (rc != TLOAM_OK) return rc;
  if (rb) {
    // the outer loop: the loop edges' r and scales by one launch and one record, then Gauss-Newton again from where it stands
    tloam_graph_robust_info& RI = RO.info;
    GraphRobustRecord R;
    auto reweight = [&](int mode, double mu) -> int {
      A.P = dP[cur];
      W.mode = mode;
      W.mu = mu;
      launch_graph_reweight(A, W, c->stream);
      HIPC(c, hipGetLastError());
      HIPC(c, hipMemcpyAsync(&R, G.rrec.p, sizeof(R), D2H, c->stream));
      HIPC(c, hipStreamSynchronize(c->stream));
      return TLOAM_OK;
    };
    const double first_cost = I.initial_cost, c2 = robust.noise_chi2;
    RI.gn_iterations = I.iterations;
    RI.cg_iterations = I.cg_iterations;
    if ((rc = reweight(kGraphReweightOnes, 0.0)) != TLOAM_OK) return rc;
    RI.max_chi2_first = R.max_r;
    if (!(R.max_r <= c2)) {
      double mu = c2 / (2.0 * R.max_r - c2);
      RI.mu_first = mu;
      RI.stop_reason = TLOAM_GRAPH_ROBUST_STOP_OUTER_LIMIT;
      for (int t = 1; t <= robust.max_outer; ++t) {
        if ((rc = reweight(kGraphReweightRule, mu)) != TLOAM_OK) return rc;
        const bool binary = R.undecided == 0;   // (the scales do not depend on the solve that follows)
        if ((rc = gauss_newton()) != TLOAM_OK) return rc;
        RI.outer_iterations = t;
        RI.mu_last = mu;
        RI.gn_iterations += I.iterations;
        RI.cg_iterations += I.cg_iterations;
        if (binary) {
          RI.stop_reason = TLOAM_GRAPH_ROBUST_STOP_BINARY;
          break;
        }
        mu = mu * robust.mu_factor;
      }
      if ((rc = reweight(kGraphReweightKeep, 0.0)) != TLOAM_OK) return rc;   // r at the result
    }
    RI.rejected = R.rejected;
    RI.kept = R.kept;
    RI.undecided = R.undecided;
    I.initial_cost = first_cost;
    HIPC(c, hipMemcpyAsync(RO.scale.data(), W.s, sizeof(double) * nl, D2H, c->stream));
    HIPC(c, hipMemcpyAsync(RO.chi2.data(), W.r, sizeof(double) * nl, D2H, c->stream));
  }
  HIPC(c, hipMemcpyAsync(P.data(), dP[cur], sizeof(Pose) * n, D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  double first[16];
  memcpy(first, poses_in, sizeof(first));   // (node 0 is fixed: its input's bits, also when the arrays are one)
  for (size_t k = 1; k < n; ++k) pose_to_matrix(P[k], poses_out + 16 * k);
  memcpy(poses_out, first, sizeof(first));
  if (info) *info = I;
  if (rout) *rout = std::move(RO);
  return TLOAM_OK;
}

}  // namespace

namespace tlh {
void graph_correct_pose(const tloam_ctx* c, size_t keyframe, const double pose_in[16], double pose_out[16]) {
  double inv[16], delta[16];
  rigid_inverse(c->place.kf[keyframe].pose, inv);
  mat_mul(&c->graph.corrected[16 * keyframe], inv, delta);
  mat_mul(delta, pose_in, pose_out);
}
}  // namespace tlh

extern "C" {

void tloam_graph_default_config(tloam_graph_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_iterations = 30;
  cfg->max_cg_iterations = 20000;
  cfg->step_tol = 1e-7;      // below it a step's change of the cost is rounding (measured)
  cfg->cg_tol = 1e-10;       // keeps the poses within 1e-10 of a direct solve's (measured)
  cfg->odom_sigma_t = 0.05;  // a keyframe step's odometry: not measured, DESIGN.md 18
  cfg->odom_sigma_r = 0.005;
  cfg->loop_sigma_t = 0.05;  // measured worst case of a verified loop
  cfg->loop_sigma_r = 0.01;
}

int tloam_graph_configure(tloam_ctx* c, const tloam_graph_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_graph_config want = cfg_or_default(cfg, tloam_graph_default_config);
  if (!graph_config_ok(want)) return TLOAM_E_INVALID;
  c->graph.cfg = want;
  c->graph.drop();
  return TLOAM_OK;
}

int tloam_graph_solve(tloam_ctx* c, const tloam_graph_config* cfg, size_t n_nodes, const double* poses_in, size_t n_edges,
                      const tloam_graph_edge* edges, double* poses_out, tloam_graph_info* info) {
  if (!c || c->nranks > 1 || (cfg && !graph_config_ok(*cfg))) return TLOAM_E_INVALID;
  const tloam_graph_robust_config off{};
  return graph_solve(c, cfg ? *cfg : c->graph.cfg, off, n_nodes, poses_in, n_edges, edges, poses_out, info, nullptr);
}

void tloam_graph_robust_default_config(tloam_graph_robust_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->enabled = 0;
  cfg->max_outer = 100;
  cfg->noise_chi2 = 36.0;   // 16.81 (chi-squared, 6 degrees of freedom, 99 %) rejected true edges (measured)
  cfg->mu_factor = 1.4;     // the usual GNC value
}

int tloam_graph_robust_configure(tloam_ctx* c, const tloam_graph_robust_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_graph_robust_config want = cfg_or_default(cfg, tloam_graph_robust_default_config);
  if (!robust_config_ok(want)) return TLOAM_E_INVALID;
  c->graph.rcfg = want;
  c->graph.drop();
  return TLOAM_OK;
}

int tloam_graph_solve_robust(tloam_ctx* c, const tloam_graph_config* cfg, const tloam_graph_robust_config* rcfg, size_t n_nodes,
                             const double* poses_in, size_t n_edges, const tloam_graph_edge* edges, double* poses_out,
                             tloam_graph_info* info, tloam_graph_robust_info* rinfo, double* loop_scale_out, double* loop_chi2_out) {
  if (!c || c->nranks > 1 || (cfg && !graph_config_ok(*cfg)) || (rcfg && !robust_config_ok(*rcfg))) return TLOAM_E_INVALID;
  RobustOut RO;
  const int rc = graph_solve(c, cfg ? *cfg : c->graph.cfg, rcfg ? *rcfg : c->graph.rcfg, n_nodes, poses_in, n_edges, edges, poses_out,
                             info, &RO);
  if (rc != TLOAM_OK) return rc;
  if (rinfo) *rinfo = RO.info;
  if (loop_scale_out && !RO.scale.empty()) memcpy(loop_scale_out, RO.scale.data(), sizeof(double) * RO.scale.size());
  if (loop_chi2_out && !RO.chi2.empty()) memcpy(loop_chi2_out, RO.chi2.data(), sizeof(double) * RO.chi2.size());
  return TLOAM_OK;
}

int tloam_graph_optimize(tloam_ctx* c, tloam_graph_info* info) {
  if (!c || c->nranks > 1 || !c->place.cfg.enabled) return TLOAM_E_INVALID;
  const PlaceState& P = c->place;
  GraphState& G = c->graph;
  const size_t n = P.kf.size();
  std::vector<double> poses(16 * n);
  for (size_t k = 0; k < n; ++k) memcpy(&poses[16 * k], P.kf[k].pose, sizeof(double) * 16);
  std::vector<tloam_graph_edge> edges;
  tloam_graph_edge E;
  memset(&E, 0, sizeof(E));
  sigma_weights(G.cfg.odom_sigma_t, G.cfg.odom_sigma_r, E.weight);
  for (size_t k = 0; k + 1 < n; ++k) {
    double inv[16];
    E.i = (int64_t)k;
    E.j = (int64_t)k + 1;
    rigid_inverse(P.kf[k].pose, inv);
    mat_mul(inv, P.kf[k + 1].pose, E.rel_pose_colmajor);
    edges.push_back(E);
  }
  sigma_weights(G.cfg.loop_sigma_t, G.cfg.loop_sigma_r, E.weight);
  std::vector<int64_t> constraint;   // a loop edge's constraint
  for (size_t k = 0; k < c->loop.out.size(); ++k) {
    const tloam_loop_constraint& L = c->loop.out[k];
    if (!L.accepted) continue;
    constraint.push_back((int64_t)k);
    E.i = L.match_keyframe;
    E.j = L.query_keyframe;
    memcpy(E.rel_pose_colmajor, L.rel_pose_colmajor, sizeof(E.rel_pose_colmajor));
    edges.push_back(E);
  }
  tloam_graph_info I;
  memset(&I, 0, sizeof(I));
  std::vector<double> out(16 * n);
  RobustOut RO;
  memset(&RO.info, 0, sizeof(RO.info));
  RO.info.stop_reason = G.rcfg.enabled ? TLOAM_GRAPH_ROBUST_STOP_ALL_INLIERS : TLOAM_GRAPH_ROBUST_STOP_OFF;
  if (n >= 1) {
    const int rc = graph_solve(c, G.cfg, G.rcfg, n, poses.data(), edges.size(), edges.data(), out.data(), &I, &RO);
    if (rc != TLOAM_OK) return rc;
  }
  G.corrected.swap(out);
  G.rinfo = RO.info;
  G.loop_constraint.swap(constraint);
  G.loop_scale.swap(RO.scale);
  G.loop_chi2.swap(RO.chi2);
  G.have = true;
  if (info) *info = I;
  return TLOAM_OK;
}

int tloam_graph_read_poses(tloam_ctx* c, size_t first, size_t count, double* poses) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const GraphState& G = c->graph;
  if (!G.have) return TLOAM_E_NOT_READY;
  const size_t n = G.corrected.size() / 16;
  if (first > n || count > n - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!poses) return TLOAM_E_INVALID;
  memcpy(poses, G.corrected.data() + 16 * first, sizeof(double) * 16 * count);
  return TLOAM_OK;
}

int tloam_graph_read_loop_scales(tloam_ctx* c, size_t first, size_t count, int64_t* constraint_index, double* scale, double* chi2) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const GraphState& G = c->graph;
  if (!G.have) return TLOAM_E_NOT_READY;
  const size_t nl = G.loop_scale.size();
  if (first > nl || count > nl - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (constraint_index) memcpy(constraint_index, G.loop_constraint.data() + first, sizeof(int64_t) * count);
  if (scale) memcpy(scale, G.loop_scale.data() + first, sizeof(double) * count);
  if (chi2) memcpy(chi2, G.loop_chi2.data() + first, sizeof(double) * count);
  return TLOAM_OK;
}

int tloam_graph_get_robust_info(tloam_ctx* c, tloam_graph_robust_info* out) {
  if (!c || c->nranks > 1 || !out) return TLOAM_E_INVALID;
  if (!c->graph.have) return TLOAM_E_NOT_READY;
  *out = c->graph.rinfo;
  return TLOAM_OK;
}

int tloam_graph_correct_pose(tloam_ctx* c, int64_t keyframe, const double pose_in[16], double pose_out[16]) {
  if (!c || c->nranks > 1 || !pose_in || !pose_out) return TLOAM_E_INVALID;
  const GraphState& G = c->graph;
  if (!G.have) return TLOAM_E_NOT_READY;
  const int64_t n = (int64_t)(G.corrected.size() / 16);
  if (keyframe == -1) keyframe = n - 1;
  if (keyframe < 0 || keyframe >= n || (size_t)keyframe >= c->place.kf.size()) return TLOAM_E_INVALID;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(pose_in[i])) return TLOAM_E_INVALID;
  tlh::graph_correct_pose(c, (size_t)keyframe, pose_in, pose_out);
  return TLOAM_OK;
}

}  // extern "C"
