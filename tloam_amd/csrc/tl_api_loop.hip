// tl_api_loop.hip -- C ABI of loop verification (include/tloam_hip.h: tloam_loop_*, tloam_place_*_keyframe_clouds; DESIGN.md
// section 17; kernels in tl_loop.hip).
//
// The keyframe clouds are kept by the odometry frame (tl_api_odom.hip notes the spans, tl_api_place.hip commits them with the
// keyframe).  A verification runs on two private child contexts of the parent's device, so that nothing the parent has
// registered, built or returned changes: the coarse stage's context (the configuration's `coarse` TLS values) and the fine
// stage's (the parent's own TLS values).  k_loop_assemble writes the query's source clouds into the coarse context's source block
// and the window's moved target clouds into the parent's scratch, from which both contexts take their targets through the path
// of tloam_set_target_frame (device to device); the fine context's source block is a device copy of the coarse one's.  Then two
// plain tloam_scan_match calls, and k_loop_score over the fine context's grids.
#include <float.h>
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

bool pos_finite(double v) { return v > 0.0 && v <= DBL_MAX; }

// the values tloam_scan_match can run with
bool tls_config_ok(const tloam_tls_config& t) {
  return t.factor_num >= 2 && t.factor_num <= 4 && pos_finite(t.edge_dist_thres) && pos_finite(t.sphere_dist_thres) &&
         pos_finite(t.planar_dist_thres) && pos_finite(t.ground_dist_thres) && std::isfinite(t.edge_dir_thres) &&
         t.edge_maxnum >= 1 && t.sphere_maxnum >= 1 && t.planar_maxnum >= 1 && t.ground_maxnum >= 1 &&
         t.max_iterations >= 1 && t.max_iterations <= 1000 && std::isfinite(t.cost_threshold) && t.cost_threshold >= 0.0 &&
         pos_finite(t.gnc_factor) && pos_finite(t.noise_bound) && pos_finite(t.fitness_thres);
}

bool loop_config_ok(const tloam_loop_config& L) {
  return (L.enabled == 0 || L.enabled == 1) && L.window >= 0 && L.window <= (1 << 20) && (L.init_mode == 0 || L.init_mode == 1) &&
         pos_finite(L.inlier_dist) && pos_finite(L.min_overlap) && L.min_overlap <= 1.0 && pos_finite(L.max_rmse) &&
         L.reserve_points >= 0 && L.reserve_points <= (int64_t)kMaxPoints && tls_config_ok(L.coarse);
}

void rigid_rows(const double T[16], double R[9], double t[3]) {   // column-major 4x4 -> row-major R, t
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = T[4 * j + i];
    t[i] = T[12 + i];
  }
}

// the score's reach in cells: every target within inlier_dist of a query lies within ceil(inlier_dist / cell) cells of the
// query's cell in each direction.  Formed in double and bounded before the cast (inlier_dist may be anything up to DBL_MAX):
// a query's cell coordinate lies in [-2, dim + 1] (cell_coord), so a reach of the largest dimension + 2 already walks the whole
// grid from anywhere, and cx + reach stays far inside int (a table holds at most 4e6 cells)
int score_reach(double inlier_dist, const GridView& g) {
  const double cells = ceil(inlier_dist * g.inv_cell);
  const int whole = std::max(g.dim[0], std::max(g.dim[1], g.dim[2])) + 2;
  if (!(cells > 1.0)) return 1;
  return cells >= (double)whole ? whole : (int)cells;
}

void drop_child(tloam_ctx*& ch) {
  if (ch) tloam_destroy(ch);
  ch = nullptr;
}

// the two child contexts for the configuration at hand (created, or rebuilt when it changed)
int ensure_children(tloam_ctx* c) {
  LoopState& L = c->loop;
  if (L.coarse && memcmp(&L.coarse->cfg, &L.cfg.coarse, sizeof(tloam_tls_config)) != 0) drop_child(L.coarse);
  if (L.fine && memcmp(&L.fine->cfg, &c->cfg, sizeof(tloam_tls_config)) != 0) drop_child(L.fine);
  int rc = TLOAM_OK;
  if (!L.coarse) rc = tloam_create(&L.cfg.coarse, c->device, &L.coarse);
  if (rc == TLOAM_OK && !L.fine) rc = tloam_create(&c->cfg, c->device, &L.fine);
  HIPC(c, hipSetDevice(c->device));
  if (rc != TLOAM_OK) c->last_error = "loop verification: creating a stage's context failed";
  return rc;
}

// spans -> launches of at most kLoopSpans spans each
void assemble(const std::vector<LoopSpan>& spans, hipStream_t s) {
  for (size_t b = 0; b < spans.size(); b += kLoopSpans) {
    LoopSpanArgs A;
    memset(&A, 0, sizeof(A));
    A.nspan = (int)std::min<size_t>(kLoopSpans, spans.size() - b);
    A.start[0] = 0;
    for (int j = 0; j < A.nspan; ++j) {
      A.s[j] = spans[b + j];
      A.start[j + 1] = A.start[j] + A.s[j].n;
    }
    launch_loop_assemble(A, s);
  }
}

// one verification of (q, m) from `init` into *o (whose dist / yaw the caller sets).  Returns TLOAM_OK unless the device failed;
// the verification's own outcome is o->status
int verify(tloam_ctx* c, int64_t q, int64_t m, const double init[16], tloam_loop_constraint* o) {
  PlaceState& P = c->place;
  LoopState& L = c->loop;
  const PlaceState::Keyframe& Kq = P.kf[(size_t)q];
  const PlaceState::Keyframe& Km = P.kf[(size_t)m];
  o->query_keyframe = q; o->query_frame = Kq.frame;
  o->match_keyframe = m; o->match_frame = Km.frame;
  memcpy(o->init_colmajor, init, sizeof(o->init_colmajor));
  memcpy(o->rel_pose_colmajor, init, sizeof(o->rel_pose_colmajor));
  o->accepted = 0;
  // the window: keyframes [m - window, m + window] clamped to [0, q - 1], ascending
  const int64_t lo = std::max<int64_t>(m - L.cfg.window, 0), hi = std::min<int64_t>(m + L.cfg.window, q - 1);
  size_t nsrc[kKinds], ntgt[kKinds] = {0, 0, 0, 0}, all_src = 0, all_tgt = 0;
  for (int k = 0; k < kKinds; ++k) {
    nsrc[k] = Kq.n[k];
    for (int64_t j = lo; j <= hi; ++j) ntgt[k] += P.kf[(size_t)j].n[4 + k];
    all_src += nsrc[k];
    all_tgt += ntgt[k];
  }
  if (all_src == 0 || all_tgt == 0) {
    o->status = TLOAM_E_NOT_READY;
    return TLOAM_OK;
  }
  int rc = ensure_children(c);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, hipStreamSynchronize(c->stream));   // (the arena's last commit)
  tloam_ctx* A = L.coarse;
  tloam_ctx* B = L.fine;
  // the coarse context's source block and the target scratch, laid out as the hand-over lays them out
  size_t cnt4[kKinds], soff[kKinds], tcnt[kKinds], toff[kKinds];
  rc = source_frame_reserve(A, nsrc, cnt4);
  if (rc != TLOAM_OK) return rc;
  staged_offsets(cnt4, kKinds, soff);
  for (int k = 0; k < kKinds; ++k) tcnt[k] = 3 * ntgt[k];
  const size_t ttotal = staged_offsets(tcnt, kKinds, toff);
  HIPC(c, L.tgt.reserve(std::max<size_t>(ttotal, 3)));
  std::vector<LoopSpan> spans;
  LoopSpan s;
  memset(&s, 0, sizeof(s));
  for (int k = 0; k < kKinds; ++k) {   // the query's source clouds, as they are
    s.src = P.arena.p + Kq.off[k]; s.dst = A->src_pack.p + soff[k]; s.n = (long long)nsrc[k]; s.rigid = 0;
    if (s.n) spans.push_back(s);
  }
  double inv_m[16];
  rigid_inverse(Km.pose, inv_m);
  for (int k = 0; k < kKinds; ++k) {   // the window's target clouds, in m's frame
    size_t at = toff[k];
    for (int64_t j = lo; j <= hi; ++j) {
      const PlaceState::Keyframe& Kj = P.kf[(size_t)j];
      if (!Kj.n[4 + k]) continue;
      double T[16];
      mat_mul(inv_m, Kj.pose, T);
      s.src = P.arena.p + Kj.off[4 + k]; s.dst = L.tgt.p + at; s.n = (long long)Kj.n[4 + k]; s.rigid = 1;
      rigid_rows(T, s.R, s.t);
      spans.push_back(s);
      at += 3 * Kj.n[4 + k];
    }
  }
  HIPC(c, hipSetDevice(c->device));
  assemble(spans, A->stream);
  source_frame_commit(A, true, soff);
  const double* tp[kKinds];
  for (int k = 0; k < kKinds; ++k) tp[k] = L.tgt.p + toff[k];
  rc = set_target_frame_from(A, tp, ntgt, hipMemcpyDeviceToDevice);   // (waits for A's stream: the assembly is done after it)
  if (rc != TLOAM_OK) { c->last_error = A->last_error; return rc; }
  size_t cnt4b[kKinds];
  rc = source_frame_reserve(B, nsrc, cnt4b);
  if (rc != TLOAM_OK) { c->last_error = B->last_error; return rc; }
  HIPC(c, hipMemcpyAsync(B->src_pack.p, A->src_pack.p, sizeof(double) * staged_size(cnt4, kKinds), hipMemcpyDeviceToDevice,
                         B->stream));
  source_frame_commit(B, true, soff);
  rc = set_target_frame_from(B, tp, ntgt, hipMemcpyDeviceToDevice);
  if (rc != TLOAM_OK) { c->last_error = B->last_error; return rc; }
  // the coarse stage from the initial guess, the fine one from its result
  double r1[16], r2[16];
  const int rc1 = tloam_scan_match(A, init, nullptr, r1, nullptr, 0, &o->coarse);
  if (rc1 == TLOAM_E_HIP || rc1 == TLOAM_E_RCCL) { c->last_error = A->last_error; HIPC(c, hipSetDevice(c->device)); return rc1; }
  if (rc1 != TLOAM_OK && rc1 != TLOAM_E_WEIGHT_RANGE) {
    o->status = rc1;
    HIPC(c, hipSetDevice(c->device));
    return TLOAM_OK;
  }
  const int rc2 = tloam_scan_match(B, r1, nullptr, r2, nullptr, 0, &o->fine);
  HIPC(c, hipSetDevice(c->device));
  if (rc2 == TLOAM_E_HIP || rc2 == TLOAM_E_RCCL) { c->last_error = B->last_error; return rc2; }
  o->status = rc1 != TLOAM_OK ? rc1 : rc2;
  if (rc2 != TLOAM_OK && rc2 != TLOAM_E_WEIGHT_RANGE) {
    memcpy(o->rel_pose_colmajor, r1, sizeof(r1));
    return TLOAM_OK;
  }
  memcpy(o->rel_pose_colmajor, r2, sizeof(r2));
  // the score over the fine stage's grids
  LoopScoreArgs S;
  memset(&S, 0, sizeof(S));
  for (int k = 0; k < kKinds; ++k) {
    const KindData& K = B->kd[k];
    S.src[k] = K.src_ptr;
    S.n[k] = (long long)K.n_src;
    if (K.grid_valid && K.n_tgt > 0) {
      S.g[k] = K.gv;
      S.reach[k] = score_reach(L.cfg.inlier_dist, K.gv);
    }
  }
  rigid_rows(r2, S.R, S.t);
  S.r2 = L.cfg.inlier_dist * L.cfg.inlier_dist;
  const size_t np = (size_t)kLoopScoreBlocks * kKinds * 2;
  HIPC(c, L.partial.reserve(np));
  S.partial = L.partial.p;
  launch_loop_score(S, B->stream);
  std::vector<double> part(np);
  HIPC(c, hipMemcpyAsync(part.data(), L.partial.p, sizeof(double) * np, hipMemcpyDeviceToHost, B->stream));
  HIPC(c, hipStreamSynchronize(B->stream));
  double inl = 0.0, ss = 0.0;
  size_t pts = 0;
  for (int k = 0; k < kKinds; ++k) {   // blocks in order, then kinds in order
    double ck = 0.0, sk = 0.0;
    for (int b = 0; b < kLoopScoreBlocks; ++b) {
      ck = ck + part[((size_t)b * kKinds + k) * 2];
      sk = sk + part[((size_t)b * kKinds + k) * 2 + 1];
    }
    inl = inl + ck;
    ss = ss + sk;
    pts += (size_t)S.n[k];
  }
  o->inliers = (int64_t)inl;
  o->points = (int64_t)pts;
  o->overlap = pts ? inl / (double)pts : 0.0;
  o->rmse = inl > 0.0 ? sqrt(ss / inl) : INFINITY;
  o->accepted = o->status == TLOAM_OK && o->overlap >= L.cfg.min_overlap && o->rmse <= L.cfg.max_rmse;
  return TLOAM_OK;
}

bool loop_on(const tloam_ctx* c) { return c && c->nranks == 1 && c->loop.cfg.enabled; }

}  // namespace

namespace tlh {
bool loop_config_valid(const tloam_loop_config& cfg) { return loop_config_ok(cfg); }

void loop_release(tloam_ctx* c) {
  LoopState& L = c->loop;
  drop_child(L.coarse);
  drop_child(L.fine);
  (void)hipSetDevice(c->device);
  LoopState fresh;   // (the scratch freed, the constraints gone; the configuration stays)
  fresh.cfg = L.cfg;
  fresh.cfg_set = L.cfg_set;
  L = std::move(fresh);
}
}  // namespace tlh

extern "C" {

void tloam_loop_default_config(tloam_loop_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->enabled = 0;
  cfg->window = 2;
  cfg->init_mode = 0;
  cfg->inlier_dist = 0.3;
  cfg->min_overlap = 0.6;    // measured: positives >= 0.70, pairs 15 m apart <= 0.52
  cfg->max_rmse = 0.2;       // measured: positives <= 0.13
  cfg->reserve_points = 0;
  tloam_default_config(&cfg->coarse);   // the shipped values, the distance thresholds doubled (measured: DESIGN.md 17)
  cfg->coarse.edge_dist_thres *= 2.0;
  cfg->coarse.sphere_dist_thres *= 2.0;
  cfg->coarse.planar_dist_thres *= 2.0;
  cfg->coarse.ground_dist_thres *= 2.0;
  cfg->coarse.max_iterations = 8;
}

int tloam_loop_configure(tloam_ctx* c, const tloam_loop_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_loop_config want = cfg_or_default(cfg, tloam_loop_default_config);
  if (!loop_config_ok(want)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  PlaceState& P = c->place;
  LoopState& L = c->loop;
  P.clear(c->stream);   // (the keyframe database empties, as tloam_place_configure empties it)
  P.retired.release();
  P.in_flight = false;
  P.arena.release();
  L.clear();
  c->graph.drop();   // (the corrected poses are those of keyframes that are gone)
  c->cmap.drop();    // (so is the closed map)
  L.cfg = want;
  L.cfg_set = true;
  if (!want.enabled) {
    loop_release(c);
    L.cfg = want;
    return TLOAM_OK;
  }
  const size_t first = 3 * (want.reserve_points > 0 ? (size_t)want.reserve_points : ((size_t)1 << 20));
  int rc = arena_grow(c, first);
  if (rc == TLOAM_OK) {
    HIPC(c, hipStreamSynchronize(c->stream));
    P.retired.release();
  } else {
    L.cfg.enabled = 0;
  }
  return rc;
}

int tloam_loop_get_info(tloam_ctx* c, tloam_loop_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  memset(info, 0, sizeof(*info));
  const LoopState& L = c->loop;
  info->n_constraints = (int64_t)L.out.size();
  for (const tloam_loop_constraint& k : L.out) info->n_accepted += k.accepted ? 1 : 0;
  info->arena_points = (int64_t)(c->place.arena_used / 3);
  info->arena_capacity_points = (int64_t)(c->place.arena.cap / 3);
  return TLOAM_OK;
}

int tloam_place_set_keyframe_clouds(tloam_ctx* c, int64_t kf, const double* const src[4], const size_t n_src[4],
                                    const double* const tgt[4], const size_t n_tgt[4]) {
  if (!loop_on(c) || kf < 0 || kf >= c->place.n_kf || (src && !n_src) || (tgt && !n_tgt)) return TLOAM_E_INVALID;
  size_t all = 0;
  for (int side = 0; side < 2; ++side) {
    const double* const* xyz = side ? tgt : src;
    const size_t* n = side ? n_tgt : n_src;
    if (!xyz) continue;
    for (int k = 0; k < kKinds; ++k) {
      if (n[k] > kMaxPoints || (n[k] > 0 && !xyz[k])) return TLOAM_E_INVALID;
      all += 3 * n[k];
    }
  }
  PlaceState& P = c->place;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (not a frame: whatever is in flight may read the storage replaced below)
  P.retired.release();
  P.in_flight = false;
  const int rc = arena_grow(c, all);
  if (rc != TLOAM_OK) return rc;
  PlaceState::Keyframe& K = P.kf[(size_t)kf];
  for (int side = 0; side < 2; ++side) {
    const double* const* xyz = side ? tgt : src;
    const size_t* n = side ? n_tgt : n_src;
    if (!xyz) continue;
    for (int k = 0; k < kKinds; ++k) {
      K.off[4 * side + k] = P.arena_used;
      K.n[4 * side + k] = n[k];
      if (n[k])
        HIPC(c, hipMemcpyAsync(P.arena.p + P.arena_used, xyz[k], sizeof(double) * 3 * n[k], hipMemcpyHostToDevice, c->stream));
      P.arena_used += 3 * n[k];
    }
  }
  HIPC(c, hipStreamSynchronize(c->stream));
  P.retired.release();
  return TLOAM_OK;
}

int tloam_place_read_keyframe_clouds(tloam_ctx* c, int64_t kf, int side, int kind, size_t capacity, size_t* n, double* out) {
  if (!loop_on(c) || !n || kf < 0 || kf >= c->place.n_kf || side < 0 || side > 1 || kind < 0 || kind >= kKinds)
    return TLOAM_E_INVALID;
  const PlaceState::Keyframe& K = c->place.kf[(size_t)kf];
  const size_t m = K.n[4 * side + kind];
  *n = m;
  if (!out) return TLOAM_OK;
  if (capacity < m) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (m)
    HIPC(c, hipMemcpyAsync(out, c->place.arena.p + K.off[4 * side + kind], sizeof(double) * 3 * m, hipMemcpyDeviceToHost,
                           c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_loop_verify_pending(tloam_ctx* c, int64_t* n_verified) {
  if (n_verified) *n_verified = 0;
  if (!loop_on(c)) return TLOAM_E_INVALID;
  PlaceState& P = c->place;
  LoopState& L = c->loop;
  HIPC(c, hipSetDevice(c->device));
  unsigned long long nl = 0;
  if (P.ctl.p) HIPC(c, hipMemcpyAsync(&nl, P.ctl.p, sizeof(nl), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (nl <= L.next_record) return TLOAM_OK;
  std::vector<tloam_place_loop> recs((size_t)nl - L.next_record);
  HIPC(c, hipMemcpyAsync(recs.data(), P.loops.p + L.next_record, sizeof(tloam_place_loop) * recs.size(), hipMemcpyDeviceToHost,
                         c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  for (const tloam_place_loop& R : recs) {
    tloam_loop_constraint o;
    memset(&o, 0, sizeof(o));
    const int64_t q = R.query_keyframe, m = R.match_keyframe;
    double init[16];
    if (L.cfg.init_mode == 0) {   // Rz(yaw), no translation: Scan Context's heading
      const double cy = cos(R.yaw), sy = sin(R.yaw);
      const double Rz[16] = {cy, sy, 0, 0, -sy, cy, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      memcpy(init, Rz, sizeof(init));
    } else {
      double inv_m[16];
      rigid_inverse(P.kf[(size_t)m].pose, inv_m);
      mat_mul(inv_m, P.kf[(size_t)q].pose, init);
    }
    const int rc = verify(c, q, m, init, &o);
    if (rc != TLOAM_OK) return rc;
    o.dist = R.dist;
    o.yaw = R.yaw;
    L.out.push_back(o);
    L.next_record++;
    if (n_verified) (*n_verified)++;
  }
  return TLOAM_OK;
}

int tloam_loop_verify_pair(tloam_ctx* c, int64_t q, int64_t m, const double init_or_null[16], tloam_loop_constraint* out) {
  if (!loop_on(c) || !out || m < 0 || q <= m || q >= c->place.n_kf) return TLOAM_E_INVALID;
  const PlaceState& P = c->place;
  double init[16];
  if (init_or_null) {
    for (int i = 0; i < 16; ++i)
      if (!std::isfinite(init_or_null[i])) return TLOAM_E_INVALID;
    memcpy(init, init_or_null, sizeof(init));
  } else {
    double inv_m[16];
    rigid_inverse(P.kf[(size_t)m].pose, inv_m);
    mat_mul(inv_m, P.kf[(size_t)q].pose, init);
  }
  HIPC(c, hipSetDevice(c->device));
  tloam_loop_constraint o;
  memset(&o, 0, sizeof(o));
  const int rc = verify(c, q, m, init, &o);
  if (rc != TLOAM_OK) return rc;
  *out = o;
  return TLOAM_OK;
}

int tloam_loop_read_constraints(tloam_ctx* c, size_t first, size_t count, tloam_loop_constraint* out) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const size_t n = c->loop.out.size();
  if (first > n || count > n - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!out) return TLOAM_E_INVALID;
  memcpy(out, c->loop.out.data() + first, sizeof(tloam_loop_constraint) * count);
  return TLOAM_OK;
}

}  // extern "C"
