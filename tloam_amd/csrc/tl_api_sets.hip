// tl_api_sets.hip -- the factor set a frame left behind or a host supplied (tloam_set_correspondences), outside a frame: read
// (tloam_get_correspondences / _weights / _costs / _normal_equations), evaluated and solved (tloam_accumulate, tloam_solve),
// timed for the bench (tloam_time_*, the four timers) -- and what else a host asks between frames: getFitnessScore
// (tloam_fitness), a radius search (tloam_knn), the tloam_debug_* aids.  The frame itself is tl_api_match.hip; the helpers the
// two units share are declared under its name in tl_ctx.hpp.
#include "tl_ctx.hpp"

using namespace tl;

namespace {

int res_kind(int res_type) {
  return res_type == TLOAM_RES_PLANE ? TLOAM_KIND_PLANAR : (res_type == TLOAM_RES_LINE ? TLOAM_KIND_EDGE : TLOAM_KIND_SPHERE);
}

// the current set evaluated at se3: the next sweep's linearisation point
int eval_at(tloam_ctx* c, const double se3[6]) {
  memcpy(c->h_small, se3, sizeof(double) * 6);
  HIPC(c, hipMemcpyAsync(c->se3_dev.p, c->h_small, sizeof(double) * 6, hipMemcpyHostToDevice, c->stream));
  launch_set_eval(c->state.p, c->se3_dev.p, c->stream);
  return TLOAM_OK;
}

// body(0) .. body(launches - 1), stopping at the first status that is not TLOAM_OK, bracketed by one HIP event pair on the
// context's stream; *mean_us is the bracket over `launches`.  The pair is destroyed on every path out.
template <class Body>
int timed_launches(tloam_ctx* c, int launches, Body body, double* mean_us) {
  struct Pair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Pair() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  HIPC(c, hipEventCreate(&ev.e0));
  HIPC(c, hipEventCreate(&ev.e1));
  HIPC(c, hipEventRecord(ev.e0, c->stream));
  int rc = TLOAM_OK;
  for (int i = 0; i < launches && rc == TLOAM_OK; ++i) rc = body(i);
  HIPC(c, hipEventRecord(ev.e1, c->stream));
  HIPC(c, hipEventSynchronize(ev.e1));
  float ms = 0.f;
  HIPC(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *mean_us = (double)ms * 1e3 / launches;
  return rc;
}

// a device span counter (K3Step::span, iter_span_note: word 1 the ticks of the 100 MHz wall clock, word 2 the count), read and
// on request reset; zeros before the context has one
int read_span(tloam_ctx* c, const DBuf<unsigned long long>& span, int reset, double* total_us, int64_t* count) {
  HIPC(c, hipSetDevice(c->device));
  unsigned long long h[4] = {0, 0, 0, 0};
  if (span.p) {
    HIPC(c, hipMemcpyAsync(h, span.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (reset) HIPC(c, hipMemsetAsync(span.p, 0, sizeof(h), c->stream));
  }
  if (total_us) *total_us = (double)h[1] * 0.01;
  if (count) *count = (int64_t)h[2];
  return TLOAM_OK;
}

// A direct set through the getters is rebuilt first if it is stale.
// The rows then hold the geometry of a search that ran on the last Solve's own verdict before the loop ended (OS_SET_STALE): search
// again at the pose the SOLVED set was built at (x_build) -- same queries, same order, same arithmetic: the same rows
int fresh_direct_set(tloam_ctx* c) {
  if (!c->set_stale) return TLOAM_OK;
  BuildParams bp;
  GridView grids[kKinds];
  outer_params(c, &bp, grids);
  HIPC(c, c->state_scratch.reserve(1));
  HIPC(c, hipMemcpyAsync(c->state_scratch.p, c->state.p, sizeof(GnState), hipMemcpyDeviceToDevice, c->stream));
  launch_pose_from_x_build(c->state_scratch.p, c->stream);
  const DirectSet ds{1, 0, 0, nullptr, c->tile_of_slot.p, c->tile_scan.p, c->row_of_pos.p};
  launch_build(c->sv, grids, bp, c->state_scratch.p, c->tile_of_slot.p, c->tile_cnt.p, c->tile_scan.p, c->tile_fill.p, c->qrec.p,
               c->scan_tmp.p, /*rebin=*/false, c->stream, nullptr, nullptr, nullptr, &c->cv, &ds);
  HIPC(c, hipStreamSynchronize(c->stream));
  c->set_stale = false;
  return TLOAM_OK;
}

}  // namespace

extern "C" {

// ---- getFitnessScore (registration.cpp:257-296) -------------------------------------------------
int tloam_fitness(tloam_ctx* c, double* fitness, double* rmse) {
  if (!c || !fitness || !rmse) return TLOAM_E_INVALID;
  *fitness = 0.0;
  *rmse = 0.0;
  if (!(c->cfg.fitness_thres > 0.0)) return TLOAM_OK;  // :258-261 (a NaN threshold finds nobody either)
  if (c->active) return TLOAM_E_NOT_READY;  // between sm_begin and sm_end the context belongs to the solve
  HIPC(c, hipSetDevice(c->device));
  const int blocks = 64;
  HIPC(c, c->misc.reserve(4096));
  const int order[kKinds] = {TLOAM_KIND_EDGE, TLOAM_KIND_SPHERE, TLOAM_KIND_PLANAR, TLOAM_KIND_GROUND};  // :287-290
  double fit_local[kKinds] = {0, 0, 0, 0}, err_local[kKinds] = {0, 0, 0, 0};
  for (int o = 0; o < kKinds; ++o) {
    const int k = order[o];
    KindData& K = c->kd[k];
    // the kd-trees are the ones built by the last scanMatching (:889-915); none yet -> no hits
    if (!K.grid_valid || K.n_src == 0 || !K.src_set || !K.src_ptr) continue;   // (a hand-over that failed registered nothing)
    // raw scan-frame source points (:271): this kind's AoS block as SoA, in scratch of its own (the slot arrays
    // sx/sy/sz belong to scan_match: SlotView holds their addresses)
    HIPC(c, c->fit_x.reserve(K.n_src)); HIPC(c, c->fit_y.reserve(K.n_src)); HIPC(c, c->fit_z.reserve(K.n_src));
    launch_aos_to_soa(K.src_ptr, K.n_src, c->fit_x.p, c->fit_y.p, c->fit_z.p, c->stream);
    launch_fitness(K.gv, c->fit_x.p, c->fit_y.p, c->fit_z.p, (int)K.n_src, c->cfg.fitness_thres, c->misc.p, blocks, c->stream);
    HIPC(c, hipMemcpyAsync(c->h_small, c->misc.p, sizeof(double) * blocks * 2, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < blocks; ++b) { err_local[k] += c->h_small[2 * b]; fit_local[k] += c->h_small[2 * b + 1]; }
  }
  if (c->nranks > 1) {  // sharded sources: hits and squared errors add up across ranks
    HIPC(c, c->misc.reserve(16));
    for (int k = 0; k < kKinds; ++k) { c->h_small[k] = fit_local[k]; c->h_small[4 + k] = err_local[k]; }
    HIPC(c, hipMemcpyAsync(c->misc.p, c->h_small, sizeof(double) * 8, hipMemcpyHostToDevice, c->stream));
    int rc = allreduce(c, c->misc.p, 8);
    if (rc != TLOAM_OK) return rc;
    HIPC(c, hipMemcpyAsync(c->h_small, c->misc.p, sizeof(double) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < kKinds; ++k) { fit_local[k] = c->h_small[k]; err_local[k] = c->h_small[4 + k]; }
  }
  for (int o = 0; o < kKinds; ++o) {
    const int k = order[o];
    if (fit_local[k] > 0.0) {  // :278-284
      *fitness += fit_local[k] / (double)c->kd[k].n_src_full;
      *rmse += sqrt(err_local[k] / fit_local[k]);
    }
  }
  return TLOAM_OK;
}

// ---- introspection --------------------------------------------------------------------------------
// The factors of a kind in source-index order.  A compact set (a frame's, a pre-built one) is its first seg_n[kind] rows as they
// stand; a direct set has a row per source point of the frame the solve began with (not of the cloud registered now): the rows
// that hold a factor (idx >= 0), sorted by source index.
int tloam_get_correspondences(tloam_ctx* c, int kind, size_t capacity, size_t* n, int32_t* src_index, double* a,
                              double* b, double* d, double* w, double* cost) {
  if (!c || kind < 0 || kind >= kKinds || !n) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  const bool direct = c->forms.set == SetForm::DIRECT && !c->prebuilt;
  size_t rows;
  if (direct) {
    const int rc = fresh_direct_set(c);
    if (rc != TLOAM_OK) return rc;
    rows = (size_t)(c->sv.slot_off[kind + 1] - c->sv.slot_off[kind]);
  } else {
    int segn[kKinds];
    HIPC(c, hipMemcpy(segn, c->seg_n.p, sizeof(segn), hipMemcpyDeviceToHost));
    rows = (size_t)segn[kind];
  }
  const CorrSeg& s = c->cv.k[kind];
  std::vector<int> idx(rows);
  if (rows > 0) HIPC(c, hipMemcpy(idx.data(), s.idx, sizeof(int) * rows, hipMemcpyDeviceToHost));
  std::vector<std::pair<int, size_t>> order;   // (source index, row) of the factors
  order.reserve(rows);
  for (size_t r = 0; r < rows; ++r)
    if (!direct || idx[r] >= 0) order.emplace_back(idx[r], r);
  if (direct) std::sort(order.begin(), order.end());
  const size_t m = order.size();
  *n = m;
  if (m > capacity) return TLOAM_E_INVALID;
  if (m == 0) return TLOAM_OK;
  std::vector<double> tmp(rows);
  // the one read path: a column of `rows` doubles read once, gathered through the order into out[i * stride + off]
  auto column = [&](const double* dev, double* out, size_t stride, size_t off) -> int {
    HIPC(c, hipMemcpy(tmp.data(), dev, sizeof(double) * rows, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m; ++i) out[i * stride + off] = tmp[order[i].second];
    return TLOAM_OK;
  };
  int rc = TLOAM_OK;
  if (src_index) for (size_t i = 0; i < m; ++i) src_index[i] = order[i].first;
  if (a && ((rc = column(s.ax, a, 3, 0)) || (rc = column(s.ay, a, 3, 1)) || (rc = column(s.az, a, 3, 2)))) return rc;
  if (b && kind == TLOAM_KIND_EDGE && ((rc = column(s.bx, b, 3, 0)) || (rc = column(s.by, b, 3, 1)) || (rc = column(s.bz, b, 3, 2)))) return rc;
  if (d && kind <= TLOAM_KIND_GROUND && (rc = column(s.d, d, 1, 0))) return rc;
  if (w && (rc = column(s.w, w, 1, 0))) return rc;
  if (cost && (rc = column(s.cost, cost, 1, 0))) return rc;
  return TLOAM_OK;
}

int tloam_get_weights(tloam_ctx* c, int kind, size_t capacity, size_t* n, double* w) {
  if (!c || kind < 0 || kind >= kKinds || !n) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  // the weights are those of the frame the last scanMatching BEGAN with (its slot table), whatever source cloud has been handed over
  // since (until round 6 the size came from the registered cloud: a larger cloud handed over after a solve made this a copy past
  // the end of the weights -- tests/tools/fuzz_call_order.py, TLOAM_E_HIP from a getter)
  const bool begun = c->w_src.p != nullptr && c->sv.slot_off[kKinds] > 0;
  const size_t m = begun ? (size_t)(c->sv.slot_off[kind + 1] - c->sv.slot_off[kind]) : c->kd[kind].n_src;
  *n = m;
  if (m > capacity || !begun) return TLOAM_E_INVALID;
  HIPC(c, hipStreamSynchronize(c->stream));
  if (c->forms.set == SetForm::DIRECT && !c->prebuilt) {   // the current GNC weights live in the rows' weight stream `w_parity`: back to source-index order
    if (w && m > 0 && !c->have_build) {   // (no search has run in this frame yet: registration.cpp:931-949, every weight is 1)
      for (size_t i = 0; i < m; ++i) w[i] = 1.0;
    } else if (w && m > 0) {
      std::vector<int> idx(m);
      std::vector<double> wr(m);
      HIPC(c, hipMemcpy(idx.data(), c->cv.k[kind].idx, sizeof(int) * m, hipMemcpyDeviceToHost));
      HIPC(c, hipMemcpy(wr.data(), direct_w_stream(c, kind, c->w_parity), sizeof(double) * m, hipMemcpyDeviceToHost));
      for (size_t r = 0; r < m; ++r) w[(size_t)(idx[r] >= 0 ? idx[r] : ~idx[r]) - (size_t)c->sv.src_lo[kind]] = wr[r];
    }
    return TLOAM_OK;
  }
  if (w && m > 0) HIPC(c, hipMemcpy(w, c->w_src.p + c->sv.slot_off[kind], sizeof(double) * m, hipMemcpyDeviceToHost));
  return TLOAM_OK;
}

int tloam_knn(tloam_ctx* c, int kind, const double* q, size_t nq, double radius, int k, int32_t* out_idx,
              double* out_d2, int32_t* out_cnt) {
  if (!c || kind < 0 || kind >= kKinds || !q || k < 1 || k > kMaxK || !(radius > 0.0) || !out_idx || !out_d2 || !out_cnt ||
      nq > kMaxPoints / (size_t)k)
    return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  KindData& K = c->kd[kind];
  if (!K.tgt_set || K.n_tgt == 0) {
    for (size_t i = 0; i < nq; ++i) out_cnt[i] = 0;
    for (size_t i = 0; i < nq * (size_t)k; ++i) { out_idx[i] = -1; out_d2[i] = 0.0; }
    return TLOAM_OK;
  }
  int rc;
  GridBuffers& tmp = c->grids_knn;  // a grid over the target currently set, sized for this radius; the scanMatching grids stay intact
  GridView views[kKinds];
  {
    double radii[kKinds] = {0, 0, 0, 0};
    radii[kind] = radius;
    rc = build_grids(c, tmp, radii, views);
    if (rc != TLOAM_OK) return rc;
  }
  DBuf<double> qa, qx, qy, qz, d2;
  DBuf<int> idx, cnt;
  hipError_t e = hipSuccess;
  if ((e = qa.reserve(3 * nq + 3)) != hipSuccess || (e = qx.reserve(nq + 1)) != hipSuccess ||
      (e = qy.reserve(nq + 1)) != hipSuccess || (e = qz.reserve(nq + 1)) != hipSuccess ||
      (e = d2.reserve(nq * k + 1)) != hipSuccess || (e = idx.reserve(nq * k + 1)) != hipSuccess ||
      (e = cnt.reserve(nq + 1)) != hipSuccess) {
    c->last_error = hipGetErrorString(e);
    return TLOAM_E_HIP;
  }
  if (nq > 0) {
    (void)hipMemcpyAsync(qa.p, q, sizeof(double) * 3 * nq, hipMemcpyHostToDevice, c->stream);
    launch_aos_to_soa(qa.p, nq, qx.p, qy.p, qz.p, c->stream);
    launch_knn(views[kind], qx.p, qy.p, qz.p, (int)nq, radius, k, idx.p, d2.p, cnt.p, c->stream);
    (void)hipMemcpyAsync(out_idx, idx.p, sizeof(int) * nq * k, hipMemcpyDeviceToHost, c->stream);
    (void)hipMemcpyAsync(out_d2, d2.p, sizeof(double) * nq * k, hipMemcpyDeviceToHost, c->stream);
    (void)hipMemcpyAsync(out_cnt, cnt.p, sizeof(int) * nq, hipMemcpyDeviceToHost, c->stream);
  }
  e = hipStreamSynchronize(c->stream);   // (before the locals go)
  if (e != hipSuccess) { c->last_error = hipGetErrorString(e); return TLOAM_E_HIP; }
  return check_device_faults(c);
}

// ---- pre-built correspondence sets ------------------------------------------------------------------
int tloam_set_correspondences(tloam_ctx* c, int res_type, size_t n, const double* p, const double* a, const double* b,
                              const double* d, const double* w) {
  if (!c || res_type < 0 || res_type >= TLOAM_NUM_RES || n > kMaxPoints) return TLOAM_E_INVALID;
  if (n > 0 && (!p || !a || !w || (res_type == TLOAM_RES_LINE && !b) || (res_type == TLOAM_RES_PLANE && !d)))
    return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  int rc = ensure_common(c);
  if (rc != TLOAM_OK) return rc;
  const int kind = res_kind(res_type);
  if (!c->prebuilt) {
    HIPC(c, hipMemsetAsync(c->seg_n.p, 0, 8 * sizeof(int), c->stream));
    for (int k = 0; k < kKinds; ++k) {
      rc = reserve_seg(c, k, 1);
      if (rc != TLOAM_OK) return rc;
      c->kd[k].pre_n_full = 0;
    }
    c->prebuilt = true;
    c->active = false;
  }
  size_t lo = 0, hi = n;
  tloam_shard_range(n, c->rank, c->nranks, &lo, &hi);
  const size_t m = hi - lo;
  KindData& K = c->kd[kind];
  K.pre_lo = lo;
  K.pre_n_full = n;
  rc = reserve_seg(c, kind, m);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, c->misc.reserve(3 * std::max<size_t>(m, 1)));
  const CorrSeg& s = c->cv.k[kind];
  if (m > 0) {
    HIPC(c, hipMemcpyAsync(c->misc.p, p + 3 * lo, sizeof(double) * 3 * m, hipMemcpyHostToDevice, c->stream));
    launch_aos_to_soa(c->misc.p, m, s.px, s.py, s.pz, c->stream);
    HIPC(c, hipMemcpyAsync(c->misc.p, a + 3 * lo, sizeof(double) * 3 * m, hipMemcpyHostToDevice, c->stream));
    launch_aos_to_soa(c->misc.p, m, s.ax, s.ay, s.az, c->stream);
    if (res_type == TLOAM_RES_LINE) {
      HIPC(c, hipMemcpyAsync(c->misc.p, b + 3 * lo, sizeof(double) * 3 * m, hipMemcpyHostToDevice, c->stream));
      launch_aos_to_soa(c->misc.p, m, s.bx, s.by, s.bz, c->stream);
    }
    if (res_type == TLOAM_RES_PLANE) HIPC(c, hipMemcpyAsync(s.d, d + lo, sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemcpyAsync(s.w, w + lo, sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipMemsetAsync(s.cost, 0, sizeof(double) * m, c->stream));
    std::vector<int> ids(m);
    for (size_t i = 0; i < m; ++i) ids[i] = (int)(lo + i);
    HIPC(c, hipMemcpyAsync(s.idx, ids.data(), sizeof(int) * m, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
  }
  const int mi = (int)m;
  HIPC(c, hipMemcpyAsync(c->seg_n.p + kind, &mi, sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  // algorithmic bytes of one sweep over the whole (job-wide) pre-built set
  const int full[kKinds] = {(int)c->kd[0].pre_n_full, 0, (int)c->kd[2].pre_n_full, (int)c->kd[3].pre_n_full};
  c->k3_alg_bytes = alg_bytes_of(full);
  plan_sweeps(c);
  {
    FormsIn in = forms_in(c);   // (a pre-built set has no source slots, whatever clouds are registered: it is compact)
    for (int k = 0; k < kKinds; ++k) in.n_src[k] = in.n_tgt[k] = 0;
    c->forms = decide_forms(in);
  }
  return reserve_partials(c);
}

int tloam_accumulate(tloam_ctx* c, const double se3[6], double H[36], double g[6], double* cost) {
  if (!c || !se3) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (!c->partials.p) return TLOAM_E_NOT_READY;
  int rc = eval_at(c, se3);
  if (rc != TLOAM_OK) return rc;
  rc = launch_k3_timed(c, true);
  if (rc != TLOAM_OK) return rc;
  launch_reduce(c->partials.p, c->k3_grid, c->state.p, c->red48.p, c->stream);
  rc = allreduce(c, c->red48.p, kReduceBuf);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, hipMemcpyAsync(c->h_small + 8, c->red48.p, sizeof(double) * kReduceBuf, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  rc = harvest_k3_events(c, 1);
  if (rc != TLOAM_OK) return rc;
  const double* t = c->h_small + 8;
  if (H) {
    int u = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) { H[i * 6 + j] = t[u]; H[j * 6 + i] = t[u]; ++u; }
  }
  if (g) for (int i = 0; i < 6; ++i) g[i] = t[21 + i];
  if (cost) *cost = t[27];
  return TLOAM_OK;
}

int tloam_get_normal_equations(tloam_ctx* c, double H[36], double g[6], double* cost) {
  if (!c) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  // (a copy of its own, not the frame's pinned mirror h_state: the stepwise API calls this between two tloam_sm_outer)
  const std::unique_ptr<GnState> S(new (std::nothrow) GnState);
  if (!S) return TLOAM_E_INVALID;
  HIPC(c, hipMemcpy(S.get(), c->state.p, sizeof(GnState), hipMemcpyDeviceToHost));
  if (H) memcpy(H, S->H, sizeof(double) * 36);
  if (g) memcpy(g, S->g, sizeof(double) * 6);
  if (cost) *cost = S->x_cost;
  return TLOAM_OK;
}

int tloam_get_costs(tloam_ctx* c, int res_type, size_t capacity, size_t* n, double* cost) {
  if (!c || res_type < 0 || res_type >= TLOAM_NUM_RES || !n) return TLOAM_E_INVALID;
  return tloam_get_correspondences(c, res_kind(res_type), capacity, n, nullptr, nullptr, nullptr, nullptr, nullptr, cost);
}

int tloam_solve(tloam_ctx* c, double se3[6], tloam_stats* stats) {
  if (!c || !se3) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (!c->partials.p) return TLOAM_E_NOT_READY;
  HIPC(c, hipMemsetAsync(c->state.p, 0, sizeof(GnState), c->stream));
  memcpy(c->h_small, se3, sizeof(double) * 6);
  HIPC(c, hipMemcpyAsync(c->state.p, c->h_small, sizeof(double) * 6, hipMemcpyHostToDevice, c->stream));
  if (c->dbg_no_eval_reuse) {
    static const int one = 1;
    HIPC(c, hipMemcpyAsync(&c->state.p->no_eval_reuse, &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  int rc = enqueue_solve(c, /*armed=*/false, c->dbg_max_sweeps > 0 ? c->dbg_max_sweeps : kSolveSweeps);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, hipMemcpyAsync(c->h_state, c->state.p, sizeof(GnState), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  const GnState& S = *c->h_state;
  rc = harvest_k3_events(c, S.gn_sweeps);
  if (rc != TLOAM_OK) return rc;
  memcpy(se3, S.x, sizeof(double) * 6);
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->gn_evaluations = S.gn_evaluations;
    stats->gn_sweeps = S.gn_sweeps;
    stats->gn_iterations = S.gn_iterations;
    stats->accepted_steps = S.accepted_steps;
    stats->solver_cost = S.x_cost;
    memcpy(stats->se3, S.x, sizeof(double) * 6);
  }
  return TLOAM_OK;
}

int tloam_time_accumulate(tloam_ctx* c, const double se3[6], int launches, double* mean_us) {
  if (!c || !se3 || launches < 1 || !mean_us) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (!c->partials.p) return TLOAM_E_NOT_READY;
  const int rc = eval_at(c, se3);
  if (rc != TLOAM_OK) return rc;
  return timed_launches(c, launches, [&](int) -> int {
    launch_k3(c->cv, c->state.p, c->partials.p, c->k3_grid, c->k3_single, c->k3_wide, true, c->stream);
    return TLOAM_OK;
  }, mean_us);
}

// Sharded contexts (collective call: every rank, same arguments): `launches` sweeps of this rank's block of the
// current set at se3, each followed (with_exchange != 0) by the exchange of the 48 doubles exactly as a GN iteration
// does it -- mailbox: posted by the sweep's last block, gathered by a one-wave kernel; RCCL / callback: all-reduce of
// the folded buffer -- bracketed by one HIP event pair.  with_exchange == 0: the sweeps alone (the last block
// still folds the rows).  The difference of the two is the latency the exchange adds to a GN iteration.
int tloam_time_sharded_sweep(tloam_ctx* c, const double se3[6], int launches, int with_exchange, double* mean_us) {
  if (!c || !se3 || launches < 1 || !mean_us) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (!c->partials.p) return TLOAM_E_NOT_READY;
  int rc = eval_at(c, se3);
  if (rc != TLOAM_OK) return rc;
  K3Fuse fuse;
  memset(&fuse, 0, sizeof(fuse));
  fuse.ticket = c->k3_ticket.p;
  fuse.out48 = c->red48.p;
  const bool mbox = with_exchange && c->comm == COMM_MAILBOX && exchanging(c);
  if (mbox) fuse.mb = c->mbox;
  return timed_launches(c, launches, [&](int) -> int {
    launch_k3_fused(c->cv, c->state.p, c->partials.p, c->k3_grid, c->k3_single, c->k3_wide, true, fuse, c->stream);
    if (mbox) launch_mbox_gather_only(c->red48.p, c->mbox, c->stream);
    else if (with_exchange) return allreduce(c, c->red48.p, kReduceBuf);
    return TLOAM_OK;
  }, mean_us);
}

// Timing helper for the bench (roofline_k1): `launches` back-to-back runs of the correspondence-search kernel
// (K1 + K2: SearchHybrid + the four builders) over the source slots of the last scan_match -- same pose, same grids,
// same query order; the kernel only rewrites the raw records and flags it wrote before -- bracketed by one HIP event
// pair.  *queries = source points searched per launch.
int tloam_time_build(tloam_ctx* c, int launches, double* mean_us, int64_t* queries) {
  if (!c || launches < 1 || !mean_us) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  if (c->active || !c->have_build || !c->qrec.p) return TLOAM_E_NOT_READY;
  BuildParams bp;
  GridView grids[kKinds];
  outer_params(c, &bp, grids);
  const int rc = timed_launches(c, launches, [&](int) -> int {
    launch_build(c->sv, grids, bp, c->state.p, c->tile_of_slot.p, c->tile_cnt.p, c->tile_scan.p, c->tile_fill.p, c->qrec.p,
                 c->scan_tmp.p, /*rebin=*/false, c->stream, nullptr);
    return TLOAM_OK;
  }, mean_us);
  if (rc != TLOAM_OK) return rc;
  if (queries) *queries = (int64_t)c->sv.slot_off[kKinds];
  return TLOAM_OK;
}

int tloam_k3_timer(tloam_ctx* c, int reset, double* total_us, int64_t* launches, double* algorithmic_bytes) {
  if (!c) return TLOAM_E_INVALID;
  if (total_us) *total_us = c->k3_total_us;
  if (launches) *launches = c->k3_launches;
  if (algorithmic_bytes) *algorithmic_bytes = c->k3_alg_bytes;
  if (reset) {
    c->k3_total_us = c->k3_all_us = 0.0;
    c->k3_launches = c->k3_all_launches = 0;
  }
  c->k3_timing = true;  // first call arms the per-launch event pairs
  return TLOAM_OK;
}

// test aid: the device SE(3) arithmetic of the minimiser step (k_debug_se3), n items of (x, delta) -> 26 doubles each
int tloam_debug_se3(tloam_ctx* c, int n, const double* x, const double* delta, double* out26) {
  if (!c || n < 1 || !x || !delta || !out26) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, c->misc.reserve((size_t)n * 38 + 8));
  double* dx = c->misc.p; double* dd = dx + 6 * (size_t)n; double* dout = dd + 6 * (size_t)n;
  HIPC(c, hipMemcpyAsync(dx, x, sizeof(double) * 6 * n, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemcpyAsync(dd, delta, sizeof(double) * 6 * n, hipMemcpyHostToDevice, c->stream));
  launch_debug_se3(dx, dd, n, dout, c->stream);
  HIPC(c, hipMemcpyAsync(out26, dout, sizeof(double) * 26 * n, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

// debugging aid: raw copy of the device-resident minimiser state (layout: tl_common.hpp GnState)
int tloam_debug_state(tloam_ctx* c, double* out, int n_doubles) {
  if (!c || !out) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  const size_t bytes = std::min(sizeof(GnState), sizeof(double) * (size_t)n_doubles);
  HIPC(c, hipMemcpy(out, c->state.p, bytes, hipMemcpyDeviceToHost));
  return (int)(sizeof(GnState) / sizeof(double));
}

int tloam_debug_partials(tloam_ctx* c, double* out, int n_doubles) {
  if (!c || !out) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  const size_t n = std::min(c->partials.cap, (size_t)std::max(n_doubles, 0));   // (rows, then whatever a profiling build put behind them)
  HIPC(c, hipMemcpy(out, c->partials.p, n * sizeof(double), hipMemcpyDeviceToHost));
  return c->k3_grid;
}

// every K3 launch since the last reset, no-op launches (after a tolerance exit) included: the population
// `rocprofv3 --kernel-trace --stats` averages over
int tloam_k3_timer_all(tloam_ctx* c, double* total_us, int64_t* launches) {
  if (!c) return TLOAM_E_INVALID;
  if (total_us) *total_us = c->k3_all_us;
  if (launches) *launches = c->k3_all_launches;
  return TLOAM_OK;
}

// The period of a GN iteration as the DEVICE clocks it (iter_span_note, tl_gn.hip): between the ends of two consecutive
// minimiser steps of one Solve -- sweep, launch boundaries, fold, exchange, step.  The first call arms it.
int tloam_gn_iter_timer(tloam_ctx* c, int reset, double* total_us, int64_t* iterations) {
  if (!c) return TLOAM_E_INVALID;
  const int rc = read_span(c, c->iter_span, reset, total_us, iterations);
  if (rc != TLOAM_OK) return rc;
  c->iter_timing = true;
  return TLOAM_OK;
}

// the streaming part of the one-launch GN iterations as their kernel clocks it (K3Step::span); always counted, nothing to arm
int tloam_k3_span(tloam_ctx* c, int reset, double* total_us, int64_t* launches) {
  if (!c) return TLOAM_E_INVALID;
  return read_span(c, c->k3_span, reset, total_us, launches);
}

}  // extern "C"
