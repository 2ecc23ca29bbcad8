// tl_api_match.hip -- the host driver of LocalRegistration::scanMatching (registration.cpp:879-1133) behind the C ABI
// (include/tloam_hip.h): the frame, stepwise (tloam_sm_begin / tloam_sm_outer / tloam_sm_end) and with the outer GNC loop driven
// from the device (tloam_scan_match).  What a host does to the factor set outside a frame is tl_api_sets.hip, which shares the
// helpers declared under this unit's name in tl_ctx.hpp.
//
// Host side mirrors the reference's control flow (outer GNC loop, mu schedule, plateau test);
// every per-point / per-correspondence computation is a HIP kernel (tl_nn.hip, tl_gn.hip).
// Helpers first, in namespaces; the four entry points, the only extern "C" of the unit, last.
#include <atomic>

#include "tl_ctx.hpp"

using namespace tl;

namespace tlh {
int reserve_seg(tloam_ctx* c, int k, size_t n) {
  KindData& K = c->kd[k];
  const size_t cap = round_up(std::max<size_t>(n, 1), kChunk) + kChunk;  // + one chunk: double2 tail reads
  HIPC(c, K.c_idx.reserve(cap));
  if (cap > K.c_stride) {  // (grow-only, like every DBuf; the contents are rewritten by the caller)
    const size_t stride = std::max(cap, K.c_stride + K.c_stride / 2);
    HIPC(c, K.c_buf.reserve(stride * kSegStreams));
    K.c_stride = stride;
  }
  K.c_cap = cap - kChunk;
  CorrSeg& s = c->cv.k[k];
  double* b = K.c_buf.p;
  const size_t st = K.c_stride;
  s.idx = K.c_idx.p;
  s.px = b + SS_PX * st; s.py = b + SS_PY * st; s.pz = b + SS_PZ * st;
  s.ax = b + SS_AX * st; s.ay = b + SS_AY * st; s.az = b + SS_AZ * st;
  s.bx = (k == TLOAM_KIND_EDGE) ? b + SS_BX * st : nullptr;
  s.by = (k == TLOAM_KIND_EDGE) ? b + SS_BY * st : nullptr;
  s.bz = (k == TLOAM_KIND_EDGE) ? b + SS_BZ * st : nullptr;
  s.d = (k <= TLOAM_KIND_GROUND) ? b + SS_D * st : nullptr;
  s.w = b + SS_W * st;
  s.cost = b + SS_COST * st;
  s.cap = (int)K.c_cap;
  s.stride = (int)st;
  return TLOAM_OK;
}
int ensure_common(tloam_ctx* c) {
  HIPC(c, c->state.reserve(1));
  HIPC(c, c->seg_n.reserve(8));
  HIPC(c, c->red48.reserve(kReduceBuf));
  HIPC(c, c->sums16.reserve(16));
  HIPC(c, c->wpart.reserve(256 * 8));
  HIPC(c, c->rank_counts.reserve((size_t)kMaxRanks * kKinds));
  HIPC(c, c->se3_dev.reserve(8));
  if (!c->k3_ticket.p) {
    HIPC(c, c->k3_ticket.reserve(4));
    HIPC(c, hipMemsetAsync(c->k3_ticket.p, 0, 4 * sizeof(int), c->stream));
    {
      // The launch counter of the tagged hand-overs (words 2..3 of the ticket buffer; tl_gn.hip k3_post_row_tagged) starts from a
      // number no other context of this process uses: a context's row buffer can be memory that a context destroyed a moment ago
      // wrote ITS rows into, with valid check words for ITS launch numbers -- which would be this context's first launch numbers
      // too if both counted from zero.  A stepper that looked before the fresh row landed then folded the dead context's sums,
      // the blocks' images of the minimiser disagreed and the launch ran into its bounded wait (round 5: seen as a one-in-two
      // TLOAM_E_HIP in the GPU suite when contexts solving DIFFERENT scenes followed each other through the stepwise API).
      static std::atomic<unsigned long long> serial{0};
      const unsigned long long base = (serial.fetch_add(1ull, std::memory_order_relaxed) + 1ull) << 36;   // 2^36 launches per context
      HIPC(c, hipMemcpyAsync(reinterpret_cast<unsigned long long*>(c->k3_ticket.p + 2), &base, sizeof(base), hipMemcpyHostToDevice, c->stream));
      HIPC(c, hipStreamSynchronize(c->stream));   // (`base` is a local)
    }
    HIPC(c, c->k3_span.reserve(4));     // K3Step::span
    HIPC(c, hipMemsetAsync(c->k3_span.p, 0, 4 * sizeof(unsigned long long), c->stream));
    HIPC(c, c->iter_span.reserve(4));   // iter_span_note
    HIPC(c, hipMemsetAsync(c->iter_span.p, 0, 4 * sizeof(unsigned long long), c->stream));
  }
  c->cv.seg_n = c->seg_n.p;
  return TLOAM_OK;
}
// The query-tile histogram and its scan, ntiles + 1 entries each.  The tile count follows the bounding boxes like the cell tables:
// a table that has to grow does so with room to spare.  The one size rule of the frame's start (the grid build's first launch, or
// k_frame_init), which zeroes the histogram, and of the query sort, which counts into it: whoever comes first sizes both tables,
// so nothing is re-allocated -- and lost -- in between.
// frame_start: the caller's launch zeroes the entries itself.  Anybody else finds the start already enqueued: a histogram that has
// to be (re)allocated then is zeroed here.  (Until round 5 it was not, and the sizes asked for at the two places differed by the
// one element that crosses an allocation step: the counting sort then ranked the queries on what the new block happened to hold
// and scattered them out of bounds -- a GPU memory fault or a silently wrong query order on the first large frame of a context,
// whenever the block was not fresh; found by tests/tools/fuzz_call_order.py.)
int reserve_tile_hist(tloam_ctx* c, size_t ntiles, bool frame_start, size_t* room) {
  const size_t n = grown(ntiles, ntiles + 1 > c->tile_cnt.cap || ntiles + 1 > c->tile_scan.cap);
  if (frame_start) HIPC(c, c->tile_cnt.reserve(n + 1));
  else HIPC(c, c->tile_cnt.reserve_zeroed(n + 1, c->stream));
  HIPC(c, c->tile_scan.reserve(n + 1));
  if (room) *room = n;   // (the tiles asked for: what the sort's other tables follow)
  return TLOAM_OK;
}
// (also called from the grid build when the sort's first pass rides on it: the SAME sizes, so that nothing is re-allocated -- and
//  lost -- between that pass and the rest of the sort)
int reserve_query_sort(tloam_ctx* c, const GridView grids[kKinds]) {
  const size_t n_slots = (size_t)c->sv.slot_off[kKinds];
  const size_t ntiles = (size_t)build_tile_count(grids, c->sv.slot_off);
  size_t nt_res = 0;
  const int rc = reserve_tile_hist(c, ntiles, /*frame_start=*/false, &nt_res);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, c->tile_fill.reserve(std::max<size_t>((size_t)nt_res, (size_t)n_slots + 1))  /* rank of every slot inside its tile */); HIPC(c, c->tile_of_slot.reserve(n_slots + 1));
  HIPC(c, c->qrec.reserve(n_slots + 1));
  HIPC(c, c->scan_tmp.reserve(scan_scratch_elems(std::max(nt_res + 1, n_slots + 1))));
  c->scan1p_q_use = scan_path(ntiles + 1, c->device_cus, !c->no_scan_1p).path == ScanPath::SINGLE_PASS;
  // (the control words of the single-pass scan read zero between launches: only a (re)allocation has to be cleared)
  if (c->scan1p_q_use) HIPC(c, c->scan1p_q.reserve_zeroed(scan_ctl_elems(nt_res + 1), c->stream));
  return TLOAM_OK;
}
BuildParams build_params(const tloam_ctx* c) {
  BuildParams bp;
  for (int k = 0; k < kKinds; ++k) {
    bp.radius[k] = kind_radius(c->cfg, k);
    bp.maxnum[k] = kind_maxnum(c->cfg, k);
    bp.active[k] = kind_active(c->cfg, k);
  }
  bp.edge_dir_thres = c->cfg.edge_dir_thres;
  return bp;
}
void outer_params(const tloam_ctx* c, BuildParams* bp, GridView grids[kKinds]) {
  *bp = build_params(c);
  for (int k = 0; k < kKinds; ++k) grids[k] = c->kd[k].gv;
}
// the sweep's launch form (grid, one-wave-per-chunk, wide) from the segments' capacities
void plan_sweeps(tloam_ctx* c) {
  int caps[kKinds];
  for (int k = 0; k < kKinds; ++k) caps[k] = (int)c->kd[k].c_cap;
  k3_plan(caps, c->device_cus, &c->k3_grid, &c->k3_single, &c->k3_wide);
}
// the only reader of the knobs that select forms
FormsIn forms_in(const tloam_ctx* c) {
  FormsIn in;
  in.nranks = c->nranks;
  in.loopback = c->loopback ? 1 : 0;
  in.mailbox = c->comm == COMM_MAILBOX ? 1 : 0;
  in.device_cus = c->device_cus;
  in.no_persistent_solve = c->no_persistent_solve ? 1 : 0;
  in.no_direct_set = c->no_direct_set ? 1 : 0;
  in.no_device_loop = c->no_device_loop ? 1 : 0;
  in.no_build_reuse = c->dbg_no_build_reuse ? 1 : 0;
  in.fused_large = c->fused_large ? 1 : 0;
  in.no_qbin_ride = c->no_qbin_ride ? 1 : 0;
  in.factor_num = c->cfg.factor_num;
  in.max_iterations = c->cfg.max_iterations;
  for (int k = 0; k < kKinds; ++k) {
    in.maxnum[k] = kind_maxnum(c->cfg, k);
    in.n_src[k] = (long long)c->kd[k].n_src;
    in.n_tgt[k] = (long long)c->kd[k].n_tgt;
    in.seg_cap[k] = (long long)c->kd[k].c_cap;
  }
  in.k3_grid = c->k3_grid;
  in.k3_single = c->k3_single ? 1 : 0;
  return in;
}
double* direct_w_stream(const tloam_ctx* c, int k, int parity) {
  return c->kd[k].c_buf.p + (size_t)(parity ? SS_W2 : SS_W) * c->kd[k].c_stride;
}
// the per-block rows of the sweeps (and, below 4096 words, the tagged rows / finish segments of the one-launch Solve): cleared
// when (re)allocated, so that nothing in them ever carries a valid check word that this context did not write
int reserve_partials(tloam_ctx* c) {
  HIPC(c, c->partials.reserve_zeroed(std::max<size_t>((size_t)c->k3_grid * kAccStride, 4096), c->stream));
  return TLOAM_OK;
}
double alg_bytes_of(const int n[kKinds]) {
  // plane 72 B, line 88 B, point 64 B per correspondence (fp64 SoA, cost write included)
  return 72.0 * ((double)n[TLOAM_KIND_PLANAR] + (double)n[TLOAM_KIND_GROUND]) + 88.0 * (double)n[TLOAM_KIND_EDGE] +
         64.0 * (double)n[TLOAM_KIND_SPHERE];
}
}  // namespace tlh

namespace {

// ---- the direct factor set (tl_common.hpp DirectSet; which frames take it: decide_forms) ------------------------------------
bool direct(const tloam_ctx* c) { return c->forms.set == SetForm::DIRECT; }
// the Solve of outer iteration `iter` reads weight stream iter & 1 (c->cv), its finish writes the other one
void direct_set_parity(tloam_ctx* c, int iter) {
  for (int k = 0; k < kKinds; ++k) c->cv.k[k].w = direct_w_stream(c, k, iter & 1);
}
// rows of the hand-over buffer of the finish, compact (riding) or direct
constexpr size_t kFinRowsDoubles = (size_t)(4 * 256 + 64) * 16;   // the blocks' rows + the rows of their groups of 64
size_t seg_cap_sum(const tloam_ctx* c) {   // the four segments' capacity: what sizes the finish (finish_wblocks)
  size_t cap = 0;
  for (int k = 0; k < kKinds; ++k) cap += c->kd[k].c_cap;
  return cap;
}
// (a quarter of the) one-wave blocks of a direct finish: a fixed function of the capacity, so that the riding form and the launch of
// its own cut the rows alike.  (Twice as many blocks on ONE ticket measured 52 instead of 31 us for the frame's last finish: the
// arrivals on the ticket are what it waits for -- hence the two-level hand-over of finish_direct_block.)
// (The same function gives the block count of every finish -- enqueue_finish, the riding large finish: the summation tree,
// hence the bits, must not depend on the path or on timing.)
int finish_wblocks(const tloam_ctx* c) { return (int)std::min<size_t>(256, std::max<size_t>(64, seg_cap_sum(c) / 2048)); }
int* direct_blk_cnt(const tloam_ctx* c, int iter) { return c->blk_cnt.p + (size_t)(iter & 1) * c->blk_cnt_n * kKinds; }
// built: 1 the set of outer iteration `iter` was built in it, 0 it is the previous one, -1 the device knows (GnState::run_build)
FinishLargeArgs direct_finish_args(tloam_ctx* c, const CorrView* cv_iter, const WeightParams* wp, const HostMirror& hm, OuterCtl ctl,
                                   int iter, int riding, int built) {
  ctl.direct = riding ? 2 : 1;
  FinishLargeArgs fin{cv_iter, wp, c->seg_n.p, c->sums16.p, hm, ctl, c->fin_rows.p, c->fin_tickets.p, finish_wblocks(c), {}, nullptr, 0, 0};
  for (int k = 0; k < kKinds; ++k) fin.w_next[k] = direct_w_stream(c, k, (iter + 1) & 1);
  fin.blk_cnt = direct_blk_cnt(c, iter);
  fin.nblk = (int)c->blk_cnt_n;
  fin.built = built;
  return fin;
}

// K3 launch; when the bench armed the timer, with a HIP event pair bound to the dispatch itself
// Every kK3SampleStride-th launch carries the pair (stride 3 is coprime to the 5 sweeps of a Solve and the 20 of
// a frame, so over a few frames every position is sampled equally): timing EVERY launch through
// hipExtLaunchKernelGGL cost ~8 % of the 1 M frame.
constexpr int kK3SampleStride = 3;
// the device-side period counter of the GN iterations, once tloam_gn_iter_timer has armed it (null otherwise: the kernels skip it)
unsigned long long* iter_span_of(const tloam_ctx* c) { return c->iter_timing ? c->iter_span.p : nullptr; }
// one sweep launch of the batch: launch(ev_start, ev_stop) with a pair from the event pool on every kK3SampleStride-th launch
// (when the timer is armed), with two null events otherwise
template <class Launch>
int launch_sampled(tloam_ctx* c, Launch launch) {
  const bool sample = c->k3_timing && (c->k3_seq++ % kK3SampleStride) == 0;
  const int idx = c->batch_launches++;
  if (!sample) {
    launch(nullptr, nullptr);
    return TLOAM_OK;
  }
  if (c->ev_used + 2 > c->ev_pool.size()) {
    const size_t old = c->ev_pool.size();
    c->ev_pool.resize(old + 256);
    for (size_t i = old; i < c->ev_pool.size(); ++i) HIPC(c, hipEventCreate(&c->ev_pool[i]));
  }
  launch(c->ev_pool[c->ev_used], c->ev_pool[c->ev_used + 1]);
  c->ev_used += 2;
  c->ev_batch_idx.push_back(idx);
  return TLOAM_OK;
}
// the one-launch GN iteration (k3_sweep_step) so sampled: the pair then brackets sweep + fold + step; the streaming part
// alone is what the kernel's own span counter measures (K3Step::span, read by tloam_k3_timer_span)
int launch_k3_step_timed(tloam_ctx* c) {
  const MboxView* mb = (exchanging(c) && c->comm == COMM_MAILBOX) ? &c->mbox : nullptr;
  return launch_sampled(c, [&](hipEvent_t e0, hipEvent_t e1) {
    launch_k3_step(c->cv, c->state.p, c->partials.p, c->k3_grid, c->k3_single, c->k3_wide, c->k3_ticket.p, c->k3_span.p, mb, c->stream, e0,
                   e1, iter_span_of(c));
  });
}
// fold the recorded event pairs into the accumulated timers (stream must be idle).  The launches of the batch belong
// to `nsolve` Solves starting at batch positions start[i]; of each, the first working[i] launches did a sweep, the
// later ones were no-op launches after `done`.
int harvest_k3_events_multi(tloam_ctx* c, int nsolve, const int* start, const int* working) {
  c->batch_launches = 0;
  if (!c->k3_timing) { c->ev_used = 0; c->ev_batch_idx.clear(); return TLOAM_OK; }
  const size_t pairs = c->ev_used / 2;
  for (size_t i = 0; i < pairs; ++i) {
    float ms = 0.f;
    HIPC(c, hipEventElapsedTime(&ms, c->ev_pool[2 * i], c->ev_pool[2 * i + 1]));
    c->k3_all_us += (double)ms * 1e3;
    c->k3_all_launches += 1;
    const int b = c->ev_batch_idx[i];
    int sv = 0;
    while (sv + 1 < nsolve && start[sv + 1] <= b) ++sv;
    if (b - start[sv] < working[sv]) {
      c->k3_total_us += (double)ms * 1e3;
      c->k3_launches += 1;
    }
  }
  c->ev_used = 0;
  c->ev_batch_idx.clear();
  return TLOAM_OK;
}

// Result of an outer iteration on the host.  With the mirror the finish kernel has been handed
// {pinned state, sequence number}: poll the number (a word in host memory the device writes last); the stream
// is only queried now and then, to notice a failed launch instead of spinning forever.  Otherwise, or if the
// stream drained without the number arriving, copy the state and synchronise.
HostMirror next_mirror(tloam_ctx* c, int slot = 0) {
  HostMirror hm;
  hm.out = c->h_mirror.dev + slot;
  hm.seq = ++c->mirror_seq;
  return hm;
}
int wait_state(tloam_ctx* c, const HostMirror& hm, int slot = 0) {
  struct Acc {
    tloam_ctx* c;
    double t0;
    ~Acc() { c->wait_us += host_now_us() - t0; }
  } acc{c, host_now_us()};
  if (hm.out) {
    // all three segments of the slot (MirrorSlot), each verified against the number, then the prefix out of them
    const MirrorSlot* ms = c->h_mirror + slot;
    int rc = TLOAM_OK;
    unsigned long long pay[3][7];
    for (int sgm = 0; sgm < 3 && rc == TLOAM_OK; ++sgm) rc = wait_segment(c, &ms->w[sgm * 8], hm.seq, pay[sgm]);
    if (rc < 0) return rc;
    if (rc == TLOAM_OK) {
      unsigned long long* dst = reinterpret_cast<unsigned long long*>(c->h_state + slot);
      for (int w = 0; w < kMirrorWords; ++w) dst[w] = pay[w / 7][w % 7];
      c->h_state[slot].host_seq = hm.seq;
      return TLOAM_OK;
    }
  }
  HIPC(c, hipMemcpyAsync(c->h_state + slot, c->state.p, sizeof(GnState), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}
}  // namespace

namespace tlh {
// the streaming sweep (launch_k3) as a sampled launch of the batch
int launch_k3_timed(tloam_ctx* c, bool force) {
  return launch_sampled(c, [&](hipEvent_t e0, hipEvent_t e1) {
    launch_k3(c->cv, c->state.p, c->partials.p, c->k3_grid, c->k3_single, c->k3_wide, force, c->stream, e0, e1);
  });
}
int harvest_k3_events(tloam_ctx* c, int working) {
  const int zero = 0;
  return harvest_k3_events_multi(c, 1, &zero, &working);
}
// one ceres::Solve on the current correspondence set, device resident: 1 + 4 sweeps at most;
// sweeps after a tolerance exit are no-op launches (GnState.done).
// prep: the launch also prepares the factor set (only the one-launch Solve, PrepareForm::IN_SOLVE)
// finish: ... and finishes the outer iteration, possibly running the following ones too (SolveFinish; needs prep).
// wp: the weight thresholds of the outer iteration this Solve belongs to (null: a Solve outside scanMatching) -- the
// one-launch Solve adds up the finish sums of its last evaluation for the finish kernel that follows.
int enqueue_solve(tloam_ctx* c, bool armed, int sweeps, const WeightParams* wp, const SolvePrep* prep, const SolveFinish* finish) {
  if (!armed) launch_solve_init(c->state.p, c->stream);  // scan_match re-arms the minimiser in its finish kernel
  if (sweeps <= 0) return TLOAM_OK;
  if (c->forms.solve == SolveForm::PERSISTENT) {
    // KITTI-size set: the whole Solve (up to `sweeps` evaluations) is one launch (k_solve_all)
    SolveFinish F;
    if (prep && finish) {
      F = *finish;
    } else {
      memset(&F, 0, sizeof(F));
      if (wp) { F.have_wp = 1; F.wp[0] = *wp; }
    }
    F.iter_span = iter_span_of(c);
    const int sabotage = c->dbg_fail_handover > 0 ? (c->dbg_fail_handover--, 1 << 16) : 0;   // test hook, see k_solve_all
    launch_solve_small(c->cv, c->state.p, c->partials.p, c->k3_ticket.p, c->k3_grid, sweeps | sabotage, prep, c->seg_n.p, &F, c->stream);
    c->batch_launches++;
    return TLOAM_OK;
  }
  for (int sweep = 0; sweep < sweeps; ++sweep) {
    int rc = TLOAM_OK;
    switch (c->forms.solve) {
      case SolveForm::PERSISTENT: break;   // (above)
      case SolveForm::FUSED_LARGE:
        // One GN iteration = ONE launch whatever the size of the set (round 4): the streaming sweep's last block folds the rows
        // and advances the minimiser (k3_sweep_step); with a mailbox it also posts, gathers and advances -- sweep + exchange + step
        rc = launch_k3_step_timed(c);
        break;
      case SolveForm::SHARDED_MBOX:
      case SolveForm::SHARDED_COLLECTIVE: {
        // sharded GN iteration = 2 launches (+ the collective): the sweep, whose last block folds the rows into the
        // 48-double buffer (the 42 normal-equation scalars + cost) and -- with the mailbox -- stores it straight into
        // every rank's buffer over xGMI; then the step, which (mailbox) adds the ranks' rows in rank order itself.
        // RCCL / callback contexts keep sweep | collective | step: the collective is enqueued by the host between two launches
        const bool mbox = c->forms.solve == SolveForm::SHARDED_MBOX;
        K3Fuse fuse;
        memset(&fuse, 0, sizeof(fuse));
        fuse.ticket = c->k3_ticket.p;
        fuse.out48 = c->red48.p;
        if (mbox) fuse.mb = c->mbox;
        launch_k3_fused(c->cv, c->state.p, c->partials.p, c->k3_grid, c->k3_single, c->k3_wide, false, fuse, c->stream);
        c->batch_launches++;
        if (mbox) {
          launch_gn_step_mbox(c->state.p, c->mbox, c->stream, iter_span_of(c));
        } else {
          rc = allreduce(c, c->red48.p, kReduceBuf);
          if (rc == TLOAM_OK) launch_gn_step(c->state.p, c->red48.p, c->stream, iter_span_of(c));
        }
        break;
      }
      case SolveForm::SMALL_STEP:
        // KITTI-size set: one launch per GN iteration (k_sweep_step_small)
        launch_sweep_step_small(c->cv, c->state.p, c->partials.p, c->k3_ticket.p, c->k3_grid, c->stream, iter_span_of(c));
        c->batch_launches++;
        break;
      case SolveForm::SWEEP_REDUCE:
        rc = launch_k3_timed(c, false);
        if (rc == TLOAM_OK) launch_reduce_and_step(c->partials.p, c->k3_grid, c->state.p, c->stream, iter_span_of(c));
        break;
    }
    if (rc != TLOAM_OK) return rc;
  }
  return TLOAM_OK;
}
}  // namespace tlh

// ---- pieces of one outer GNC iteration, shared by the stepwise API (the host decides between iterations) and by
//      tloam_scan_match's device-driven loop (every iteration enqueued at once, one host wait per frame) -----------
namespace {
constexpr int kMaxOuterFast = kMirrorSlots;   // outer iterations the device-driven loop plans for
// :976-1020 the four builders (K1 + K2), then the flag scan, the index-order caps and the compaction as the frame's prepare form
// says.  refresh_gate: the call stands for both alternatives of a device-gated iteration (compaction, or the refresh of the
// unchanged set).
// ride: the finish of the previous outer iteration rides on this search launch (large single-rank sets, device-driven loop:
// k_build_finish_large; the search then runs on GnState::spec_build instead of `gate`)
int enqueue_build(tloam_ctx* c, const BuildParams& bp, const GridView grids[kKinds], bool rebin, const int* gate,
                  const int* refresh_gate = nullptr, const FinishLargeArgs* ride = nullptr, int iter = 0) {
  const size_t n_slots = (size_t)c->sv.slot_off[kKinds];
  // direct set: the search writes the rows itself -- no flag scan, no compaction, no refresh (the Solve reads the live weight stream)
  const bool dir = direct(c);
  const DirectSet ds{dir ? 1 : 0, rebin ? 1 : 0, (ride && !rebin) ? 0 : 1, dir ? direct_blk_cnt(c, iter) : nullptr,
                     c->tile_of_slot.p, c->tile_scan.p, dir ? c->row_of_pos.p : nullptr};
  if (ride && !rebin) {
    const size_t ntiles = (size_t)build_tile_count(grids, c->sv.slot_off);
    launch_build_finish_large(c->sv, grids, bp, c->state.p, c->tile_scan.p + ntiles, c->qrec.p, *ride, c->stream, dir ? &ds : nullptr);
  } else {
    launch_build(c->sv, grids, bp, c->state.p, c->tile_of_slot.p, c->tile_cnt.p, c->tile_scan.p, c->tile_fill.p,
                 c->qrec.p, c->scan_tmp.p, rebin, c->stream, gate, c->scan1p_q_use ? c->scan1p_q.p : nullptr, c->h_fault.dev + kFaultScan1p,
                 dir ? &c->cv : nullptr, dir ? &ds : nullptr, rebin && c->qbin_rode);
    if (rebin) c->qbin_rode = false;   // (consumed: a second sort of this frame -- a re-run -- bins for itself)
  }
  switch (c->forms.prepare) {
    case PrepareForm::NONE:
    case PrepareForm::IN_SOLVE:   // (the Solve launch that follows is handed a SolvePrep; tloam_sm_outer, which hands none, prepares)
      return TLOAM_OK;
    case PrepareForm::SMALL:
      // small single-rank frames: the scan, the caps, the compaction AND the alternative (refresh) are one launch
      launch_prepare_small(c->sv, c->cv, bp, c->seg_n.p, c->state.p, gate, refresh_gate, c->stream);
      return TLOAM_OK;
    case PrepareForm::TILES: {
      // single rank: the tile-local scan only -- the compaction adds the tiles' offsets itself -- and ONE launch for both
      // alternatives of a device-gated iteration (compaction, or the refresh of the unchanged set): two launches less
      const int tiles = scan_tiles_only(c->flags.p, c->scan.p, n_slots + 1, c->scan_tmp.p, c->stream, gate);
      if (tiles > 0) {
        launch_compact(c->sv, c->cv, bp, c->seg_n.p, nullptr, 0, 1, c->state.p, c->stream, gate, refresh_gate, c->scan_tmp.p, tiles);
        return TLOAM_OK;
      }
      break;   // (too few slots for tiles: the full scan)
    }
    case PrepareForm::FULL: break;
  }
  const bool sharded = c->forms.prepare == PrepareForm::FULL;   // (not a tile scan that fell through: that is one rank)
  launch_exclusive_scan_u64(c->flags.p, c->scan.p, n_slots + 1, c->scan_tmp.p, c->stream, gate);
  const double* rank_counts = nullptr;
  if (sharded) {
    launch_rank_counts(c->sv, c->rank_counts.p, c->rank, c->nranks, c->stream);
    const int rc = allreduce(c, c->rank_counts.p, c->nranks * kKinds);
    if (rc != TLOAM_OK) return rc;
    rank_counts = c->rank_counts.p;
  }
  // seg_n: every kind with slots and a positive cap is rewritten by the compaction, the others keep the 0 of
  // k_frame_init; only a sharded rank can find its cap already filled by the lower ranks and write nothing
  if (sharded) HIPC(c, hipMemsetAsync(c->seg_n.p, 0, kKinds * sizeof(int), c->stream));
  launch_compact(c->sv, c->cv, bp, c->seg_n.p, rank_counts, c->rank, c->nranks, c->state.p, c->stream, gate);
  if (refresh_gate) launch_refresh(c->sv, c->cv, c->stream, refresh_gate);
  return TLOAM_OK;
}
// budget of K3 sweeps of outer iteration `iter`: the most it needed in the last three frames
int planned_sweeps_for(tloam_ctx* c, int iter) {
  if ((int)c->planned_sweeps.size() < 3 * (iter + 1)) c->planned_sweeps.resize(3 * ((size_t)iter + 1), 0);  // 0 = no history yet
  const int* hist = &c->planned_sweeps[3 * (size_t)iter];
  int planned = hist[0] == 0 ? kSolveSweeps  // first frame of this context: the full budget
                             : std::min(std::max(std::max(hist[0], hist[1]), std::max(hist[2], 1)), kSolveSweeps);
  if (c->forms.solve == SolveForm::PERSISTENT) planned = kSolveSweeps;   // one launch runs the Solve to its end: nothing to predict
  if (c->dbg_planned_sweeps > 0) planned = std::min(c->dbg_planned_sweeps, kSolveSweeps);
  return planned;
}
WeightParams weight_params(const tloam_ctx* c, double mu, const BuildParams& bp) {
  WeightParams wp;
  wp.th1 = (mu + 1) / mu * c->noise_bound_sq;   // :1049
  wp.th2 = mu / (mu + 1) * c->noise_bound_sq;   // :1050
  wp.mu = mu;
  wp.noise_bound_sq = c->noise_bound_sq;
  for (int k = 0; k < kKinds; ++k) wp.active[k] = bp.active[k];
  return wp;
}
double next_mu(const tloam_ctx* c, double mu, int iter) { return mu * exp((double)(iter + 1) * c->cfg.gnc_factor); }   // :1089
// a result slot's `incomplete` word as the outcome of its outer iteration: OS_COMM_ERROR and OS_INCOMPLETE become the error
// they stand for, with last_error; any other word is TLOAM_OK (a caller that tops an unfinished Solve up does so before it asks).
// *hand_over_timed_out (may be null) is set when the in-launch hand-over of one rank timed out: the device loop's fall-back.
int slot_error(tloam_ctx* c, int incomplete, bool* hand_over_timed_out) {
  if (incomplete == OS_COMM_ERROR) {
    if (exchanging(c)) {
      c->last_error = "mailbox exchange timed out: a peer rank did not post (dead process or diverged call sequence)";
      return TLOAM_E_RCCL;
    }
    c->last_error = "in-launch hand-over of the fused GN iteration timed out (a block of the grid never posted its row)";
    if (hand_over_timed_out) *hand_over_timed_out = true;
    return TLOAM_E_HIP;
  }
  if (incomplete == OS_INCOMPLETE) {
    c->last_error = "the minimiser did not terminate within its evaluation budget";
    return TLOAM_E_INVALID;
  }
  return TLOAM_OK;
}
// :1049-1086 thresholds + weight update, :1091-1094 cost sums, publish (+ device-side loop control when ctl.fast)
int enqueue_finish(tloam_ctx* c, const WeightParams& wp, const HostMirror& hm, const OuterCtl& ctl, int iter = 0, int built = 1) {
  const int wblocks = finish_wblocks(c);
  switch (c->forms.finish) {
    case FinishForm::DIRECT: {   // (c->cv carries the weight stream of outer iteration `iter`: direct_set_parity)
      const FinishLargeArgs fin = direct_finish_args(c, &c->cv, &wp, hm, ctl, iter, /*riding=*/0, built);
      launch_finish_direct(fin, c->state.p, c->stream);
      break;
    }
    case FinishForm::SMALL:   // one 1024-thread block does weights + sums + publish in a single launch
      launch_weights_finish_small(c->cv, c->sv, wp, c->seg_n.p, c->sums16.p, c->state.p, hm, ctl, c->stream);
      break;
    case FinishForm::LARGE:
      launch_weights(c->cv, c->sv, wp, c->wpart.p, wblocks, c->state.p, c->stream);
      launch_outer_finish(c->wpart.p, wblocks, c->seg_n.p, c->state.p, c->state.p, c->sums16.p, hm, ctl, c->stream);  // + publish + re-arm
      break;
    case FinishForm::SHARDED: {
      launch_weights(c->cv, c->sv, wp, c->wpart.p, wblocks, c->state.p, c->stream);
      launch_outer_finish(c->wpart.p, wblocks, c->seg_n.p, nullptr, c->state.p, c->sums16.p, hm, ctl, c->stream);
      const int rc = allreduce(c, c->sums16.p, 16);
      if (rc != TLOAM_OK) return rc;
      launch_outer_publish(c->sums16.p, c->state.p, hm, c->comm == COMM_MAILBOX ? c->mbox.ctr + 1 : nullptr, c->stream);
      break;
    }
  }
  return TLOAM_OK;
}
// host bookkeeping of a finished outer iteration from the mirrored state S (:1089-1121); returns whether the loop ends.
// *weight_violation: the reference's assert (:871) would have fired in this iteration.
bool account_outer(tloam_ctx* c, int iter, const GnState& S, double mu, int sweeps_before, bool* weight_violation) {
  // (an iteration that ran inside the launch of an earlier one was never planned: planned_sweeps_for has not sized the history)
  if (c->planned_sweeps.size() < 3 * ((size_t)iter + 1)) c->planned_sweeps.resize(3 * ((size_t)iter + 1), 0);
  int* hist = &c->planned_sweeps[3 * (size_t)iter];
  {
    const int used = std::min(std::max(S.gn_sweeps - sweeps_before, 1), kSolveSweeps);
    if (hist[0] == 0) hist[1] = hist[2] = used;  // the first observation stands for the whole window
    else { hist[2] = hist[1]; hist[1] = hist[0]; }
    hist[0] = used;
  }
  c->mu = next_mu(c, mu, iter);
  tloam_stats& st = c->stats;
  st.outer_iterations = iter + 1;
  st.gn_evaluations = S.gn_evaluations;
  st.gn_sweeps = S.gn_sweeps;
  st.host_wait_us = (int32_t)c->wait_us;
  st.gn_iterations = S.gn_iterations;
  st.accepted_steps = S.accepted_steps;
  *weight_violation = S.bad_weights > st.weight_range_violations;
  st.weight_range_violations = S.bad_weights;
  st.mu = c->mu;
  st.solver_cost = S.x_cost;
  memcpy(st.se3, S.x, sizeof(double) * 6);
  int nn[kKinds];
  for (int k = 0; k < kKinds; ++k) {
    c->cur_cost[k] = S.kind_cost[k];
    st.kind_cost[k] = S.kind_cost[k];
    st.n_corr[k] = S.n_corr[k];
    nn[k] = S.n_corr[k];
  }
  c->k3_alg_bytes = alg_bytes_of(nn);
  bool fin = false;
  if (fabs(c->cur_cost[TLOAM_KIND_PLANAR] - c->prev_cost[TLOAM_KIND_PLANAR]) < c->cfg.cost_threshold) {  // :1108
    st.converged_early = 1;
    fin = true;
  } else {
    for (int k = 0; k < kKinds; ++k) c->prev_cost[k] = c->cur_cost[k];  // :1113-1116 (slots re-zeroed by the next compaction)
    c->iter = iter + 1;
    if (c->iter >= c->cfg.max_iterations) fin = true;
  }
  if (fin) c->iter = c->cfg.max_iterations;
  return fin;
}
// :1027-1033.  When iteration 0 reaches this point no Evaluate() has run yet, so every residual slot the
// reference takes maxCoeff() over is still the 0 it was initialised with (:931-949); the literal formula
// then gives mu = 1/(0 - 1) = -1 -> 1e-10.
double initial_mu(const tloam_ctx* c) {
  const double max_residual = 0.0;
  double mu = 1 / (2 * max_residual / c->noise_bound_sq - 1.0);
  if (mu <= 0) mu = 1e-10;
  return mu;
}
// the set of outer iteration `iter` is (re)built iff the pose has moved since the last build (the frame's first always builds)
bool pose_moved_since_build(const tloam_ctx* c, int iter) {
  return iter == 0 || memcmp(c->build_x, c->stats.se3, sizeof(c->build_x)) != 0;
}

// ---- scanMatching with the outer GNC loop driven from the device ------------------------------------------------
// Every outer iteration of the frame is enqueued up front -- builders + scan + compaction gated on "the pose moved",
// the refresh gated on "it did not", the planned sweeps, the finish kernel, which makes the loop decisions of
// registration.cpp:1108-1121 itself (plateau break, max_iterations, the next iteration's gates) and mirrors the
// iteration's result into its own pinned slot -- and the host waits ONCE, for the last slot.  (The stepwise API keeps
// the host in the loop: one round trip of ~12 us plus ~4 us of launch catch-up per following kernel and per outer
// iteration on an otherwise idle GPU.)  A Solve that runs out of its planned budget stops the device loop; the host tops
// it up and re-enters the loop behind the top-up.
// KITTI-size frames (RideForm::IN_SOLVE: set prepared and iteration finished in the Solve launch): a frame is grid
// build + (search + Solve launch) per RUN of outer iterations -- the Solve launch ends its iteration itself and goes on
// with the next one while the pose stands still.  Only the launches of the first kEnqueueAhead iterations are enqueued up
// front; the host waits for the result slots IN ORDER and adds a (search, Solve) pair when a slot carries OS_NEEDS_HOST.
struct DeviceLoopPlan {
  int planned[kMaxOuterFast] = {}, solve_start[kMaxOuterFast] = {}, used[kMaxOuterFast] = {};
  double mus[kMaxOuterFast] = {};
  HostMirror hms[kMaxOuterFast];
  // finish-in-the-Solve mode (SolveFinish): the launches of iterations [0, enq_end) are in the stream; a later iteration is
  // enqueued when the device says that it is needed (OS_NEEDS_HOST) -- see scan_match_device_loop
  int enq_end = 0;
  SolveFinish F;
  SolvePrep prep;
};
bool in_launch_finish(const tloam_ctx* c) { return c->forms.finish_rides == RideForm::IN_SOLVE; }
// iterations enqueued ahead of the device's verdicts in finish-in-the-Solve mode: iteration 0 almost always moves the pose
// (so the search and the Solve of iteration 1 will run), the later ones almost never do (they run inside the launch of
// iteration 1): launches for them would be no-ops that the frame's successor has to queue behind.
constexpr int kEnqueueAhead = 2;   // (1 and 4 measured the same within noise and are bit-identical: round 3 / 4 A/Bs)
// finish-in-the-Solve mode: the launches of iterations [from, to): the search if the pose moved (always in the frame's
// first), then the Solve + finish -- a launch that returns at once when an earlier one has already run its iteration
int enqueue_iterations_in_launch_mode(tloam_ctx* c, int from, int to, const BuildParams& bp, const GridView grids[kKinds],
                                      DeviceLoopPlan& P) {
  GnState* st = c->state.p;
  for (int iter = from; iter < to; ++iter) {
    int rc = enqueue_build(c, bp, grids, /*rebin=*/iter == 0, iter == 0 ? nullptr : &st->run_build);
    if (rc != TLOAM_OK) return rc;
    P.prep.run_build = iter == 0 ? nullptr : &st->run_build;
    P.prep.run_refresh = iter == 0 ? nullptr : &st->run_refresh;
    P.F.first_iter = iter;
    P.planned[iter] = planned_sweeps_for(c, iter);
    P.solve_start[iter] = c->batch_launches;
    rc = enqueue_solve(c, /*armed=*/true, P.planned[iter], &P.F.wp[iter], &P.prep, &P.F);
    if (rc != TLOAM_OK) return rc;
  }
  if (to > P.enq_end) P.enq_end = to;
  return TLOAM_OK;
}
// enqueue outer iterations first .. M-1.  first == 0: the frame's first iteration (always builds).  first > 0: a restart
// behind a stand-alone finish of iteration first - 1 that has set the gates (run_build / run_refresh) on the device.
int enqueue_outer_iterations(tloam_ctx* c, int first, double mu, const BuildParams& bp, const GridView grids[kKinds],
                             DeviceLoopPlan& P) {
  const int M = c->cfg.max_iterations;
  GnState* st = c->state.p;
  const int* run_build = &st->run_build;
  const int* run_refresh = &st->run_refresh;
  // Where the finish of every iteration but the last goes.  ON_SEARCH_SMALL, KITTI-size frames: it does not get a launch of its
  // own, it rides on the correspondence search of the next iteration (k_build_finish_small: they are independent of each other);
  // ON_SEARCH_LARGE: 1 M-class frames the same way with k_weights + k_outer_finish (k_build_finish_large)
  const RideForm rides = c->forms.finish_rides;
  const int wblocks_large = finish_wblocks(c);
  if (rides == RideForm::ON_SEARCH_LARGE) HIPC(c, c->fin_rows.reserve((size_t)4 * 256 * 8));
  bool pending = false;   // the finish of the previous iteration has not been enqueued yet (it rides on this search)
  WeightParams wp_prev;
  OuterCtl ctl_prev{0.0, 0, 0};
  int rc = TLOAM_OK;
  // the scan + caps + compaction (or the refresh) of an iteration: a launch of its own (k_prepare_small), or the prologue of
  // the one-launch Solve (SolvePrep)
  const bool in_solve = c->forms.prepare == PrepareForm::IN_SOLVE;
  SolvePrep prep;
  memset(&prep, 0, sizeof(prep));
  prep.sv = c->sv;
  for (int k = 0; k < kKinds; ++k) prep.maxnum[k] = bp.maxnum[k];
  // ... and the finish of an iteration (weights, sums, loop decisions, result slot): a launch of its own / riding on the next
  // search, or the tail of the one-launch Solve, which then goes on with the next iteration itself while the pose stands still
  if (rides == RideForm::IN_SOLVE) {
    SolveFinish& F = P.F;
    memset(&F, 0, sizeof(F));
    F.enabled = 1;
    F.have_wp = 1;
    F.n_iter = M;
    F.cost_threshold = c->cfg.cost_threshold;
    F.sums16 = c->sums16.p;
    F.iter_span = iter_span_of(c);
    double m = mu;
    for (int iter = first; iter < M; ++iter) {
      P.mus[iter] = m;
      P.hms[iter] = next_mirror(c, iter);
      F.wp[iter] = weight_params(c, m, bp);
      F.hm[iter] = P.hms[iter];
      m = next_mu(c, m, iter);
    }
    P.prep = prep;
    P.enq_end = first;
    return enqueue_iterations_in_launch_mode(c, first, std::min(M, first + kEnqueueAhead), bp, grids, P);
  }
  for (int iter = first; iter < M; ++iter) {
    if (direct(c)) direct_set_parity(c, iter);   // what this iteration's Solve (and its finish) read; the search does not care
    if (iter == 0) {
      rc = enqueue_build(c, bp, grids, /*rebin=*/true, nullptr);
    } else if (pending && rides == RideForm::ON_SEARCH_SMALL) {
      FinishSmallArgs fin{&c->cv, &wp_prev, c->seg_n.p, c->sums16.p, P.hms[iter - 1], ctl_prev, c->wpart.p, c->k3_ticket.p + 1};
      launch_build_finish_small(c->sv, grids, bp, st, fin, c->stream);
      if (c->forms.prepare == PrepareForm::SMALL) launch_prepare_small(c->sv, c->cv, bp, c->seg_n.p, st, run_build, run_refresh, c->stream);
    } else if (pending) {   // (ON_SEARCH_LARGE)
      FinishLargeArgs fin{&c->cv, &wp_prev, c->seg_n.p, c->sums16.p, P.hms[iter - 1], ctl_prev, c->fin_rows.p, c->k3_ticket.p + 1,
                          wblocks_large, {}};
      CorrView cv_prev = c->cv;
      if (direct(c)) {   // the finish of iteration iter - 1 reads ITS weight stream and writes this iteration's
        for (int k = 0; k < kKinds; ++k) cv_prev.k[k].w = direct_w_stream(c, k, (iter - 1) & 1);
        fin = direct_finish_args(c, &cv_prev, &wp_prev, P.hms[iter - 1], ctl_prev, iter - 1, /*riding=*/1, iter - 1 == 0 ? 1 : -1);
      }
      rc = enqueue_build(c, bp, grids, /*rebin=*/false, run_build, run_refresh, &fin, iter);
    } else {
      rc = enqueue_build(c, bp, grids, /*rebin=*/false, run_build, run_refresh, nullptr, iter);   // both alternatives, device-gated
    }
    pending = false;
    if (rc != TLOAM_OK) return rc;
    prep.run_build = iter == 0 ? nullptr : run_build;   // (the frame's first iteration always builds: no gate)
    prep.run_refresh = iter == 0 ? nullptr : run_refresh;
    P.planned[iter] = planned_sweeps_for(c, iter);
    P.solve_start[iter] = c->batch_launches;
    const WeightParams wp_iter = weight_params(c, mu, bp);
    rc = enqueue_solve(c, /*armed=*/true, P.planned[iter], &wp_iter, in_solve ? &prep : nullptr);
    if (rc != TLOAM_OK) return rc;
    P.mus[iter] = mu;
    P.hms[iter] = next_mirror(c, iter);
    const OuterCtl ctl{c->cfg.cost_threshold, 1, iter == M - 1 ? 1 : 0};
    if (rides != RideForm::NO && iter < M - 1) {
      wp_prev = weight_params(c, mu, bp);
      ctl_prev = ctl;
      pending = true;
    } else {
      rc = enqueue_finish(c, weight_params(c, mu, bp), P.hms[iter], ctl, iter, iter == 0 ? 1 : -1);
      if (rc != TLOAM_OK) return rc;
    }
    mu = next_mu(c, mu, iter);
  }
  return TLOAM_OK;
}

// The host's wait for outer iteration `iter`.  frame_first (behind everything the frame enqueues: its start, a top-up): the last
// slot first -- it is written last (stream order), whatever the frame did; the iteration's own slot was written before it and
// is already there -- this only unpacks it.  Finish-in-the-Solve mode: the slots are waited for in order -- the frame's result
// is there when its last iteration's is, and a launch may have to be added on the way.
int wait_slots(tloam_ctx* c, const DeviceLoopPlan& P, int iter, bool frame_first) {
  const int M = c->cfg.max_iterations;
  if (frame_first && !in_launch_finish(c)) {
    const int rc = wait_state(c, P.hms[M - 1], M - 1);
    if (rc != TLOAM_OK) return rc;
  }
  if (iter < M - 1 || in_launch_finish(c)) return wait_state(c, P.hms[iter], iter);
  return TLOAM_OK;
}

int scan_match_device_loop(tloam_ctx* c, bool* weight_violation) {
  const int M = c->cfg.max_iterations;
  BuildParams bp;
  GridView grids[kKinds];
  outer_params(c, &bp, grids);
  int rc = reserve_query_sort(c, grids);
  if (rc != TLOAM_OK) return rc;
  GnState* st = c->state.p;
  DeviceLoopPlan P;
  rc = enqueue_outer_iterations(c, 0, initial_mu(c), bp, grids, P);
  if (rc != TLOAM_OK) return rc;
  // ---- the frame's bookkeeping, iteration by iteration, from the mirrored slots
  int topups = 0;
  for (int iter = 0; iter < M; ++iter) {
    rc = wait_slots(c, P, iter, /*frame_first=*/iter == 0);
    if (rc != TLOAM_OK) return rc;
    GnState* Sm = &c->h_state[iter];
    const bool needs_host = (Sm->incomplete & OS_NEEDS_HOST) != 0;
    if (Sm->incomplete & OS_SET_STALE) c->set_stale = true;   // (direct set: the loop ended beside a search that had already run)
    Sm->incomplete &= ~(int)(OS_NEEDS_HOST | OS_SET_STALE);
    const GnState* S = Sm;
    if (S->host_seq != P.hms[iter].seq) {
      c->last_error = "device-driven loop: the result slot of an outer iteration was not written";
      return TLOAM_E_HIP;
    }
    if (S->incomplete == OS_SKIPPED) break;   // the loop had ended before this iteration
    if (S->incomplete == OS_COMM_ERROR) return slot_error(c, OS_COMM_ERROR, &c->hand_over_timed_out);
    if (S->incomplete == OS_INCOMPLETE) {
      // The Solve of this iteration ran out of its planned budget: the device stopped the loop there (the sweeps of
      // the later iterations, gated only on `done`, have meanwhile continued this same Solve; their builds, refreshes
      // and finish kernels were gated off).  Top the Solve up to its full budget, finish the iteration with the DEVICE
      // deciding as usual, and enqueue the rest of the frame behind it: one more wait instead of a host round trip per
      // remaining outer iteration.
      if (++topups > M) {
        c->last_error = "the minimiser did not terminate within its evaluation budget";
        return TLOAM_E_INVALID;
      }
      HIPC(c, hipMemsetAsync(&st->stop, 0, sizeof(int), c->stream));
      P.solve_start[iter] = c->batch_launches;
      P.planned[iter] = kSolveSweeps;
      const WeightParams wp_top = weight_params(c, P.mus[iter], bp);
      if (direct(c)) direct_set_parity(c, iter);
      rc = enqueue_solve(c, /*armed=*/true, kSolveSweeps, &wp_top);
      if (rc != TLOAM_OK) return rc;
      P.hms[iter] = next_mirror(c, iter);
      // (the finish that found the Solve unfinished has cleared the device's gates: whether this iteration built its set is the
      //  host's to say -- the pose the previous iteration ended at against the pose of the last build, as the bookkeeping below)
      const int built_top = pose_moved_since_build(c, iter) ? 1 : 0;
      rc = enqueue_finish(c, wp_top, P.hms[iter], OuterCtl{c->cfg.cost_threshold, 1, iter == M - 1 ? 1 : 0}, iter, built_top);
      if (rc != TLOAM_OK) return rc;
      if (iter + 1 < M) {
        rc = enqueue_outer_iterations(c, iter + 1, next_mu(c, P.mus[iter], iter), bp, grids, P);
        if (rc != TLOAM_OK) return rc;
      }
      rc = wait_slots(c, P, iter, /*frame_first=*/true);
      if (rc != TLOAM_OK) return rc;
      S = &c->h_state[iter];
      rc = slot_error(c, S->incomplete, &c->hand_over_timed_out);
      if (rc != TLOAM_OK) return rc;
    }
    const int sweeps_before = c->stats.gn_sweeps;
    // the compact set of this iteration was (re)built iff the pose had moved since the last build
    if (pose_moved_since_build(c, iter)) memcpy(c->build_x, c->stats.se3, sizeof(c->build_x));
    c->have_build = true;
    c->mu = P.mus[iter];
    bool wv = false;
    const bool fin = account_outer(c, iter, *S, P.mus[iter], sweeps_before, &wv);
    P.used[iter] = std::min(S->gn_sweeps - sweeps_before, P.planned[iter]);
    if (wv) *weight_violation = true;
    if (fin) break;
    // the launch that ran this iteration has ended because the pose moved: the search and the Solve of the next one, unless
    // they are in the stream already
    if (in_launch_finish(c) && needs_host && iter + 1 >= P.enq_end && iter + 1 < M) {
      const bool trace = getenv("TLOAM_DEBUG_RESUME") != nullptr;   // development aid / test census: how often the host adds a launch
      if (trace) fprintf(stderr, "[tloam resume] outer iteration %d enqueued by the host\n", iter + 1);
      rc = enqueue_iterations_in_launch_mode(c, iter + 1, iter + 2, bp, grids, P);
      if (rc != TLOAM_OK) return rc;
    }
  }
  rc = harvest_k3_events_multi(c, M, P.solve_start, P.used);
  if (rc != TLOAM_OK) return rc;
  if (direct(c)) {   // what the getters and the timing helpers see: the weights the LAST Solve captured; the current ones: the other stream
    const int K = std::max(c->stats.outer_iterations, 1);
    direct_set_parity(c, K - 1);
    c->w_parity = K & 1;
  }
  return 0;
}
}  // namespace

extern "C" {

// ---- scanMatching, stepwise ---------------------------------------------------------------------
int tloam_sm_begin(tloam_ctx* c, const double predict[16], const double* omega3) {
  if (!c || !predict) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  for (int k = 0; k < kKinds; ++k)  // the reference asserts (registration.cpp:928-929)
    if (c->kd[k].n_src_full < 10 || c->kd[k].n_tgt < 10) return TLOAM_E_TOO_FEW_POINTS;
  for (int k = 0; k < kKinds; ++k)  // a hand-over that failed half way (staging, upload) left nothing registered
    if (!c->kd[k].src_set || !c->kd[k].tgt_set) { c->last_error = "a source / target hand-over failed: hand the frame over again"; return TLOAM_E_NOT_READY; }
  Pose P;
  if (!pose_from_matrix(predict, &P)) return TLOAM_E_BAD_POSE;  // SOPHUS_ENSURE in the reference
  double x[6];
  se3_log(P, x);  // :881
  if (sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < 1e-2) {  // :884-886
    double u[3] = {0.0, 0.0, 1.0};
    if (omega3) {
      const double nn = sqrt(omega3[0] * omega3[0] + omega3[1] * omega3[1] + omega3[2] * omega3[2]);
      if (nn > 0.0) { u[0] = omega3[0] / nn; u[1] = omega3[1] / nn; u[2] = omega3[2] / nn; }
    }
    x[3] = u[0] * 1e-4; x[4] = u[1] * 1e-4; x[5] = u[2] * 1e-4;
  }
  int rc = ensure_common(c);
  if (rc != TLOAM_OK) return rc;
  // ---- per-source-slot arrays (:931-949 weights = 1, residual slots = 0)
  size_t off = 0;
  for (int k = 0; k < kKinds; ++k) {
    c->sv.slot_off[k] = (int)off;
    c->sv.src_lo[k] = (int)c->kd[k].src_lo;
    off += c->kd[k].n_src;
  }
  c->sv.slot_off[kKinds] = (int)off;
  const size_t ns = std::max<size_t>(off, 1);
  HIPC(c, c->sx.reserve(ns)); HIPC(c, c->sy.reserve(ns)); HIPC(c, c->sz.reserve(ns)); HIPC(c, c->w_src.reserve(ns));
  HIPC(c, c->raw.reserve(ns * 8));
  HIPC(c, c->flags.reserve(ns + 1)); HIPC(c, c->scan.reserve(ns + 1));
  HIPC(c, c->scan_tmp.reserve(scan_scratch_elems(ns + 1)));
  c->sv.sx = c->sx.p; c->sv.sy = c->sy.p; c->sv.sz = c->sz.p; c->sv.w_src = c->w_src.p;
  c->sv.raw = c->raw.p;
  c->sv.flags = c->flags.p; c->sv.scan = c->scan.p;
  c->set_stale = false;
  c->w_parity = 0;
  // ---- compact segments: at most min(n_src, maxnum) factors per kind (a direct set: one row per source point, which is the same)
  for (int k = 0; k < kKinds; ++k) {
    const size_t cap = std::min<size_t>(c->kd[k].n_src, (size_t)std::max(kind_maxnum(c->cfg, k), 0));
    rc = reserve_seg(c, k, cap);
    if (rc != TLOAM_OK) return rc;
  }
  c->prebuilt = false;
  plan_sweeps(c);
  // ---- the frame's shape is known: its launch forms.  Everything below, and every later call of the frame, reads them
  c->forms = decide_forms(forms_in(c));
  if (direct(c)) {
    HIPC(c, c->fin_rows.reserve(kFinRowsDoubles));
    c->blk_cnt_n = (off + 63) / 64;   // one-wave blocks of the thread-per-query search (logical: the sorted queries, 64 each)
    HIPC(c, c->blk_cnt.reserve(2 * c->blk_cnt_n * kKinds + 8));
    HIPC(c, c->row_of_pos.reserve(off + 64));
    if (!c->fin_tickets.p) {
      HIPC(c, c->fin_tickets.reserve(128));
      HIPC(c, hipMemsetAsync(c->fin_tickets.p, 0, c->fin_tickets.cap * sizeof(int), c->stream));
    }
  }
  // the one-launch Solve compacts the factor set itself when every kind's flag bytes fit a wave (SlotView::flagb)
  c->sv.flagb = nullptr;
  if (c->forms.prepare == PrepareForm::IN_SOLVE) {
    HIPC(c, c->flagb.reserve((size_t)kKinds * kFlagbStride));
    c->sv.flagb = c->flagb.p;
  }
  rc = reserve_partials(c);
  if (rc != TLOAM_OK) return rc;
  // ---- the start of the frame -- scan-frame sources AoS -> SoA slots, weights = 1 (:931-949), flag-scan terminator,
  //      minimiser state zeroed with `parameters` = x (passed by value) and armed for the first Solve -- rides on the
  //      first launch of the grid build
  FrameInitHook hook;
  memset(&hook, 0, sizeof(hook));
  for (int k = 0; k < kKinds; ++k) { hook.fi.src_aos[k] = c->kd[k].src_ptr; hook.fi.slot_off[k] = c->sv.slot_off[k]; }
  hook.fi.slot_off[kKinds] = c->sv.slot_off[kKinds];
  for (int i = 0; i < 6; ++i) hook.fi.x[i] = x[i];
  hook.fi.no_eval_reuse = c->dbg_no_eval_reuse ? 1 : 0;
  hook.fi.direct = direct(c) ? 1 : 0;
  if (direct(c)) direct_set_parity(c, 0);
  // 1 M-class single-rank frames: the first pass of the query sort rides on the last launch of the grid build (QueryBinRide)
  QueryBinRide qbin;
  memset(&qbin, 0, sizeof(qbin));
  c->qbin_rode = false;
  if (c->forms.qbin_ride) {
    qbin.sv = c->sv;
    qbin.bp = build_params(c);
    qbin.st = c->state.p;
    hook.qbin = &qbin;
  }
  hook.b = FrameInitBufs{c->sx.p, c->sy.p, c->sz.p, c->w_src.p, c->flags.p, c->state.p, c->seg_n.p};
  hook.n_slots = c->sv.slot_off[kKinds];
  // ---- :889-915 four search structures over the submap clouds: one launch per build phase for all kinds
  {
    double radius[kKinds];
    GridView views[kKinds];
    for (int k = 0; k < kKinds; ++k) radius[k] = kind_radius(c->cfg, k);
    // a sharded rank searches only the kinds it holds source points of (tloam_shard_ranges_frame): the other grids are not built
    if (c->nranks > 1)
      for (int k = 0; k < kKinds; ++k)
        if (c->kd[k].n_src == 0) radius[k] = 0.0;
    if (c->grids_ahead && c->grids_next_gen == c->tgt_gen && one_rank(c)) {
      // built when the targets were handed over (tloam_set_target_frame): they become the context's search structures now;
      // the frame's start is a launch of its own, below.  Used once: a second scanMatching over the same targets builds its own
      std::swap(c->grids, c->grids_next);
      for (int k = 0; k < kKinds; ++k) { c->kd[k].gv = c->gv_next[k]; c->kd[k].grid_valid = true; }
      c->grids_ahead = false;
    } else {
      rc = build_grids(c, c->grids, radius, views, &hook);
      if (rc != TLOAM_OK) return rc;
      c->qbin_rode = hook.qbin_done;
      // (a kind whose grid was skipped -- radius forced to 0 above: a sharded rank without source points of it -- has an EMPTY
      //  view: it is not a search structure getFitnessScore or anybody else may use)
      for (int k = 0; k < kKinds; ++k) { c->kd[k].gv = views[k]; c->kd[k].grid_valid = radius[k] > 0.0; }
    }
  }
  if (!hook.consumed) {  // (no grid launch: cannot happen with >= 10 targets per kind, kept for safety)
    GridView gviews[kKinds];
    for (int k = 0; k < kKinds; ++k) gviews[k] = c->kd[k].gv;
    const size_t ntiles = (size_t)build_tile_count(gviews, c->sv.slot_off);
    rc = reserve_tile_hist(c, ntiles, /*frame_start=*/true);
    if (rc != TLOAM_OK) return rc;
    hook.fi.tile_cnt = c->tile_cnt.p;
    hook.fi.n_tile_cnt = (int)ntiles + 1;
    launch_frame_init(hook.fi, hook.b, c->stream);
  }
  if (direct(c)) {
    // a kind whose target cloud has no finite point has no search grid: its queries are not in the sorted order, and the rows of a
    // direct set ARE that order -- such a frame compacts (the frame's start, already enqueued, has set seg_n to the row counts)
    FormsIn in = forms_in(c);
    for (int k = 0; k < kKinds; ++k) in.has_grid[k] = c->kd[k].gv.n > 0 ? 1 : 0;
    c->forms = decide_forms(in);
    if (!direct(c)) HIPC(c, hipMemsetAsync(c->seg_n.p, 0, kKinds * sizeof(int), c->stream));
  }
  c->wait_us = 0.0;
  c->mu = 1.0;  // :961
  c->noise_bound_sq = c->cfg.noise_bound * c->cfg.noise_bound;
  if (c->noise_bound_sq < 1e-16) c->noise_bound_sq = 1e-2;  // :963-964
  for (int k = 0; k < kKinds; ++k) { c->prev_cost[k] = INFINITY; c->cur_cost[k] = INFINITY; }  // :952-959
  c->iter = 0;
  c->active = true;
  c->have_build = false;
  memset(&c->stats, 0, sizeof(c->stats));
  memcpy(c->stats.se3, x, sizeof(x));
  c->ev_used = 0;
  c->ev_batch_idx.clear();
  c->batch_launches = 0;
  return TLOAM_OK;
}

int tloam_sm_outer(tloam_ctx* c, int* done, tloam_stats* stats) {
  if (!c || !c->active) return TLOAM_E_NOT_READY;
  HIPC(c, hipSetDevice(c->device));
  const int iter = c->iter;
  if (iter >= c->cfg.max_iterations) {  // loop condition :966
    if (done) *done = 1;
    if (stats) *stats = c->stats;
    return TLOAM_OK;
  }
  int rc;
  BuildParams bp;
  GridView grids[kKinds];
  outer_params(c, &bp, grids);
  rc = reserve_query_sort(c, grids);
  if (rc != TLOAM_OK) return rc;
  // The correspondence search is a pure function of (pose, clouds).  In the reference's GNC dynamics the
  // outer iterations after the first usually reject every step, so the pose -- hence every
  // neighbour list, fit and gate -- is bit-identical to the previous outer iteration: then only the
  // captured weights and the zeroed side-channel slots of the compact set have to be refreshed.
  const bool same_pose = c->have_build && !pose_moved_since_build(c, iter) && !c->dbg_no_build_reuse;
  if (direct(c)) direct_set_parity(c, iter);
  if (!same_pose) {
    rc = enqueue_build(c, bp, grids, /*rebin=*/iter == 0, nullptr, nullptr, nullptr, iter);
    if (rc != TLOAM_OK) return rc;
    // (the host between the iterations hands the Solve no SolvePrep: a set whose flag bytes fit is prepared like any small one)
    if (c->forms.prepare == PrepareForm::IN_SOLVE) launch_prepare_small(c->sv, c->cv, bp, c->seg_n.p, c->state.p, nullptr, nullptr, c->stream);
    memcpy(c->build_x, c->stats.se3, sizeof(c->build_x));
    c->have_build = true;
  } else if (!direct(c)) {
    launch_refresh(c->sv, c->cv, c->stream);
  }
  if (iter == 0) c->mu = initial_mu(c);
  // ---- :1036-1047 ceres::Solve, device resident.  Only as many sweeps as this outer iteration needed in the
  //      last three frames are enqueued (typically 2 of 5 from the second iteration on: the retried rejected steps
  //      are served by the evaluation reuse); the weight update and the finish kernel are gated on the
  //      minimiser having terminated, and raise `incomplete` otherwise -- then the Solve is topped up.
  const int planned = planned_sweeps_for(c, iter);
  const double mu = c->mu;
  const WeightParams wp = weight_params(c, mu, bp);
  rc = enqueue_solve(c, /*armed=*/true, planned, &wp);  // armed by sm_begin / the previous iteration's finish kernel
  if (rc != TLOAM_OK) return rc;
  const OuterCtl host_decides{c->cfg.cost_threshold, 0, 0};
  const int sweeps_before = c->stats.gn_sweeps;
  for (int attempt = 0;; ++attempt) {
    const HostMirror hm = next_mirror(c);
    rc = enqueue_finish(c, wp, hm, host_decides, iter, same_pose ? 0 : 1);
    if (rc != TLOAM_OK) return rc;
    rc = wait_state(c, hm);
    if (rc != TLOAM_OK) return rc;
    if (!c->h_state->incomplete) break;
    if (c->h_state->incomplete == OS_COMM_ERROR) return slot_error(c, OS_COMM_ERROR, nullptr);
    if (attempt > 0 || planned >= kSolveSweeps) return slot_error(c, OS_INCOMPLETE, nullptr);
    rc = enqueue_solve(c, /*armed=*/true, kSolveSweeps - planned, &wp);  // top up, then weights + finish again
    if (rc != TLOAM_OK) return rc;
  }
  const GnState& S = *c->h_state;
  rc = harvest_k3_events(c, S.gn_sweeps - sweeps_before);
  if (rc != TLOAM_OK) return rc;
  bool weight_violation = false;
  const bool fin = account_outer(c, iter, S, mu, sweeps_before, &weight_violation);
  if (direct(c)) c->w_parity = (iter + 1) & 1;   // (c->cv stays on the stream this Solve captured)
  if (done) *done = fin ? 1 : 0;
  if (stats) *stats = c->stats;
  return weight_violation ? TLOAM_E_WEIGHT_RANGE : TLOAM_OK;  // the iteration is complete either way (:871)
}

int tloam_sm_end(tloam_ctx* c, double result[16], tloam_stats* stats) {
  if (!c || !c->active || !result) return TLOAM_E_NOT_READY;
  const Pose T = se3_exp(c->stats.se3);  // :1124 exp(se3_pose_).matrix()
  pose_to_matrix(T, result);
  if (stats) *stats = c->stats;
  c->active = false;
  return check_device_faults(c);   // (every iteration's result has been waited for: the frame's kernels are done)
}

int tloam_scan_match(tloam_ctx* c, const double predict[16], const double* omega3, double result[16],
                     double* scan_xyz, size_t n_scan, tloam_stats* stats) {
  if (n_scan > kMaxPoints) return TLOAM_E_INVALID;
  static const bool stamps = getenv("TLOAM_HOST_STAMPS") != nullptr;
  const double hs0 = stamps ? host_now_us() : 0.0;
  if (c) c->hs_entry = hs0;
  int rc = tloam_sm_begin(c, predict, omega3);
  if (rc != TLOAM_OK) return rc;
  const double hs1 = stamps ? host_now_us() : 0.0;
  // which bounded wait of the look-back scan ran out, if any (to be read before check_device_faults clears the words)
  auto scan_fault_raised = [&] { return c->h_fault && __atomic_load_n(&c->h_fault[kFaultScan1p], __ATOMIC_ACQUIRE) != 0u; };
  // A look-back scan of this frame gave up: the clouds are intact in HBM and check_device_faults has switched the context to the
  // multi-launch scans -- the frame is run again, once per context.  Otherwise the frame returns rc_in
  auto rerun_after_scan_fault = [&](bool scan_fault, int rc_in) -> int {
    if (!scan_fault || c->scan1p_retried) return rc_in;
    c->scan1p_retried = true;
    return tloam_scan_match(c, predict, omega3, result, scan_xyz, n_scan, stats);
  };
  // A frame that fails on the way -- an unwritten result slot, a minimiser that "did not terminate", a time-out inside a launch --
  // may have failed on the garbage a timed-out look-back scan left behind: the frame is closed, the fault words are looked at
  // (check_device_faults moves the context to the forms that wait for nothing and clears them: the NEXT frame is not blamed), and
  // if it was the scan the frame is run again, as behind tloam_sm_end.
  auto frame_failed = [&](int rc_in) -> int {
    (void)hipStreamSynchronize(c->stream);
    c->active = false;
    const bool scan_fault = scan_fault_raised();
    (void)check_device_faults(c);
    return rerun_after_scan_fault(scan_fault, rc_in);
  };
  int done = 0;
  bool weight_violation = false;
  if (c->forms.loop == LoopForm::DEVICE) {   // (else the stepwise machinery below)
    rc = scan_match_device_loop(c, &weight_violation);
    if (rc == TLOAM_E_HIP && c->forms.solve == SolveForm::PERSISTENT && c->hand_over_timed_out) {
      // A block of the one-launch Solve was never scheduled beside the others (a device shared with long-running kernels,
      // fewer usable CUs than the attribute says): the waits inside the launch are bounded, the frame is intact in HBM --
      // solve it again with one launch per GN iteration, and keep this context on that path (the forms follow from the knob:
      // tloam_sm_begin decides them again).
      c->no_persistent_solve = true;
      c->persistent_solve_timed_out = true;
      c->fallback_events++;
      c->hand_over_timed_out = false;
      (void)hipStreamSynchronize(c->stream);
      c->active = false;
      rc = tloam_sm_begin(c, predict, omega3);
      if (rc != TLOAM_OK) return rc;
      weight_violation = false;
      rc = scan_match_device_loop(c, &weight_violation);
    }
    if (rc < 0) return frame_failed(rc);
    done = rc == 0 ? 1 : 0;
  }
  while (!done) {
    rc = tloam_sm_outer(c, &done, nullptr);
    if (rc == TLOAM_E_WEIGHT_RANGE) { weight_violation = true; continue; }  // reported after the solve
    if (rc != TLOAM_OK) return frame_failed(rc);
  }
  const double hs2 = stamps ? host_now_us() : 0.0;
  const bool scan_fault = scan_fault_raised();   // (tloam_sm_end's check_device_faults clears the words)
  rc = tloam_sm_end(c, result, stats);
  if (stamps && c) {
    const double hs3 = host_now_us();
    if (c->hs_exit > 0.0) c->hs[0] += hs0 - c->hs_exit;   // the caller, between two calls
    c->hs[1] += hs1 - hs0;                                 // sm_begin: set-up + the grid build's launches
    c->hs[2] += hs2 - hs1 - c->wait_us;                    // the loop: enqueueing, bookkeeping (without the wait)
    c->hs[3] += c->wait_us;
    c->hs[4] += hs3 - hs2;                                 // sm_end
    c->hs_exit = hs3;
    if (++c->hs_n % 200 == 0) {
      fprintf(stderr, "[tloam host stamps] per frame over 200: caller %.2f  begin %.2f (first launch called at %.2f, issued at %.2f)  "
                      "loop-without-wait %.2f  wait %.2f  end %.2f us\n",
              c->hs[0] / 200, c->hs[1] / 200, c->hs[5] / 200, c->hs[6] / 200, c->hs[2] / 200, c->hs[3] / 200, c->hs[4] / 200);
      for (int i = 0; i < 8; ++i) c->hs[i] = 0.0;
    }
  }
  if (rc == TLOAM_E_HIP) return rerun_after_scan_fault(scan_fault, rc);
  if (rc != TLOAM_OK) return rc;
  if (scan_xyz && n_scan > 0) {  // :1126-1128 out_result_.scan_cloud->Transform(curr_frame_pose)
    HIPC(c, c->misc.reserve(3 * n_scan));
    HIPC(c, hipMemcpyAsync(c->misc.p, scan_xyz, sizeof(double) * 3 * n_scan, hipMemcpyHostToDevice, c->stream));
    launch_transform_cloud(c->misc.p, n_scan, result, c->stream);
    HIPC(c, hipMemcpyAsync(scan_xyz, c->misc.p, sizeof(double) * 3 * n_scan, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
  }
  return weight_violation ? TLOAM_E_WEIGHT_RANGE : TLOAM_OK;
}

}  // extern "C"
