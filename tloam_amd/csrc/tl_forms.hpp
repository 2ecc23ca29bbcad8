// tl_forms.hpp -- the launch forms of a scanMatching frame, decided by one function (DESIGN.md section 5 has the table).
// Host only, plain C++17, no HIP: tests/host/frame_forms_main.cpp includes it alone.  The driver (tl_api_match.hip) fills a
// FormsIn from the context, keeps decide_forms' answer in tloam_ctx::forms and switches on it; nothing else combines knobs, rank
// layout and sizes.  The size limits the decision rests on are the constants below; the kernel files take them from here.
#pragma once

namespace tl {

// ---- the size limits -----------------------------------------------------------------------------------------------
#ifndef TLOAM_K1_QUAD_LIMIT
#define TLOAM_K1_QUAD_LIMIT 131072
#endif
#ifndef TLOAM_K1_WIDE_LIMIT
#define TLOAM_K1_WIDE_LIMIT 16384
#endif
constexpr int kQuadLimit = TLOAM_K1_QUAD_LIMIT;   // at most this many queries: four lanes per query (latency-bound regime); more:
                                                  // a thread per query, the size class of the direct set
constexpr int kWideLimit = TLOAM_K1_WIDE_LIMIT;   // at most this many: sixteen lanes per query (one row of the 27 cells per lane)
constexpr int kPrepareSmallLimit = 16384;         // source slots k_prepare_small (one block) scans, caps and compacts
constexpr int kFinishSmallLimit = 16384;          // segment capacity one 1024-thread block finishes (k_weights_finish_small)
constexpr int kFlagbStride = 4096;                // SlotView::flagb, flag bytes per kind: 64 lanes x 64 slots
constexpr int kTaggedRows = 16;                   // blocks whose rows are their own flag (tl_gn.hip): the one-launch Solve's grid
constexpr int kMaxOuterInLaunch = 8;              // outer iterations a one-launch Solve can finish (SolveFinish)
constexpr int kResultSlots = 8;                   // pinned result slots: outer iterations the device-driven loop plans for

// ---- what the decision may look at ---------------------------------------------------------------------------------
struct FormsIn {
  int nranks = 1, loopback = 0, mailbox = 0;   // rank layout; the exchange is the mailbox (else a collective: RCCL, callback)
  int device_cus = 0;
  // the knobs (environment, read once at create; no_persistent_solve is also set by the fall-back after a hand-over timed out)
  int no_persistent_solve = 0, no_direct_set = 0, no_device_loop = 0, no_build_reuse = 0, fused_large = 0, no_qbin_ride = 0;
  int factor_num = 4, max_iterations = 0;
  long long maxnum[4] = {0, 0, 0, 0}, n_src[4] = {0, 0, 0, 0}, n_tgt[4] = {0, 0, 0, 0};
  int has_grid[4] = {1, 1, 1, 1};   // the kind's target cloud has a search grid (known once the grids are built)
  // the sweep plan (k3_plan) and the capacities it was made from
  int k3_grid = 1, k3_single = 0;
  long long seg_cap[4] = {0, 0, 0, 0};
};

// ---- the forms: one enum per decision of the driver ------------------------------------------------------------------
enum class SetForm { COMPACT, DIRECT };
enum class PrepareForm {
  NONE,       // direct set: the search writes the rows
  IN_SOLVE,   // flag bytes (SlotView::flagb): a Solve launch that is handed a SolvePrep prepares the set itself
  SMALL,      // k_prepare_small
  TILES,      // tile scan, k_compact adds the tiles' offsets
  FULL        // full scan, rank counts + exchange when sharded, k_compact, k_refresh
};
enum class SolveForm {
  PERSISTENT,           // k_solve_all
  FUSED_LARGE,          // k3_sweep_step
  SHARDED_MBOX,         // fused sweep + post, gather + step
  SHARDED_COLLECTIVE,   // fused sweep, all-reduce, step
  SMALL_STEP,           // k_sweep_step_small
  SWEEP_REDUCE          // k3_accumulate + k_reduce_and_step
};
enum class FinishForm {
  DIRECT,    // the direct finish
  SMALL,     // k_weights_finish_small
  LARGE,     // k_weights + k_outer_finish
  SHARDED    // ... + exchange + k_outer_publish
};
enum class RideForm { NO, ON_SEARCH_SMALL, ON_SEARCH_LARGE, IN_SOLVE };   // k_build_finish_small / _large, SolveFinish
enum class LoopForm { DEVICE, HOST };

struct FrameForms {
  SetForm set = SetForm::COMPACT;
  PrepareForm prepare = PrepareForm::FULL;
  SolveForm solve = SolveForm::SWEEP_REDUCE;
  FinishForm finish = FinishForm::LARGE;        // the finish as a launch of its own
  RideForm finish_rides = RideForm::NO;         // where the device loop puts the finish of every iteration but the last
  LoopForm loop = LoopForm::HOST;               // who drives tloam_scan_match's outer loop
  bool qbin_ride = false;                       // the query sort's first pass may ride on the grid build
};

inline FrameForms decide_forms(const FormsIn& in) {
  FrameForms f;
  const bool one_rank = in.nranks == 1 && !in.loopback;   // else the sharded forms run (a loop-back exchanges with itself)
  long long n_slots = 0, cap_sum = 0;
  bool uncapped = true, grids = true, flag_bytes = true;
  for (int k = 0; k < 4; ++k) {
    n_slots += in.n_src[k];
    cap_sum += in.seg_cap[k];
    uncapped = uncapped && in.n_src[k] <= in.maxnum[k] && in.n_tgt[k] != 0;
    grids = grids && in.has_grid[k];
    flag_bytes = flag_bytes && in.n_src[k] <= kFlagbStride;
  }
  const bool prepare_small = one_rank && n_slots <= kPrepareSmallLimit;
  const bool finish_small = one_rank && cap_sum <= kFinishSmallLimit;

  // The Solve.  fused_large: one GN iteration is one launch whatever the size of the set; sharded, only the mailbox can do that
  // (it also posts, gathers and advances) -- RCCL / callback contexts keep sweep | collective | step: the host enqueues the collective.
  if (one_rank && in.k3_single && !in.no_persistent_solve && in.k3_grid <= kTaggedRows && in.k3_grid <= in.device_cus)
    f.solve = SolveForm::PERSISTENT;
  else if (in.fused_large && (one_rank ? !in.k3_single : in.mailbox != 0))
    f.solve = SolveForm::FUSED_LARGE;
  else if (!one_rank)
    f.solve = in.mailbox ? SolveForm::SHARDED_MBOX : SolveForm::SHARDED_COLLECTIVE;
  else
    f.solve = in.k3_single ? SolveForm::SMALL_STEP : SolveForm::SWEEP_REDUCE;

  // The direct set: one rank, searched one thread per query, all four builders running, no cap that could bind -- a kind's cap >=
  // its source points ("first N valid in index order", registration.cpp:448 / :538 / :592 / :735, then selects everything valid,
  // whatever the order) -- and a search grid for every kind (the rows ARE the sorted query order).  Everything else compacts.
  const bool direct = !in.no_direct_set && one_rank && in.factor_num == 4 && n_slots > kQuadLimit && uncapped && grids;
  f.set = direct ? SetForm::DIRECT : SetForm::COMPACT;
  f.prepare = direct                                                        ? PrepareForm::NONE
              : (f.solve == SolveForm::PERSISTENT && prepare_small && flag_bytes) ? PrepareForm::IN_SOLVE
              : prepare_small                                               ? PrepareForm::SMALL
              : one_rank                                                    ? PrepareForm::TILES
                                                                            : PrepareForm::FULL;
  f.finish = direct ? FinishForm::DIRECT : finish_small ? FinishForm::SMALL : one_rank ? FinishForm::LARGE : FinishForm::SHARDED;

  // device-driven outer loop where the stepwise machinery is not asked for: one rank, the planned iterations fit the result
  // slots, no development knob that needs the host between iterations
  const bool device_loop = one_rank && in.max_iterations >= 1 && in.max_iterations <= kResultSlots && !in.no_build_reuse && !in.no_device_loop;
  f.loop = device_loop ? LoopForm::DEVICE : LoopForm::HOST;
  if (device_loop) {
    if (f.prepare == PrepareForm::IN_SOLVE && finish_small && in.max_iterations <= kMaxOuterInLaunch)
      f.finish_rides = RideForm::IN_SOLVE;
    else if (prepare_small && finish_small && n_slots > 0 && n_slots <= kWideLimit)
      f.finish_rides = RideForm::ON_SEARCH_SMALL;
    else if (one_rank && !finish_small && n_slots > kQuadLimit)
      f.finish_rides = RideForm::ON_SEARCH_LARGE;
  }
  f.qbin_ride = one_rank && !in.no_qbin_ride && n_slots > kQuadLimit;
  return f;
}

}  // namespace tl
