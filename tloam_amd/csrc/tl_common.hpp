// tl_common.hpp -- shared device-side data structures of the MI355X T-LOAM pose-optimisation path.
//
// HBM layout (all fp64 SoA, one array per component, 256-B aligned, sized for 288 GB parts):
//   source clouds   sx/sy/sz[k][n_src_local], GNC weights w_src[k][n]      (one slot per source point)
//   target clouds   tx/ty/tz[k][n_tgt] (as given) + cell-sorted packed copy gp[k] (x,y,z,idx) + cell table
//   raw records     per source slot: a(3) b(3) d + flags        (written by the builder, K1+K2)
//   compact set     one SoA segment per kind: idx, px py pz, ax ay az, [bx by bz], [d], w, cost
//                   (streamed by K3; cost written back)
//   partials        [gridDim][32] per-block sums of H(21) g(6) cost(1)
//   GnState         the Ceres-minimiser / dogleg state machine + pose, device resident
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tloam_hip.h"
#include "tl_forms.hpp"
#include "tl_grid_plan.hpp"
#include "tl_se3.hpp"

namespace tl {

constexpr int kKinds = 4;
static_assert(kKinds == kGridKinds, "tl_grid_plan.hpp plans one grid per kind");
constexpr int kAccN = 28;        // 21 upper-triangular H + 6 g + 1 cost
constexpr int kAccStride = 32;   // padded row of the partials buffer
constexpr int kReduceBuf = 48;   // the all-reduced buffer: 28 used + per-kind tail
constexpr int kChunk = 128;      // correspondences per wave-chunk in K3 (64 lanes x 2)
constexpr int kMaxK = 8;         // max neighbours of tloam_knn
constexpr int kMaxRanks = 16;    // ranks one frame can be sharded over (rank_counts rows, mailbox slots); a node has 8 GPUs

// residual type of a kind (registration.cpp:981-992 builder -> cost functor)
__host__ __device__ inline int res_type_of_kind(int kind) {
  return kind == TLOAM_KIND_EDGE ? TLOAM_RES_LINE : (kind == TLOAM_KIND_SPHERE ? TLOAM_RES_POINT : TLOAM_RES_PLANE);
}

// ---- uniform grid over a target cloud (the device stand-in for KDTreeFlann) -----------------
struct GridView {
  const double4* gp;  // cell-sorted targets, packed (x, y, z, original index as integer bits): ONE 32-byte
                      // record per candidate, so a cell's points share cache lines
  const int* cell_start;  // ncell + 1
  double org[3];
  double inv_cell;    // 1 / cell
  double cell;
  int dim[3];
  int n;
};

// ---- compact correspondence set: one SoA segment per kind ------------------------------------
// stream order inside a kind's buffer (stream s starts at base + s * stride doubles)
enum SegStream : int { SS_PX = 0, SS_PY, SS_PZ, SS_AX, SS_AY, SS_AZ, SS_W, SS_D, SS_BX, SS_BY, SS_BZ, SS_COST, SS_W2, kSegStreams };
// (SS_W2: the second weight stream of a DIRECT set -- see DirectSet below; unused by compact sets)
struct CorrSeg {
  int* idx;                 // global source index of each correspondence
  double *px, *py, *pz;     // source point (sensor frame)
  double *ax, *ay, *az;     // plane normal | line point a | target point
  double *bx, *by, *bz;     // line point b (edge only, else null)
  double* d;                // plane offset (planar/ground only, else null)
  double* w;                // TLS weight captured at build time
  double* cost;             // side channel (`mutable double* cost`, registration.hpp:51,76,96)
  int cap;                  // capacity (multiple of kChunk)
  int stride;               // doubles between consecutive streams of the kind's buffer (SegStream order)
};
struct CorrView {
  CorrSeg k[kKinds];
  const int* seg_n;         // DEVICE: number of valid entries per kind [4]
};

// ---- the DIRECT factor set of large frames (round 6) ------------------------------------------------------------------------
// Frames searched one thread per query (> 131072 source points), on one rank, with every kind active and caps that cannot bind
// (a kind's cap >= its source points: the 1 M-class frames) do not compact at all.  The search processes its queries in the
// TILE-SORTED order of the frame's query sort; ROW r of kind k's segment IS the query at sorted position slot_off[k] + r, for the
// whole frame, and the search writes the factor's geometry straight into that row (coalesced: consecutive lanes are consecutive
// rows).  A query without a factor leaves a HOLE: a row that adds exact zeros to every sum and whose side-channel cost is exactly
// 0 -- plane n = 0, d = 0 (r = 0, J = 0 whatever the weight); line a = b = 0 (the sweep takes 1 / |a - b| as 0); point q.x = NaN
// (the sweep takes weight and q.x as 0) -- so the sweep and the weight update run over the rows as they are, ~10 % of them holes.
//   p, idx     written by the frame's first search (the rows never move); idx[r] = the source index, ~index (negative) on a hole:
//              what the finish counts the factors by and the getters filter on
//   a, b, d    written by every search
//   w          TWO streams: the Solve of outer iteration k reads stream k & 1 -- the weights "captured by value at construction"
//              (registration.hpp:51,76,96) --, its finish writes every row of stream (k + 1) & 1 (updateWeight, registration.cpp:
//              858-876; a row it leaves alone is copied).  No capture pass, no per-slot weight array
//   cost       written by every sweep (every row: a hole's is 0), read by the finish
// What is gone: the flag scan, the compaction (~45 us per outer iteration of the 1 M frame) and the raw records.  What it costs:
// the holes in the sweep (+10 % rows).  The sums run over the rows in tile order instead of index order: same factors, another
// rounding of the last bits (the parity bar on the pose is 1e-9).  Frames whose caps CAN bind, sharded frames and everything
// smaller keep the compact set: "first N valid in index order" (registration.cpp:448, :538, :592, :735) needs the index order.
struct DirectSet {
  int on;          // 0: raw records + flags (compacted afterwards)
  int first;       // the frame's first search: also writes p, idx, and weight stream 0 = 1 (registration.cpp:931-949)
  int set_x_build; // the launch records the pose the set is built at (GnState::x_build); 0 when a finish in the SAME launch does
  // factors per kind found by every one-wave block of THIS search, [blocks][4]: what n_corr is added up from -- by the finish of
  // the outer iteration the set is solved in, not from the rows (the NEXT search may be rewriting them beside that finish).
  // Two buffers, by the parity of the outer iteration the search belongs to.
  int* blk_cnt;
  // The ROW of a sorted position.  The frame's query sort places the queries of one bin (a cell, or a tile) in the ARRIVAL order of
  // an atomic: two runs over the same frame permute them, and a factor set whose rows followed the sorted positions would add its
  // sums up in another order every time (same factors, other last bits).  The rows therefore take the bins' queries in SLOT order:
  // the frame's first search works out, per query, how many queries of its bin have a lower slot (bins hold one or two queries on
  // average; beyond kDirectBinMax the arrival order stands) and keeps the row of every sorted position for the later searches.
  // Run to run the same rows, the same sums, the same bits -- as with a compact set.
  const int* tile_of_slot;
  const unsigned long long* tile_scan;
  int* row_of_pos;
};
constexpr int kDirectBinMax = 1024;

// ---- per-source-slot arrays of one scan_match (concatenated over kinds) ----------------------
struct SlotView {
  const double *sx, *sy, *sz;  // source points (sensor frame)
  double* w_src;               // GNC weights
  // raw builder output: one 64-byte record per slot (a[3], b[3], d, pad) -- K1 writes it with four 16-byte
  // stores into ONE line (the seven separate SoA arrays cost a 32-byte sector per 8-byte scattered store:
  // PMC WRITE_SIZE 269 MB per 1 M queries for 64 MB of records)
  double* raw;
  unsigned long long* flags;   // low 32: counted, high 32: valid (then scanned in place -> exclusive prefix)
  unsigned long long* scan;    // exclusive scan of flags
  // the same two bits per slot as ONE BYTE (bit 0 valid, bit 1 counted) at [kind * kFlagbStride + slot-in-kind], or null:
  // what the one-launch Solve reads when it compacts the factor set itself (k_solve_all, SolvePrep) -- a lane takes in
  // 64 slots with four 16-byte loads.  Only for frames whose kinds have at most kFlagbStride source points each.
  unsigned char* flagb;
  int slot_off[kKinds + 1];    // concatenated slot ranges per kind
  int src_lo[kKinds];          // global index of local slot 0 (sharded contexts)
};

// ---- Ceres TrustRegionMinimizer + DoglegStrategy state -----------------
enum GnPhase : int { PH_ITER0 = 0, PH_CAND = 1 };

struct GnState {
  // ---- host-visible prefix: what the host reads after an outer iteration / a Solve.  The finish kernels
  //      mirror exactly these kMirrorWords 8-byte words (two 64-byte PCIe writes) and then host_seq.
  double x[6];        // accepted iterate == `parameters` (registration.hpp:328)
  double x_cost;
  double kind_cost[kKinds];
  int n_corr[kKinds];
  // counters (whole scan_match)
  int gn_evaluations, gn_iterations, accepted_steps;
  int gn_sweeps;      // sweeps actually consumed (<= gn_evaluations, see gn_consume_wave)
  int bad_weights;
  int incomplete;     // set by the gated weight/finish kernels when the Solve had not terminated yet
  unsigned long long host_seq;  // sequence number of the host mirror (see HostMirror); right after the prefix
  // ---- device-only from here
  double x_cand[6];   // candidate evaluated by the sweep in flight
  Pose T_eval;        // exp(point being swept)
  Rt Rt_eval;         // the same as rotation matrix + translation (what K3 streams against)
  Pose T_cur;         // exp(x), used by the builders
  // minimiser
  double x_norm, gmax, model_cost_change;
  double g[6], H[36]; // robustified normal equations at x
  double S[6];        // Jacobi scaling (fixed at iteration 0 of each Solve)
  // dogleg (DoglegStrategy).  Kept in the form the step's hot path needs (tl_step.hpp): D = the clamped diagonal
  // itself (min_diagonal_^2 .. max_diagonal_^2, i.e. Ceres' diagonal_ SQUARED), gn = the Gauss-Newton step in the
  // Jacobi-scaled space (-y of (Hs + mu D) y = gs, i.e. gauss_newton_step_ / diagonal_), gn_norm = | gauss_newton_step_ |
  double radius, mu, alpha, step_norm, gn_norm;
  double D[6], grad[6], gn[6], U[12], sg[2], sB[4];
  int reuse, subspace_1d;
  int cand_gn;        // the candidate in the state (x_cand, T_eval, model_cost_change) is the Gauss-Newton step of the dogleg data above
  int phase, iteration, invalid, step_successful, done;
  int no_eval_reuse;  // development knob (TLOAM_NO_EVAL_REUSE): every evaluation runs its own sweep
  int comm_error;     // a mailbox exchange timed out (sharded contexts): published to the host as incomplete = 3
  // ---- outer GNC loop driven from the device (tloam_scan_match enqueues ALL outer iterations at once and waits once)
  double x_build[6];  // `parameters` the compact set was built at (written by the compaction)
  double prev_planar; // planar side-channel cost sum of the previous outer iteration (registration.cpp:1108), +inf at start
  int stop;           // 0 running | 1 the loop has ended (plateau break :1108 or max_iterations) | 2 Solve out of budget
  int run_build;      // gates of the NEXT outer iteration's launches: builders + scan + compaction run iff the pose moved,
  int run_refresh;    // the refresh iff it did not (see k_refresh); both 0 once the loop has ended
  int spec_build;     // written by the minimiser step: 1 iff the Solve has terminated at a pose other than x_build -- the gate of
                      // a correspondence search that runs CONCURRENTLY with the finish of that Solve (k_build_finish_small)
  int next_outer;     // device-driven loop: the outer iteration to run next (advanced by every finish).  A one-launch Solve that
                      // also finishes its iteration may run the FOLLOWING ones too (SolveFinish); the launches enqueued for
                      // those find their iteration taken and return
  int fin_valid;      // fin_sum / fin_bad hold the finish sums of the Solve that has just ended (k_solve_all); consumed by the finish
  double fin_sum[kKinds], fin_bad;
  double dbg[12];     // LAST: phase time stamps of the step kernel (TLOAM_STEP_PROFILE builds only)
};
constexpr int kMirrorWords = 16;  // x[6], x_cost, kind_cost[4], n_corr[4] (2 words), 6 ints (3 words)
static_assert(offsetof(GnState, host_seq) == kMirrorWords * 8, "host-visible prefix of GnState");
// End of an outer iteration: the finish kernel copies the host-visible prefix of the state into pinned host
// memory and then stores the sequence number, so the host reads the result by polling one word instead of paying a
// copy kernel plus a stream synchronisation per outer iteration (registration.cpp:1108 is a host decision).
// out == nullptr: off.
// The slot is written WITHOUT any fence: it is three 64-byte segments, each carrying seven words of the prefix and,
// last, check_mix(sequence number) XOR seg_word of each of those seven words; one wave stores all 24 words with one instruction.  In
// practice every segment leaves the GPU as one aligned 64-byte write (a full cache line for the host); the host does
// not rely on that: it accepts a segment only when the check word agrees with the payload it reads
// (tlh::wait_segment), so a torn segment reads as "not there yet".  (A system-scope release would first write back
// every dirty L2 line of the kernel, ~2 us; writing the number behind the words with only a wave-level wait is NOT
// safe: the two cache lines travel through different L2 channels.)
struct MirrorSlot {
  unsigned long long w[24];
};
// The check word of every 64-byte hand-over segment (result slots, block rows, pose broadcasts, finish sums, submap sizes) is
// check_mix(number) XOR the seven payload words.  Consecutive numbers differ in a few low bits; multiplied by an odd 64-bit
// constant they differ in about half of all bits, so a segment whose check word is still the old one and of which ONE payload
// word has arrived can only pass if that word changed by exactly that 64-bit pattern -- not by a counter step or a
// last-mantissa-bit change.  Zeroed memory checks for number 0 only; numbers start at 1.
__host__ __device__ inline unsigned long long check_mix(unsigned long long number) { return number * 0x9E3779B97F4A7C15ull; }
// The segments the HOST reads (result slots, submap sizes) enter their check word through seg_word: position-dependent and
// non-linear in the word.  With a plain XOR of the payload a segment whose check word had arrived and whose payload had not
// passed whenever the old and the new payload XORed alike -- (58, 58) after (0, 0), (459, 16) after (458, 17): the sizes of a
// submap update read back as those of the update before in 2-4 % of contexts (round 5, tests/tools/stress_rows.py).
__host__ __device__ inline unsigned long long seg_word(unsigned long long w, int pos) {
  unsigned long long v = (w + 0x9E3779B97F4A7C15ull * (unsigned long long)(pos + 1)) * 0xBF58476D1CE4E5B9ull;
  return v ^ (v >> 29);
}
struct HostMirror {
  MirrorSlot* out;
  unsigned long long seq;
};
// status of an outer iteration as the host reads it in GnState.incomplete
// OS_NEEDS_HOST (a flag on top of the status, result slot only): the launch that finished this iteration inside the Solve
// has ended because the pose moved -- the loop goes on with a correspondence search, which the host enqueues unless it
// already has
// OS_SET_STALE (a flag like OS_NEEDS_HOST, direct sets only): the loop ended in the launch whose search had already run on the
// Solve's own verdict -- the rows hold the geometry of a set that was never solved; the host rebuilds them before anybody reads
enum OuterStatus : int { OS_OK = 0, OS_INCOMPLETE = 1, OS_COMM_ERROR = 3, OS_PLATEAU = 4, OS_SKIPPED = 8, OS_NEEDS_HOST = 16, OS_SET_STALE = 32 };
// device-driven loop control handed to the finish kernels (fast == 0: the host decides, as in the stepwise API)
struct OuterCtl {
  double cost_threshold;  // registration.cpp:1108
  int fast;               // 1: evaluate the plateau test / pose comparison on the device and set the gates
  int last;               // this is outer iteration max_iterations - 1
  int direct;             // direct set: a finish that sends the loop into a rebuild records the pose of that build (x_build) itself
                          // -- the search that does the rebuild runs beside it in the same launch -- and flags a stale set
};

// ---- one-shot peer exchange of a sharded context ("mailbox") -------------
// Every rank owns a small buffer in fine-grained (uncached) device memory that its peers map through HIP IPC:
//   [2 parities][kMaxRanks writers][kMboxSlot doubles]   (<= 64 values ... , word kMboxSlot-1 = the exchange id)
// Exchange number id (1, 2, ...; counted on the device, identically on every rank): rank r stores its values
// into slot [id & 1][r] of EVERY rank's buffer over xGMI, fences at system scope, stores the id; a reader waits for
// the id in all nranks slots of its OWN buffer and adds the rows in rank order (deterministic, identical on all
// ranks).  Two parities suffice: a rank can only post id + 2 after it has gathered id + 1, which every rank posts
// only after it has finished gathering id.
constexpr int kMboxSlot = 80;   // up to 64 values + padding; the last word carries the exchange id
struct MboxView {
  double* peer[kMaxRanks];        // device-visible address of every rank's buffer (peer[rank] = the local one)
  unsigned long long* ctr;        // [0] exchanges completed so far (device-resident, survives frames); [1] error flag
  int rank, nranks;
};
constexpr size_t kMboxDoubles = (size_t)2 * kMaxRanks * kMboxSlot;

// ---- host-callable launchers (defined in tl_nn.hip / tl_gn.hip) ------------------------------
struct ScanTemp;  // opaque

// AoS double[3] -> SoA, for a sub-range
void launch_aos_to_soa(const double* aos, size_t n, double* x, double* y, double* z, hipStream_t s);

// exclusive scan of u64 values (tl_scan.hip); tmp must hold scan_scratch_elems(n) u64 (tl_grid_plan.hpp)
// gate != nullptr: a device flag; the launches do nothing where it reads 0
void launch_exclusive_scan_u64(const unsigned long long* in, unsigned long long* out, size_t n,
                               unsigned long long* tmp, hipStream_t s, const int* gate = nullptr);

// grid build for all four kinds at once (one launch per phase, blockIdx.y = kind): bbox (finished on the
// host), histogram over the CONCATENATED cell tables, one exclusive scan, finalize, scatter
struct GridSet {
  const double* tx[kKinds];
  const double* ty[kKinds];
  const double* tz[kKinds];
  int n[kKinds];
  int tgt_off[kKinds];          // offset of the kind's points in the concatenated point arrays
  long long cell_base[kKinds];  // offset of the kind's cells in the concatenated cell arrays (cell_start: + kind in the packed
                                // layout -- GridPlan::Kind::start_base, tl_grid_plan.hpp)
  long long ncell[kKinds];
  double org[kKinds][3];
  double inv_cell[kKinds];
  int dim[kKinds][3];
};
struct IngestArgs {   // k_ingest_targets: the four target clouds as uploaded (AoS) and where their SoA copies go
  const double* aos[kKinds];
  double *x[kKinds], *y[kKinds], *z[kKinds];
  int n[kKinds];
};
void launch_ingest_targets(const IngestArgs& A, double* bbox_rows /*[kind][64][6]*/, hipStream_t s);
struct FrameInit {
  const double* src_aos[kKinds];
  int direct;         // direct set: seg_n[k] = the kind's rows (= its source points) for the whole frame instead of 0
  int slot_off[kKinds + 1];
  double x[6];
  int no_eval_reuse;  // development knob, copied into the state
  unsigned long long* tile_cnt;  // query-tile histogram of the first builder pass, zeroed here (n_tile_cnt entries)
  int n_tile_cnt;
};
struct FrameInitBufs {
  double *sx, *sy, *sz, *w_src;
  unsigned long long* flags;
  GnState* st;
  int* seg_n;
};
// start of a scan_match folded into the first launch of the grid build (k_grid_count_all): `on` = 0 leaves the launch
// as it was; `consumed` tells the caller whether a launch carried it (no targets at all = no grid launch)
struct BuildParams {
  double radius[kKinds];
  int maxnum[kKinds];
  int active[kKinds];
  double edge_dir_thres;
};
// The first pass of the frame's query sort (k_query_bin: the bin of every source point under the predicted pose, one returning
// atomic each) needs the grids' DIMENSIONS, not the grids: on the 1 M-class frames it rides on the last launch of the grid build
// (the scatter of the targets into their cells -- writes against atomics) as one more row of blocks instead of following it.
struct QueryBinRide {
  SlotView sv;
  BuildParams bp;
  const GnState* st;
  int* tile_of_slot;
  int* rank_in_tile;
  unsigned long long* tile_cnt;
};
struct FrameInitHook {
  FrameInit fi;
  FrameInitBufs b;
  int n_slots;
  bool consumed;
  // in: non-null = the caller wants the query binning to ride (it has filled sv / bp / st); out: qbin_done
  QueryBinRide* qbin;
  bool qbin_done;
};
#if defined(__HIPCC__)
// start-of-Solve values of the minimiser (Ceres defaults: initial_trust_region_radius 1e4, min_mu 1e-8);
// the sweep point is the current pose
__device__ __forceinline__ void arm_solver(GnState& s) {
  s.radius = 1e4;
  s.mu = 1e-8;
  s.reuse = 0;
  s.cand_gn = 0;
  s.subspace_1d = 0;
  s.phase = PH_ITER0;
  s.iteration = 0;
  s.invalid = 0;
  s.step_successful = 1;
  s.done = 0;
  s.gmax = 1e300;
  s.T_eval = s.T_cur;
  s.Rt_eval = to_rt(s.T_cur);
}
// Start of a scan_match: de-interleave the four source clouds into the concatenated SoA slot arrays, set the GNC
// weights to 1 and the flag-scan terminator to 0 (registration.cpp:931-949); block 0 also zeroes the minimiser state,
// installs `parameters` = log(predict) (:881) and arms the first Solve.  Called by `nblocks` blocks of 256 threads.
__device__ __forceinline__ void frame_init_body(const FrameInit& fi, const FrameInitBufs& b, int block, int nblocks) {
  const int n = fi.slot_off[kKinds];
  for (int slot = block * 256 + (int)threadIdx.x; slot < n; slot += nblocks * 256) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < kKinds; ++q) k += (slot >= fi.slot_off[q]) ? 1 : 0;
    const double* a = fi.src_aos[k] + 3 * (size_t)(slot - fi.slot_off[k]);
    b.sx[slot] = a[0]; b.sy[slot] = a[1]; b.sz[slot] = a[2];
    b.w_src[slot] = 1.0;
  }
  for (int i = block * 256 + (int)threadIdx.x; i < fi.n_tile_cnt; i += nblocks * 256) fi.tile_cnt[i] = 0ull;
  if (block == 0) {
    constexpr int kWords = (int)(sizeof(GnState) / sizeof(double));
    for (int i = threadIdx.x; i < kWords; i += 256) reinterpret_cast<double*>(b.st)[i] = 0.0;
    if (threadIdx.x < 8)
      b.seg_n[threadIdx.x] = (fi.direct && threadIdx.x < kKinds) ? fi.slot_off[threadIdx.x + 1] - fi.slot_off[threadIdx.x] : 0;
    if (threadIdx.x == 0) b.flags[n] = 0ull;
    __syncthreads();
    if (threadIdx.x == 0) {
      GnState* st = b.st;
#pragma unroll
      for (int i = 0; i < 6; ++i) st->x[i] = fi.x[i];
      st->T_cur = se3_exp(st->x);
      st->no_eval_reuse = fi.no_eval_reuse;
      st->prev_planar = __builtin_inf();   // registration.cpp:952-959
      st->run_build = 1;                   // the first outer iteration always builds
      arm_solver(*st);
    }
  }
}
#endif
void launch_frame_init(const FrameInit& fi, const FrameInitBufs& b, hipStream_t s);
void launch_bbox_all(const GridSet& gs, double* out /*[4][64][6], device or pinned host*/, hipStream_t s);
// T = the histogram's element: unsigned on the frame-size path, unsigned long long where the u64 scans follow
template <typename T>
void launch_grid_count_all(const GridSet& gs, T* cell_cnt, int* cell_of_pt, int* rank_of_pt, hipStream_t s,
                           const FrameInitHook* frame = nullptr);
void launch_grid_finalize_all(const GridSet& gs, const unsigned long long* cell_scan, int* cell_start,
                              unsigned long long* cell_cnt /* re-zeroed */, hipStream_t s);
// medium-size scans (scan_path: TILES): tile-local scan only (returns the tile count, 0 = not applicable), the consumer adds the
// tiles' offsets itself
int scan_tiles_only(const unsigned long long* in, unsigned long long* out, size_t n, unsigned long long* totals, hipStream_t s,
                    const int* gate = nullptr);
// The frame-size grid build (GridScan::TILES: a padded table of more than 16 Ki entries and at most 1024 scan tiles): 32-bit
// histogram, tile-local scan that leaves the histogram empty again, then finalize + scatter in ONE launch -- three launches per
// build.  The table's layout differs from the other paths': kind k's ncell + 1 entries start at cell_base[k], a MULTIPLE OF 4,
// in the histogram, the scan and cell_start alike (n_tab = the padded total, a multiple of 4; totals: 1024 entries).
void launch_grid_scan_tiles(unsigned* cell_cnt /* re-zeroed */, unsigned* cell_scan, size_t n_tab, unsigned* totals, hipStream_t s);
void launch_grid_finalize_scatter_all(const GridSet& gs, const unsigned* cell_scan, const unsigned* totals, int tiles, long long n_tab,
                                      int* cell_start, const int* cell_of_pt, const int* rank_of_pt, double4* gp, hipStream_t s);
void launch_grid_scatter_all(const GridSet& gs, const int* cell_of_pt, const unsigned long long* cell_scan,
                             const int* rank_of_pt, double4* gp, hipStream_t s);
// large tables (more than 1024 scan tiles: the 1 M-class frames): ONE single-pass launch scans the histogram, writes cell_start
// and re-zeroes the histogram (no scan array), then the scatter -- count | scan + finalize | scatter.  ctl: scan_ctl_elems(n)
// words, zero when allocated (k_scan_1p, tl_scan.hip).  Only where every block of the launch is resident at once on THIS device
// (scan_path: SINGLE_PASS); fault: pinned host word the kernel raises if its bounded look-back times out
void launch_scan_counts_1p(const unsigned long long* in, unsigned long long* out, size_t n, unsigned long long* ctl, unsigned* fault,
                           hipStream_t s);
void launch_grid_scan_finalize_scatter_1p(const GridSet& gs, unsigned long long* cell_cnt, size_t ncells_plus_1, int* cell_start,
                                          unsigned long long* ctl, unsigned* fault, const int* cell_of_pt, const int* rank_of_pt, double4* gp,
                                          hipStream_t s, const QueryBinRide* qbin = nullptr, const GridView* views = nullptr);

// start-of-frame initialisation, one launch
// K1+K2: per source slot kNN + fit + gates -> raw records + flags
// scan1p_ctl: control words of the single-pass scan of the query-sort histogram (large frames; the caller has asked
// scan_path), or null: the multi-launch scan; scan1p_fault: see launch_scan_counts_1p
// direct_cv != null: the search writes the DIRECT set (DirectSet) -- st is then written (x_build) where ds.set_x_build says so
void launch_build(const SlotView& sv, const GridView grids[kKinds], const BuildParams& bp, GnState* st,
                  int* tile_of_slot, unsigned long long* tile_cnt, unsigned long long* tile_scan, int* tile_fill,
                  double4* qrec, unsigned long long* scan_tmp, bool rebin, hipStream_t s, const int* gate = nullptr,
                  unsigned long long* scan1p_ctl = nullptr, unsigned* scan1p_fault = nullptr, const CorrView* direct_cv = nullptr,
                  const DirectSet* ds = nullptr, bool binned = false);   // binned: the sort's first pass rode on the grid build
int build_tile_count(const GridView grids[kKinds], const int slot_off[kKinds + 1]);  // bins of the query counting sort (per kind: its tiles, or the cells of its tiles)
// cap + compaction (after the flag scan)
// refresh_gate != null: the launch also stands for the refresh alternative (see CompactArgs); tiles > 0: `sv.scan` holds
// tile-local scans and `totals` the tiles' totals (scan_tiles_only)
void launch_compact(const SlotView& sv, const CorrView& cv, const BuildParams& bp, int* seg_n,
                    const double* rank_counts, int rank, int nranks, GnState* st, hipStream_t s, const int* gate = nullptr,
                    const int* refresh_gate = nullptr, const unsigned long long* totals = nullptr, int tiles = 0);
void launch_rank_counts(const SlotView& sv, double* rank_counts, int rank, int nranks, hipStream_t s);
// same correspondences, new outer iteration: re-capture the weights, zero the side-channel slots
void launch_refresh(const SlotView& sv, const CorrView& cv, hipStream_t s, const int* gate = nullptr);
// small single-rank frames: flag scan + caps + compaction (run_build, or always if null) or refresh (run_refresh) in ONE launch
void launch_prepare_small(const SlotView& sv, const CorrView& cv, const BuildParams& bp, int* seg_n, GnState* st,
                          const int* run_build, const int* run_refresh, hipStream_t s);
// generic hybrid search (tloam_knn / fitness)
void launch_knn(const GridView& g, const double* qx, const double* qy, const double* qz, int nq,
                double radius, int k, int* out_idx, double* out_d2, int* out_cnt, hipStream_t s);
void launch_fitness(const GridView& g, const double* qx, const double* qy, const double* qz, int nq,
                    double radius, double* partial /*[blocks*2]*/, int blocks, hipStream_t s);

// ---- device-resident submap maintenance (tl_submap.hip; front_end.cpp:201-275) ----------------
// One Crop + VoxelDownSample launch sequence over up to TWO clouds stored back to back ("segments": the edge and
// the ground submap of an update -- same pipeline, different box and voxel size).  Points [0, n0) are segment 0,
// [n0, n) segment 1; the segment is part of the voxel key, so the segments never mix, and because the voxels are
// emitted in order of first occurrence segment 0's come out first.  One cloud: n0 == n.
struct VoxelJob {
  const double *x, *y, *z;   // input clouds, SoA, concatenated
  size_t n, n0;
  double lo[2][3], hi[2][3]; // crop boxes, inclusive (+-inf: no crop)
  double voxel[2];           // voxel sizes
  unsigned long long mask;   // hash-table capacity - 1 (power of two >= 2 n)
};
constexpr int kVoxLocal = 32;   // members of a voxel its leader orders in LDS (k_vox_emit, k_map_emit); a fuller voxel goes another way
struct VoxelWork {           // scratch, sized by the caller (see voxel_table_size)
  double* min_partial;       // [256][6], or [submap_front_rows][6] behind k_submap_front
  double* vmin;              // [2][3] voxel_min_bound per segment
  unsigned long long *keys, *cnt;   // [cap + 1]: the voxel keys, the head of every slot's member list
  int *slot_of_pt, *urank, *members;   // [n]: hash slot of a point (-1: none), the next member of its list, the heap sort's scratch
  unsigned long long* leader;          // [emit blocks + 1]: look-back words of k_vox_emit
  unsigned long long* leader_scan;     // [2] control words: blocks of k_vox_emit started so far, cursor of `members`
  int* overflow;             // set when a voxel index leaves [0, 2^21)
  unsigned long long* n_out; // [2] receives the sizes of the down-sampled clouds
  // != nullptr: the sizes, the overflow flag and host_seq are also stored into one 64-byte segment of pinned host memory
  // ([0] n_out[0], [1] n_out[1], [2] overflow, [7] host_seq) by ONE instruction of the last kernel -- the host polls the
  // number instead of paying two device-to-host copies and a stream synchronisation
  unsigned long long* host_seg;
  unsigned long long host_seq;
  double* out[2][3];         // (x, y, z) of the down-sampled cloud per segment
  // k_vox_emit's look-back scan: blocks take their places from blockIdx while the whole grid is resident on this device
  // (vox_emit_resident_blocks), from a start ticket otherwise; fault: pinned host word raised if the bounded look-back times out
  int use_ticket;
  unsigned* fault;
};
size_t voxel_table_size(size_t n);
int vox_emit_resident_blocks(int device_cus);   // blocks of k_vox_emit the device holds at once, with a margin (tl_submap.hip)
void launch_transform_to_soa2(const double* aos, size_t n, const double M[16], double* ax, double* ay, double* az,
                              double* bx, double* by, double* bz, hipStream_t s);
struct AssembleArgs {          // per segment: old submap cloud (SoA) followed by the new scan cloud (AoS, to transform)
  const double *ox[2], *oy[2], *oz[2];
  const double* aos[2];
  size_t n_old[2], n_new[2], base[2];
  double M[16];                // column-major pose
};
void launch_assemble(const AssembleArgs& A, double* wx, double* wy, double* wz, hipStream_t s);
int submap_front_ring_max();   // planar ring frames one launch_submap_front call takes
void launch_soa_to_aos(const double* x, const double* y, const double* z, size_t n, double* aos, hipStream_t s);
void launch_blit_doubles(const double* src_host_view, double* dst, size_t n, hipStream_t s);   // pinned host -> device by a kernel
void launch_crop_voxel(const VoxelJob& J, const VoxelWork& W, hipStream_t s, bool front_done = false);
// the front of a submap update in one launch (k_submap_front): planar ring transform + assembly of the edge / ground clouds +
// the crop + voxel job's table clear and min bound; launch_crop_voxel(front_done = true) follows
size_t submap_front_rows(size_t n_ring_max, size_t n_seg_max);
void launch_submap_front(int count, const double* const aos[], const size_t n[], const double* const poses[], const AssembleArgs& A,
                         const VoxelJob& J, const VoxelWork& W, double* px, double* py, double* pz, double* qx, double* qy, double* qz,
                         double* wx, double* wy, double* wz, hipStream_t s, int copy_frame = -1, double* copy_dst = nullptr);
// (copy_dst: frame `copy_frame`'s cloud is read from pinned host memory and copied to this device buffer on the way; every
//  AoS cloud the launch reads must start on a 16-byte boundary and may be read up to one double past its end)

// ---- the odometry frame (tl_odom.hip): index lists -> point rows, device to device -----------------
// One job: row i of the destination = source point idx2[idx1[i]] (a missing list is the identity), for i < min(*count, n).
// Coordinates at x[p * stride], y[p * stride], z[p * stride]: stride 3 with (x, y, z) = (base, base + 1, base + 2) is AoS,
// stride 1 with three arrays is SoA.  Indices outside [0, n1) / [0, src_n) are not followed (the row is left as it was).
struct GatherJob {
  const double *sx, *sy, *sz;
  double *dx, *dy, *dz;
  const int* idx1;
  const int* idx2;
  const int* count;   // device word: the list's length (nullptr: n)
  int n;              // rows the grid covers: an upper bound of the length, known to the host
  int n1, src_n;      // bounds of idx1's values (the length of idx2's list) and of the source point index
  int ss, ds;         // strides of source and destination, in doubles
};
constexpr int kGatherMaxJobs = 8;
struct GatherArgs { GatherJob j[kGatherMaxJobs]; };
void launch_gather_lists(const GatherArgs& A, int jobs, hipStream_t s);
// after launch_feat_select and a two-segment voxel job: ctl[0..6] = planar / sphere candidates, the lengths of the scan
// selections (the prefix of the ranked list extractPlanarSphere keeps, :178-190), the two voxel counts, the voxel overflow flag
struct OdomCountArgs {
  const unsigned long long* total;   // scan[n] of launch_feat_select: planar << 32 | sphere
  const double* ranked;              // FeatRankOut: planar flatness, then sphere flatness
  int planar_num, sphere_num;
  double planar_scan_thres, cvr_scan;
  const unsigned long long* vox_n;   // VoxelWork::n_out
  const int* vox_overflow;           // VoxelWork::overflow
  int* ctl;
};
void launch_odom_counts(const OdomCountArgs& A, hipStream_t s);

// ---- the global map of the odometry frame (tl_map.hip) ------------------------
// VoxelDownSample of one transformed scan whose voxels can hold hundreds of returns (1 m cells on a raw scan): the leader of a voxel
// (its smallest member) comes from an atomicMin, not from a walk of the member list; voxels of up to kVoxLocal members are
// averaged by their leader as in k_vox_emit, larger ones by a workgroup each, their members sorted by index in LDS
// Open3D TransformPoints: new = T * (x, y, z, 1), rows accumulated left to right; point = new.head<3>() / new(3).  Units that
// call it are compiled with -ffp-contract=off (the oracle's pc_transform rounds so)
__device__ __forceinline__ void map_transform_point(const double* M, double x, double y, double z, double* px, double* py,
                                                    double* pz) {
  double r[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) r[a] = ((M[a] * x + M[4 + a] * y) + M[8 + a] * z) + M[12 + a] * 1.0;
  *px = r[0] / r[3];
  *py = r[1] / r[3];
  *pz = r[2] / r[3];
}
struct MapFrontArgs {
  const double* aos;          // the raw scan, AoS
  size_t n;
  double M[16];               // column-major pose
};
struct MapVoxWork {
  double *x, *y, *z;          // the transformed scan, SoA (written by k_map_front)
  size_t n;
  double voxel;
  double lo, hi;              // box on every axis, inclusive: the finite doubles (a non-finite return is in no voxel)
  unsigned long long mask;    // hash-table capacity - 1 (voxel_table_size(n))
  double* min_partial;        // [blocks of k_map_front][3]
  double* vmin;               // [3] voxel_min_bound
  unsigned long long* keys;   // [mask + 1]
  int *head, *first, *count, *bigslot;   // [mask + 1]: member list head, smallest member, members, big-voxel number
  int *slot_of_pt, *next;     // [n]: hash slot of every point (-1: none), next member of its voxel's list
  int* members;               // [n]: the members of the big voxels, one piece per voxel
  unsigned long long* leader; // [emit blocks + 1]: look-back words of k_map_emit
  int* ctl;                   // [0] overflow, [1] ticket of k_map_front, [2] start tickets of k_map_emit, [3] big voxels, [4] their members
  int4* bigq;                 // [big_max]: (slot, output position, first member in `members`, members)
  int* bigfill;               // [big_max]
  int big_max;                // n / (kVoxLocal + 1) + 1
  double *ox, *oy, *oz;       // the means: the map at its current end
  unsigned long long* n_out;  // [1] voxels
  unsigned long long* host_seg;   // pinned: [0] voxels, [2] overflow, [7] check word (as VoxelWork::host_seg)
  unsigned long long host_seq;
  int use_ticket;
  unsigned* fault;
};
inline int map_big_max(size_t n) { return (int)(n / (kVoxLocal + 1) + 1); }
// front | insert | emit | scatter | big: no host synchronisation; the count reaches the host segment with k_map_emit
void launch_map_voxel(const MapFrontArgs& A, const MapVoxWork& W, hipStream_t s);
int map_emit_resident_blocks(int device_cus);
void launch_transform_aos(const double* aos, size_t n, const double M[16], double* out, hipStream_t s);

// ---- the merged voxel map of the odometry frame (tl_vmap.hip) ------------------------
// One grid for the whole run (origin, voxel fixed); per voxel an int64 count and int64 sums of the quantised offsets
// q = floor(frac(s) * 2^24 + 0.5), so that the sums are the same in any order.  A voxel's key packs i + 2^20 of each axis in
// 21 bits (bit 63 clear: ~0 marks a free slot).  Persistent state in id order (keys, N, Qx, Qy, Qz) and an open-addressing
// table slot -> id (-1: free) of load <= 1/2; a frame is staged in a table of its own and committed only once it is accepted
constexpr int kVmapBits = 20;                       // |i| < 2^20 on every axis
constexpr double kVmapQScale = 16777216.0;          // 2^24
struct VmapStageWork {
  const double *sx, *sy, *sz; // the transformed scan, SoA (the append map's k_map_front), or null: transform `aos` here
  const double* aos;          // the raw scan, AoS
  double M[16];               // column-major pose
  size_t n;
  double voxel, origin[3];
  // the frame's table [fmask + 1]
  unsigned long long fmask;
  unsigned long long* fkey;
  int* flead;                 // smallest point index of the voxel in this scan
  unsigned long long* fsum;   // [4][fmask + 1]: N, Qx, Qy, Qz of the frame
  int* fid;                   // the voxel's id (existing or new)
  int* slot_of_pt;            // [n]
  // the persistent table (read only here)
  unsigned long long pmask;
  const int* ptab;
  const unsigned long long* pkey;
  long long base;             // voxels before this frame: the first new id
  unsigned long long* look;   // [emit blocks + 1] look-back words of k_vmap_emit
  unsigned long long* ctl;    // [0] overflow, [1] finite points, [2] start tickets of k_vmap_emit, [3] fault, [4] new voxels
  unsigned long long* host_seg;   // pinned: [0] new voxels, [1] points, [2] overflow, [3] fault, [7] check word
  unsigned long long host_seq;
};
struct VmapTable {            // the persistent map
  unsigned long long pmask;
  int* ptab;
  unsigned long long* pkey;
  long long *pn, *pqx, *pqy, *pqz;
};
struct VmapTableView {        // the same, read only: what every stage on top of a map takes of it (VoxelRowStore::view)
  unsigned long long pmask;
  const int* ptab;
  const unsigned long long* pkey;
  const long long *pn, *pqx, *pqy, *pqz;
};
// What the stages on top of the closed map share of their arguments (tlh::map_grid_of fills the first):
struct MapGrid {              // the map a stage looks voxels up in: the grid, the rows' table, the voxels
  double voxel, origin[3];
  VmapTableView map;
  long long nv;
};
struct ScanAt {               // a live scan (or a ray-cast's segment ends) at a pose
  const double* pts;          // AoS, sensor frame
  long long n;
  double M[16];               // the pose, column-major, as it stands
};
// The carve gate: which voxels of the closed map count for a query.  One with N < min_count does not; with `gate` on, neither
// does one the carve saw through.  The only definition: the carved read (tl_carve.hip), the diff, the ray-cast and the free
// space's reads all ask it, so they agree about which voxels exist
struct CarveGate {
  const long long* miss;      // [nv] the carve's M (read when `gate`)
  long long min_count, min_miss;
  double miss_ratio;
  int gate;
  int reserved0;
  __device__ __forceinline__ bool seen_through(long long Mv, long long N) const {
    return Mv >= min_miss && (double)Mv > miss_ratio * (double)N;
  }
  // voxel `id` counts (N is read only when min_count > 1 or the gate is on, M only when the gate is on)
  __device__ __forceinline__ bool counts(const VmapTableView& map, int id) const {
    if (min_count > 1 || gate) {
      const long long N = map.pn[id];
      if (N < min_count) return false;
      if (gate && seen_through(miss[id], N)) return false;
    }
    return true;
  }
};
struct VmapReadArgs {
  VmapTableView map;
  double voxel, origin[3];
  size_t first, count;        // ids [first, first + count)
  double lo[3], hi[3];        // read_box: the box (inclusive) ...
  long long min_count;        // ... and the smallest N
  double* out_c;              // AoS centroids (compacted for read_box)
  long long* out_n;           // counts (may be null)
  unsigned long long* look;   // read_box: [blocks + 1] look-back words, zero before the launch
  unsigned long long* ctl;    // read_box: [0] start tickets, [1] fault, [2] selected voxels; zero before the launch
};
// clear | stage | emit: no host synchronisation; the new-voxel count reaches the host segment with k_vmap_emit
void launch_vmap_stage(const VmapStageWork& W, hipStream_t s);
// an accepted frame's staged voxels into the persistent map (the new ones keyed and entered in the table)
void launch_vmap_commit(const VmapStageWork& W, const VmapTable& T, hipStream_t s);
// the table of `T` (all slots free) rebuilt from the keys of ids [0, n)
// (n == 0 launches nothing, unless `even_empty`: a caller whose launch count must not depend on n)
void launch_vmap_rehash(const VmapTable& T, size_t n, hipStream_t s, bool even_empty = false);
void launch_vmap_read(const VmapReadArgs& A, hipStream_t s);
void launch_vmap_read_box(const VmapReadArgs& A, hipStream_t s);

// ---- the closed map: every keyframe's clouds under its own pose into one grid (tl_cmap.hip) ---------
// The voxel map's grid, key, q and centroid (above); its rows are read by k_vmap_read / k_vmap_box.  The input is a table of
// spans of the keyframe cloud arena in global point order -- keyframes ascending, a keyframe's selected clouds in slot order --
// and the K poses, both in HBM: a point finds its span from its global index, so a build is the same launches for any K
struct CmapSpan {
  long long off;              // first double of the span in the arena
  long long start;            // global index of its first point
  int kf;
  int reserved0;
};
struct SpanInput {            // what the build, the carve and the surfel pass read their points from
  const double* arena;
  const CmapSpan* span;       // [nspan + 1], spans of at least one point; span[nspan].start = n
  int nspan;
  int nkf;
  long long n;                // points of all spans
  const double* pose;         // [nkf][16] column-major
};
struct CmapWork {
  SpanInput in;
  int runs;                   // 1: runs of equal keys among a wave's consecutive lanes are summed before the table is touched
  int* kf_over;               // [in.nkf] 1: a finite point of the keyframe left the grid (k_cmap_flag): it adds nothing
  double voxel, origin[3];
  // the build table [fmask + 1]
  unsigned long long fmask;
  unsigned long long* fkey;
  unsigned long long* flead;  // smallest global index of the voxel
  unsigned long long* fsum;   // [4][fmask + 1]: N, Qx, Qy, Qz
  int* slot_of_pt;            // [n]
  unsigned long long* look;   // [emit blocks + 1] look-back words of k_cmap_emit
  unsigned long long* ctl;    // [0] distinct voxels (k_cmap_stage), [1] points added, [2] start tickets of k_cmap_emit, [3] fault,
                              // [4] voxels numbered (k_cmap_emit)
  VmapTable rows;             // the closed map (k_cmap_emit): a voxel beyond row_cap is numbered and not written
  long long row_cap;
};
// clear | flag | stage, then emit: no host synchronisation in either; each returns the launches it made
int launch_cmap_stage(const CmapWork& W, hipStream_t s);
int launch_cmap_emit(const CmapWork& W, hipStream_t s);

// ---- the closed map extended in place by later keyframes (tl_extend.hip).  The new keyframes' points are
// staged by the build's own clear | flag | stage (launch_cmap_stage over a span table of the new keyframes alone: a staging table
// and a slot per NEW point); the staged voxels are then numbered against the map's table and committed into its rows
struct StagedVoxels {         // the staging table as the stages after the commit read it
  unsigned long long fmask;
  const unsigned long long* fkey;   // kFree: an empty slot
  const int* fid;                   // the voxel's id in the map
  const unsigned long long* fsum;   // [4][fmask + 1]: N, Qx, Qy, Qz the call added
};
struct ExtendWork {
  CmapWork w;                 // the staging; w.rows / w.row_cap: the map being extended; w.ctl [2] start tickets of k_ext_emit,
                              // [3] fault, [4] fresh voxels (k_ext_emit); [0] staged (= touched) voxels, [1] points (k_cmap_stage)
  int* fid;                   // [w.fmask + 1] the id of a staged voxel (k_ext_emit)
  long long base;             // the map's voxels before the call: the first fresh id
  long long side_cap;         // ids the two arrays below hold (<= row_cap): the ids the call can reach
  unsigned long long* miss;   // [side_cap] or null: M of a fresh id is zeroed
  unsigned long long* sums;   // [side_cap][kSurfelSums] or null: the thirteen sums of a fresh id are zeroed
};
// emit (numbers the staged voxels; reads the map's table), then commit (writes the rows): each returns the launches it made
int launch_extend_emit(const ExtendWork& X, hipStream_t s);
int launch_extend_commit(const ExtendWork& X, hipStream_t s);

// ---- the carve of the closed map: per occupied voxel, the rays of the keyframes that passed through it (tl_carve.hip,
// DESIGN.md section 21).  A ray is a stored point of a keyframe: from the translation of the keyframe's pose to the point under
// that pose.  The rays come from a span table of the closed map's kind (CmapSpan) written for the carve's ray mask; the map is
// looked up through its own slot table and nothing in it is written: the counts are an array of their own, in id order
struct CarveWork {
  SpanInput in;               // the rays: the points of all spans, under the poses the closed map was built with
  MapGrid grid;               // the closed map
  double max_range, end_margin, radius2;   // radius2 = radius * radius (+inf: the distance does not decide)
  unsigned long long* miss;   // [grid.nv] M in id order
  unsigned long long* ctl;    // [0] skipped rays, [1] steps, [2] tested, [3] misses, [4] voxels with M > 0
};
// clear | rays | count: no host synchronisation; returns the launches it made (the same for every size)
int launch_carve(const CarveWork& W, hipStream_t s);
// its parts, for the extension: the rays of W.in walked and their misses ADDED to what W.miss and W.ctl hold; the
// voxels with M > 0 added to W.ctl[4]
int launch_carve_rays(const CarveWork& W, hipStream_t s);
int launch_carve_count(const CarveWork& W, hipStream_t s);
struct CarveReadArgs {
  VmapReadArgs rows;          // the closed map's rows, the box (when `boxed`), min_count, the outputs, look and ctl as k_vmap_box's
  CarveGate gate;             // a voxel is left out when gate.seen_through(M, N) (gate.gate is not asked: the read is the gate's)
  long long* out_m;           // the misses of the voxels kept (may be null)
  int boxed;                  // 0: the whole map
};
void launch_carve_read(const CarveReadArgs& A, hipStream_t s);

// ---- the surfels of the closed map: per voxel the second moments of its points, and from them a normal and three variances
// (tl_surfel.hip).  The points are the build's: a span table of the closed map's kind written for the
// build's cloud mask, under the poses of the build.  The map is looked up through its own slot table and nothing in it is
// written: the sums and the results are arrays of their own, in id order
constexpr int kSurfelSums = 13;   // Ns, Rx Ry Rz, Sxx Sxy Sxz Syy Syz Szz, Wx Wy Wz
struct SurfelWork {
  SpanInput in;               // the points of all spans, under the poses the closed map was built with
  int* kf_over;               // [in.nkf] 1: a finite point of the keyframe left the grid (k_surfel_flag): it adds nothing
  MapGrid grid;               // the closed map
  int runs;                   // 1: runs of equal voxels among a wave's consecutive lanes are summed before the atomics
  int min_points;             // a voxel of fewer points is not solved
  unsigned long long* sums;   // [grid.nv][kSurfelSums] int64 (two's complement) in id order
  double* normal;             // [grid.nv][3]
  double* eval;               // [grid.nv][3] ascending, m^2
  unsigned long long* ctl;    // [0] points summed, [1] orphan points, [2] solved voxels
};
// clear | flag | accum | solve: no host synchronisation; returns the launches it made (the same for every size)
int launch_surfels(const SurfelWork& W, hipStream_t s);
// its parts, for the extension: the points of W.in (W.kf_over as the caller flagged it) ADDED to what W.sums and
// W.ctl hold; then the voxels of a staging table solved again, a thread per slot, the voxels that became solved added to W.ctl[2]
int launch_surfel_accum(const SurfelWork& W, hipStream_t s);
int launch_surfel_solve_staged(const SurfelWork& W, const StagedVoxels& V, hipStream_t s);
struct SurfelReadArgs {
  VmapReadArgs rows;          // the closed map's rows, the box (when `boxed`), min_count, out_c, out_n (Ns), look and ctl as k_vmap_box's
  const unsigned long long* sums;
  const double *normal, *eval;
  int min_points;
  int boxed;                  // 0: the whole map
  double max_sigma2;          // a voxel is kept when it is solved, ev2 > 0, ev0 <= max_sigma2 and ev1 - ev0 >= min_planarity * ev2
  double min_planarity;
  double *out_nrm, *out_ev;   // [3] per voxel kept (may be null)
};
void launch_surfel_read(const SurfelReadArgs& A, hipStream_t s);

// ---- localisation of a scan in the closed map: point-to-plane Gauss-Newton on the surfels (tl_localise.hip, DESIGN.md
// section 23).  The map is looked up through its own slot table and nothing of it, of the carve or of the surfels is written
struct LocRecord {            // what a probe hit reads of a voxel: one 64-byte line
  double c[3];                // the row centroid
  double n[3];                // the surfel's normal
  int eligible;               // the surfel passes the gate
  int pad[3];
};
static_assert(sizeof(LocRecord) == 64, "a voxel record is one cache line");
constexpr int kLocTerms = 28;       // H's upper triangle by rows (21), g (6), cost
constexpr int kLocRow = 32;         // a block's partial row: the terms, matched, used, finite (the counts as doubles: exact below 2^53), one unused
constexpr int kLocMaxIterations = 64;
constexpr int kLocMaxBatch = 32;    // hypotheses of one scan in one set of launches (tloam_closed_map_localise_batch)
constexpr int kLocFinite = 30;      // the row slot of the scan's finite points
struct LocLog {               // tloam_closed_map_localise_record
  double pose[16];
  double tau, cost;
  double d[6];
  long long matched, used;
};
struct LocState {             // the stage's words in HBM: written by the host before a call, by k_loc_step during it
  double M[16];               // the matrix the next sweep runs at
  double tau;                 // ... and its truncation
  double pw;                  // max_residual0 * shrink^k
  Pose T;                     // the state
  double sums[kLocRow];       // of the last executed sweep
  int done;                   // the call has ended: the launches behind return on entry
  int status;
  int iterations;
  int reserved0;
};
struct LocPrepArgs {
  MapGrid grid;               // the closed map
  const unsigned long long* sums;   // the surfels' thirteen per voxel
  const double *normal, *eval;
  int min_points;
  double max_sigma2, min_planarity;
  LocRecord* rec;
};
struct LocSweepArgs {
  const double* pts;          // the scan, AoS
  long long n;
  LocState* st;
  MapGrid grid;               // the closed map
  const LocRecord* rec;
  double* partial;            // [blocks][kLocRow]
  int* ids;                   // [n] or null
  double* res;                // [n] or null
};
struct LocStepArgs {
  LocState* st;
  const double* partial;
  int nblocks;
  int k;                      // the iteration; -1: sum only (tloam_closed_map_linearise)
  int max_iterations, min_matches;
  double shrink, min_residual, step_tol_t, step_tol_r, min_pivot_ratio;
  LocLog* log;                // [max_iterations]
};
inline int loc_blocks(long long n) { return (int)((n + 255) / 256); }
void launch_loc_prepare(const LocPrepArgs& A, hipStream_t s);
// B hypotheses (1: the single call, a linearise): st [B], partial [B][blocks][kLocRow], log [B][kLocMaxIterations]; ids and
// res are written when non-null, which only B = 1 callers pass
void launch_loc_sweep(const LocSweepArgs& A, int B, hipStream_t s);
void launch_loc_step(const LocStepArgs& A, int B, hipStream_t s);

// relocalisation: a candidate of the place search made a hypothesis of the batched localiser
struct PlaceCandidate;
struct RelocHyp {
  long long keyframe;
  int shift, skipped;           // skipped: d is not < max_dist (or the build's pose is no rigid transform): never swept
  double d, yaw;
  double prior[16];             // P_build[keyframe] * Rz(yaw), column-major
};
struct RelocPriorArgs {
  const PlaceCandidate* cand;   // [B] of k_place_rank / k_place_shift
  const double* poses;          // [K][16] the poses the closed map's build used
  int B, S;
  double max_dist;
  double max_residual0, min_residual;
  RelocHyp* hyp;                // [B]
  LocState* st;                 // [B] the batched localiser's state words
};
void launch_reloc_priors(const RelocPriorArgs& A, hipStream_t s);

// ---- a scan diffed against the closed map (tl_diff.hip): a label per point from the localiser's voxel
// records, and per voxel the rays of the scan that passed through it (`through`) and the returns that fell in it (`hits`).
// Nothing of the closed map, the carve or the surfels is written: the counts are arrays of their own, in id order
constexpr int kDiffCtl = 16;    // control words: [0..3] the label counts, [4] skipped rays, [5] steps, [6] tested, [7] the sum of
                                // through, [8] voxels with through > 0, [9] voxels with hits > 0
struct DiffWork {
  ScanAt scan;                // the scan
  MapGrid grid;               // the closed map
  double max_range, end_margin, radius2;   // the rays': radius2 = radius * radius
  double plane_tol, near2;    // the labels': near2 = near * near
  CarveGate gate;             // a voxel that does not count explains no point (min_count = 1)
  const LocRecord* rec;       // [nv] the localiser's records
  unsigned long long* through;   // [nv]
  unsigned long long* hits;      // [nv]
  unsigned char* labels;      // [n]
  int* ids;                   // [n] or null
  unsigned long long* ctl;    // [kDiffCtl], zero before the launches
};
// (clear |) points | rays | count: no host synchronisation; returns the launches it made (the same for every size)
int launch_diff(const DiffWork& W, bool clear, hipStream_t s);
struct DiffReadArgs {
  VmapReadArgs rows;          // the closed map's rows, the box (when `boxed`), min_count, the outputs, look and ctl as k_vmap_box's
  const long long *through, *hits;   // [count] in id order
  long long min_through;
  double gone_ratio;          // a voxel is kept when through >= min_through && (double) through > gone_ratio * (double) hits
  long long *out_through, *out_hits;   // of the voxels kept (may be null)
  int boxed;                  // 0: the whole map
};
void launch_diff_read(const DiffReadArgs& A, hipStream_t s);

// ---- the closed map ray-cast (tl_raycast.hip): per segment from the pose's translation the first voxel
// it meets, from the localiser's voxel records.  Nothing of the closed map, the carve, the surfels or the diff is written
constexpr int kRaycastCtl = 8;   // control words: [0] skipped, [1] missed, [2] centroid hits, [3] plane hits, [4] steps, [5] tested
struct RaycastWork {
  ScanAt scan;                // the segment ends (scan.pts) and the pose
  MapGrid grid;               // the closed map
  double max_range, radius2;  // radius2 = radius * radius, radius = radius_cells * voxel
  CarveGate gate;             // a voxel that does not count is passed through
  int planes;                 // 0 the centroid test alone, 1 the plane test where eligible, 2 the plane test alone
  int reserved0;
  const LocRecord* rec;       // [nv] the localiser's records
  unsigned char* status;      // [n]
  double* range;              // [n]
  int* ids;                   // [n] or null
  unsigned long long* ctl;    // [kRaycastCtl], zero before the launch
};
void launch_raycast(const RaycastWork& W, hipStream_t s);   // one launch

// ---- the closed map's free space (tl_free.hip): a dense grid of 4 x 4 x 4-cell bricks, one 64-bit word a
// brick, bit ((cz & 3) << 4) | ((cy & 3) << 2) | (cx & 3) set when a ray saw through the cell.  Nothing of the closed map, the
// carve, the surfels or the diff is written; whether a cell is a voxel is resolved when the grid is read
constexpr int kFreeCtl = 8;      // control words: [0] skipped rays, [1] cells marked, [2] cells outside, [3] free cells, [4] bricks nonzero
struct FreeGrid {
  unsigned long long* words;  // [nwords]: brick (bx, by, bz) at ((bz - blo[2]) * nb[1] + (by - blo[1])) * nb[0] + (bx - blo[0])
  int blo[3];                 // the lowest brick of the box per axis (brick = cell >> 2)
  int nb[3];                  // bricks per axis
  long long nwords;
};
struct FreeWork {
  SpanInput in;               // the keyframe form: the rays of all spans, under the poses the closed map holds
  ScanAt scan;                // the scan form: the ends at one pose
  MapGrid grid;               // the closed map (its table is not read by the walk)
  double max_range, end_margin;
  FreeGrid g;
  unsigned long long* ctl;    // [kFreeCtl], zero before the launches
};
int launch_free_clear(const FreeGrid& g, hipStream_t s);                 // the words zeroed; returns the launches it made
int launch_free_rays(const FreeWork& W, bool spans, hipStream_t s);      // rays | count: the same two launches for every size
struct FreeQuery {            // what a read of the grid resolves occupancy with
  MapGrid grid;               // the closed map
  CarveGate gate;             // which of its voxels count
  FreeGrid g;
};
struct FreePointsArgs {
  FreeQuery q;
  ScanAt scan;                // the points, and the pose when `posed`
  int posed;                  // 1: the points are in the sensor frame of scan.M; 0: in the map frame
  int reserved0;
  unsigned char* state;       // [n]
  int* ids;                   // [n] or null
  unsigned long long* ctl;    // [0..3] points per state, zero before the launch
};
void launch_free_points(const FreePointsArgs& A, hipStream_t s);
struct FreeCellsArgs {
  FreeQuery q;
  int boxed;                  // 1: only centres inside [lo, hi] (inclusive)
  int reserved0;
  double lo[3], hi[3];
  double* out_c;              // AoS centres, brick index ascending, then bit ascending
  unsigned long long* look;   // [blocks + 1] look-back words, zero before the launch
  unsigned long long* ctl;    // [0] start tickets, [1] fault, [2] cells written; zero before the launch
};
void launch_free_cells(const FreeCellsArgs& A, hipStream_t s);
struct FreeColumnsArgs {
  FreeQuery q;
  int z0, z1;                 // the band's cells, clipped to the box (z0 > z1: empty)
  long long min_free;
  unsigned char* state;       // [4 nb[1]][4 nb[0]], y outer
};
void launch_free_columns(const FreeColumnsArgs& A, hipStream_t s);

// ---- the closed map's clearance (tl_clear.hip): a dense field of uint16 over the free-space grid's box,
// [z][y][x], x fastest: d2, the squared distance in cells to the nearest obstacle cell, exact up to R * R, kClearBeyond above.
// Nothing of the closed map, the carve, the surfels, the diff or the free-space grid is written
constexpr int kClearCtl = 8;     // control words: [0] obstacle cells, [1] finite cells, [2] the sum of d2, [3] the largest d2;
                                 // of a query [0..3] the points per state / the segments per status
constexpr unsigned short kClearBeyond = 0xFFFF, kClearOutside = 0xFFFE;
constexpr int kClearTile = 64;   // outputs along the pass axis per block of k_clear_axis: its LDS strip is kClearTile + 2 R rows
struct ClearField {
  const unsigned short* d2;   // [n[2]][n[1]][n[0]] (null: none -- the seed and the passes take their buffers beside this)
  int lo[3];                  // the lowest cell of the box per axis
  int n[3];                   // cells per axis, each a multiple of 4
  long long cells;
  int R, wrap;                // wrap: unknown_is_obstacle -- an UNKNOWN cell and everything outside the box is an obstacle
};
struct ClearBuildArgs {
  FreeQuery q;
  ClearField f;               // (f.d2 is not read)
  unsigned short *out, *tmp;  // [cells] each: seed -> tmp, x: tmp -> out, y: out -> tmp, z: tmp -> out
  unsigned long long* ctl;    // [kClearCtl], zero before the launches
};
int launch_clear_build(const ClearBuildArgs& A, hipStream_t s);   // seed | voxels | x | y | z | count; returns the launches
struct ClearPointsArgs {
  FreeQuery q;
  ClearField f;
  ScanAt scan;                // the points, and the pose when `posed`
  int posed, reserved0;
  unsigned char* state;       // [n]
  unsigned short* d2;         // [n]
  double* distance;           // [n] or null
  unsigned long long* ctl;    // [0..3] points per state, zero before the launch
};
void launch_clear_points(const ClearPointsArgs& A, hipStream_t s);
struct ClearSegmentsArgs {
  MapGrid grid;               // the closed map's grid (its table is not read)
  ClearField f;
  ScanAt scan;                // the segments' ends, and the pose when `posed`
  const double* starts;       // [3 n] AoS
  int posed, need;            // need: a cell with d2 < need blocks
  double max_segment;
  unsigned char* status;      // [n]
  unsigned short* min_d2;     // [n]
  double* t_block;            // [n] or null
  unsigned long long* ctl;    // [0..3] segments per status, zero before the launch
};
void launch_clear_segments(const ClearSegmentsArgs& A, hipStream_t s);
struct ClearColumnsArgs {
  const unsigned char* state; // [ny][nx] of k_free_columns
  int nx, ny, R, wrap;
  unsigned short *out, *tmp;  // [ny][nx] each: seed -> out, x: out -> tmp, y: tmp -> out
};
int launch_clear_columns(const ClearColumnsArgs& A, hipStream_t s);   // seed | x | y; returns the launches

// ---- a dense field of uint32 over a box of cells, [z][y][x], x fastest, relaxed in tiles to a min-fixpoint by rounds (the
// engine: tl_tile.hpp; its host runner: tl_ctx.hpp's tile_rounds; the box arithmetic: tl_tile_box.hpp): the route's costs and
// the frontiers' labels
constexpr int kTileMaxBatch = 1024;             // the most rounds between two waits (rounds_per_wait's range)
struct TileField {
  unsigned* v;                // [n[2]][n[1]][n[0]]
  int lo[3];                  // the lowest cell of the box per axis
  int n[3];                   // cells per axis (the frontiers': n[0] a multiple of 4)
  int tiles[3];               // tiles per axis (tl_tile_box.hpp's kTileX x kTileY x kTileZ, the last of an axis partial)
  int reserved0;
  long long cells;
};

// ---- the route through the closed map (tl_route.hip): a dense field of uint32 over the clearance field's
// box (or over a column layer: n[2] = 1), [z][y][x], x fastest: the least 3-4-5 chamfer weight to an accepted goal over the
// traversable cells.  Nothing but the field, its tile flags and the control words is written
constexpr unsigned kRouteUnreached = 0xFFFFFFFFu, kRouteBlocked = 0xFFFFFFFEu, kRouteOutside = 0xFFFFFFFDu;
constexpr int kRouteCtl = kTileMaxBatch + 8;     // control words: [0] goals accepted, [1] rejected, [2] tiles the goals marked;
                                                 // [4] traversable cells, [5] reached cells, [6] the sum, [7] the largest cost;
                                                 // [8 + k] the tiles round k of a batch marked
struct RouteSeedArgs {
  TileField f;
  const unsigned short* d2;   // the clearance (field or column layer) over the same box
  int need;                   // max(need, 1): a cell with d2 >= need is traversable
  int flat;                   // 1: the column form -- a goal is placed by x and y, its z cell is lo[2]
  double voxel, origin[3];
  ScanAt goals;               // the goals, and the pose when `posed`
  int posed, reserved0;
  unsigned* next;             // [tiles] the flags of the first round, zero before the launches
  unsigned long long* ctl;    // [kRouteCtl], zero before the launches
};
void launch_route_seed(const RouteSeedArgs& A, hipStream_t s);   // seed | goals: two launches
// One round: a block a tile, the tiles flagged in `now` relaxed (and their flags taken down), their neighbours flagged in `next`,
// the fresh flags counted into *marks
void launch_route_round(const TileField& f, unsigned* now, unsigned* next, unsigned long long* marks, hipStream_t s);
void launch_route_count(const TileField& f, unsigned long long* ctl, hipStream_t s);
struct RoutePointsArgs {
  TileField f;
  double voxel, origin[3];
  ScanAt scan;                // the points, and the pose when `posed`
  int posed, reserved0;
  unsigned* cost;             // [n]
  double* distance;           // [n] or null
  unsigned long long* ctl;    // [0..3] points reached / unreached / blocked / outside, zero before the launch
};
void launch_route_points(const RoutePointsArgs& A, hipStream_t s);
struct RoutePathsArgs {
  TileField f;
  double voxel, origin[3];
  ScanAt scan;                // the starts, and the pose when `posed`
  int posed, reserved0;
  long long max_cells;
  unsigned char* status;      // [n]
  int* n_cells;               // [n]
  unsigned* cost;             // [n]
  double* centres;            // [n * max_cells * 3], zero before the launch
};
void launch_route_paths(const RoutePathsArgs& A, hipStream_t s);

// ---- the frontiers of the closed map (tl_frontier.hip): a dense field of uint32 over the free-space
// grid's box (or over a column layer: n[2] = 1), [z][y][x], x fastest: a frontier cell's value is the least linear index of its
// 26-connected component of frontier cells, every other cell's its state's sentinel.  Nothing but the field, its tile flags, the
// cluster table and the control words is written
constexpr unsigned kFrontFree = 0xFFFFFFFFu, kFrontUnknown = 0xFFFFFFFEu, kFrontOccupied = 0xFFFFFFFDu, kFrontOutside = 0xFFFFFFFCu;
constexpr int kFrontRounds0 = 32;                      // the first of the rounds' control words
constexpr int kFrontCtl = kTileMaxBatch + kFrontRounds0;
// control words: [0] tiles the frontier cells marked, [1] the unknown faces; [2] free, [3] unknown, [4] occupied, [5] frontier
// cells, [6] roots; [8] the roots' start tickets, [9] their look-back's fault, [10] roots written; [12] [13] [14] the same of the
// kept list; [15] cells kept, [16] the largest component; [20] [21] [22] the same three of a cells read; [24 .. 28] the points of
// a query per kind; [kFrontRounds0 + k] the tiles round k of a batch marked
struct FrontTable {           // the clusters of a field, ascending in root
  const unsigned* roots;      // [nroots]
  const int* kept_of;         // [nroots] a component's index in the kept list, -1 when it is not kept
  long long nroots;
};
struct FrontSeedArgs {
  FreeQuery q;                // the 3-D form: brick words, then the counting voxel rows
  const unsigned char* state; // the column form: [n[1]][n[0]] of k_free_columns (null: the 3-D form)
  TileField f;
  unsigned* next;             // [tiles] the flags of the first round, zero before the launches
  unsigned long long* ctl;    // [kFrontCtl], zero before the launches
};
int launch_front_seed(const FrontSeedArgs& A, hipStream_t s);   // states (| voxels) | mark; returns the launches
// One round: k_route_round's form with min over the 26 neighbours that are frontier cells
void launch_front_round(const TileField& f, unsigned* now, unsigned* next, unsigned long long* marks, hipStream_t s);
void launch_front_count(const TileField& f, unsigned long long* ctl, hipStream_t s);
struct FrontGatherArgs {
  TileField f;
  unsigned* roots;                             // [nroots] out, ascending
  tloam_closed_map_frontier_cluster* rec;      // [nroots] out
  tloam_closed_map_frontier_cluster* kept_rec; // [nroots] out: the records with cells >= min_cells, in order
  int* kept_of;                                // [nroots] out
  long long nroots;
  unsigned min_cells;
  int reserved0;
  unsigned long long* look;   // [blocks_of(cells / 4) + 1 + blocks_of(nroots) + 1], zero before the launches
  unsigned long long* ctl;
};
int launch_front_gather(const FrontGatherArgs& A, hipStream_t s);   // roots | accumulate | keep; returns the launches
struct FrontCellsArgs {
  TileField f;
  FrontTable t;
  unsigned root;              // kFrontFree: the cells of every kept cluster
  int reserved0;
  double voxel, origin[3];
  long long m;                // the cells the host counted: nothing is written past them
  double* centres;            // [3 m] out
  unsigned* roots_out;        // [m] out
  unsigned long long* look;   // [blocks_of(cells / 4) + 1], zero before the launch
  unsigned long long* ctl;    // [20 .. 22] zero before the launch
};
void launch_front_cells(const FrontCellsArgs& A, hipStream_t s);
struct FrontPointsArgs {
  TileField f;
  FrontTable t;
  double voxel, origin[3];
  ScanAt scan;                // the points, and the pose when `posed`
  int posed, reserved0;
  unsigned* label;            // [n]
  int* cluster;               // [n] or null
  unsigned long long* ctl;    // [0 .. 4] points frontier / free / unknown / occupied / outside, zero before the launch
};
void launch_front_points(const FrontPointsArgs& A, hipStream_t s);
struct FrontCostsArgs {
  TileField f;
  FrontTable t;
  const unsigned* cost;       // the route field over the same box
  int reach, reserved0;
  unsigned long long* keys;   // [kept] all ones before the launch: min (cost << 32 | linear)
};
void launch_front_costs(const FrontCostsArgs& A, hipStream_t s);

// ---- the view gain of the closed map (tl_view.hip): per view the distinct UNKNOWN cells of the frontier
// field its rays cross, as the popcount of a bit window round the view's origin cell.  Nothing but the records, the windows and
// the counters is written
constexpr int kViewCounters = 8;   // a view's counters: unknown visits, free visits, steps, rays skipped / occupied / left the
                                   // box / ended, cells beyond the window
constexpr int kViewLdsThreads = 1024, kViewThreads = 256;
struct ViewArgs {
  TileField f;                // the frontier field: the states
  MapGrid grid;               // the map's grid: origin and voxel (ray_begin)
  double max_range;
  const double* poses;        // [16 views of the call] column-major, as they stand
  const double* ends;         // [3 rays] sensor frame
  long long rays;
  long long words;            // of one window: ceil(S^3 / 32)
  int W, S;
  long long view0;            // the first view of this launch (a chunk's); block b of the LDS form is view view0 + b
  int bpv, reserved0;         // the global form: blocks a view
  unsigned* win;              // the global form: [views of the chunk][words], zero before the ray launch
  unsigned long long* cnt;    // the global form: [views of the chunk][kViewCounters], zero before the ray launch
  tloam_closed_map_view_record* out;   // [views of the call]
  unsigned long long* beyond;        // [views of the call] a view's visited cells beyond its window
  double* centres;            // the cells form: [3 capacity] out, ascending in bit index (null: none)
  long long capacity;
};
size_t view_lds_static();                                      // the LDS form's static shared memory, bytes
hipError_t launch_view_lds(const ViewArgs& A, long long views, bool cells, hipStream_t s);   // one launch
void launch_view_rays(const ViewArgs& A, long long views, hipStream_t s);                    // the global form: the rays ...
void launch_view_count(const ViewArgs& A, long long views, bool cells, hipStream_t s);       // ... then the popcount and the records

// ---- deskew of a scan under constant velocity (tl_deskew.hip) -------------
struct DeskewArgs {
  const double* in;               // AoS xyz [3n]
  const double* t;                // timed mode: seconds relative to the pose's instant [n]; null: azimuth mode
  double* out;                    // AoS [3n]; null: the times are checked and nothing is written
  unsigned long long* max_shift;  // bits of max |p' - p| (atomic max; zero before the launch); null: not reduced
  unsigned long long* bad;        // set to 1 when a time is refused (zero before the launch); null in azimuth mode
  long long n;
  double xi[6];                   // the frame's motion log(step): (upsilon, omega)
  double period;                  // timed: s = t / period
  double direction, start, ref;   // azimuth: s = wrap_[0,2pi)(direction * (atan2(y, x) - start)) / 2pi - ref
};
void launch_deskew(const DeskewArgs& A, hipStream_t s);

// ---- place recognition: Scan Context descriptors and the keyframe search (tl_place.hip) ----------
constexpr int kPlaceMaxRings = 64, kPlaceMaxSectors = 360, kPlaceMaxCandidates = 32;
struct PlaceDescArgs {
  const double* aos;              // AoS xyz [3n], sensor frame
  long long n;
  unsigned long long* bins;       // [R S] order-preserving images of the bin maxima; all zero before (k_place_keys zeroes them after)
  double* desc;                   // [R S] row-major by ring
  double* ring_key;               // [R]
  double* sector_key;             // [S]
  long long* frame_out;           // commit (null: describe only): the keyframe's frame number and pose
  double* pose_out;               // [16] column-major
  long long frame;
  double pose[16];
  int R, S;
  double max_radius, height_offset;
};
void launch_place_describe(const PlaceDescArgs& A, hipStream_t s);   // k_place_bin (n > 0), k_place_keys

struct PlaceCandidate { double d; int shift; int keyframe; };
struct PlaceSearchArgs {
  const double* desc;             // the database [K][R S], ring keys [K][R], frame numbers [K]
  const double* ring_key;
  const long long* frames;
  double* kdist;                  // scratch [m]
  int* taken;                     // scratch [m]
  PlaceCandidate* cand;           // scratch [num_candidates]
  tloam_place_loop* loops;        // the loop records [K]
  unsigned long long* n_loops;    // their count
  const double* q_desc;           // the query's descriptor and ring key when it is not a keyframe (null: keyframe q's)
  const double* q_ring_key;
  int q;                          // the query keyframe
  int m;                          // keyframes 0 .. m-1 are searched (m >= 1)
  int ncand;                      // min(num_candidates, m)
  int R, S;
  double dist_thres;
};
void launch_place_search(const PlaceSearchArgs& A, hipStream_t s);   // k_place_rank, k_place_shift, k_place_pick
void launch_place_candidates(const PlaceSearchArgs& A, hipStream_t s);   // k_place_rank, k_place_shift: cand[0 .. ncand), no record

// ---- loop verification: keyframe clouds, the local target, the score (tl_loop.hip) ------------------
constexpr int kLoopSpans = 16;    // spans per launch of k_place_clouds / k_loop_assemble
struct LoopSpan {
  const double* src;              // AoS xyz; rows idx[i] of it when idx is set, else rows i
  const int* idx;
  double* dst;                    // AoS xyz [3n]
  long long n;
  int rigid;                      // 1: x' = ((R00 x + R01 y) + R02 z) + t0 per axis; 0: the bytes as they are
  int reserved0;
  double R[9], t[3];              // row-major rotation, translation
};
struct LoopSpanArgs {
  LoopSpan s[kLoopSpans];
  long long start[kLoopSpans + 1];   // rows before span j (start[nspan] = all rows)
  int nspan;
};
void launch_place_clouds(const LoopSpanArgs& A, hipStream_t s);    // k_place_clouds: a keyframe's eight clouds into the arena
void launch_loop_assemble(const LoopSpanArgs& A, hipStream_t s);   // k_loop_assemble: a verification's source and target
constexpr int kLoopScoreBlocks = 256;
struct LoopScoreArgs {
  const double* src[kKinds];      // the source clouds, AoS
  long long n[kKinds];
  GridView g[kKinds];             // the fine stage's grids over the target clouds (g.n == 0: no target of the kind)
  int reach[kKinds];              // cells walked around the query's: ceil(inlier_dist / cell)
  double R[9], t[3];              // the fine pose
  double r2;                      // inlier_dist^2: a point is an inlier when its nearest target is closer
  double* partial;                // [kLoopScoreBlocks][kKinds][2]: inliers, sum of their squared distances
};
void launch_loop_score(const LoopScoreArgs& A, hipStream_t s);

// ---- pose-graph optimisation of the keyframes (tl_graph.hip) ----------------------------------------
constexpr int kGraphThreads = 512;    // k_graph_step is ONE workgroup: its barriers order the conjugate gradients, nothing spins
struct GraphRecord {                  // what one Gauss-Newton iteration reports
  double cost_before, cost_after, max_step, cg_residual;
  int cg_iterations, cg_limit;        // cg_limit 1: the solve ended on max_cg
};
struct GraphArgs {
  int n, m;                       // nodes, edges (edges 0 .. n-2 the chain)
  int chunk;                      // nodes per thread: thread t owns nodes 1 + t chunk .. 1 + (t + 1) chunk - 1
  int max_cg;
  double cg_tol2;                 // cg_tol^2
  const Pose* P;                  // [n] the poses linearised at
  Pose* Pn;                       // [n] the stepped poses
  const int2* ij;                 // [m]
  const Pose* Zinv;               // [m] rigid_inverse(Z)
  const double* w;                // [m][6]
  const int* node_start;          // [n + 1] a node's entries of node_ent, in edge order
  const int* node_ent;            // 2 edge + side: side 0 the edge ends at the node (j), 1 it starts there (i)
  Rt* A;                          // [m] rigid_inverse(P_j) * P_i: J_i = -Ad(A)
  double* contrib;                // [2 m][6] an edge's terms for its j and its i node
  Rt *Q, *Qi;                     // [n] rigid_inverse(P_0) * P_k and its inverse
  double *x, *r, *z, *p, *ap, *tmp;   // [n][6]
  GraphRecord* rec;
};
void launch_graph_step(const GraphArgs& A, hipStream_t s);   // k_graph_step: linearise, solve, step, the new cost
// the robust mode: the loop edges' statistics r_e at A.P with the base weights, their scales, the solver's
// weights w = s * w0
constexpr int kGraphReweightOnes = 0;   // s = 1 (after the plain solve: only r is wanted)
constexpr int kGraphReweightRule = 1;   // s from r by the scale rule at mu
constexpr int kGraphReweightKeep = 2;   // s as stored (after the last solve: only r is wanted)
struct GraphRobustRecord {
  double max_r;                   // over the loop edges (a NaN is passed over)
  double sum_sr;                  // sum of s_e r_e: the loop edges' share of the cost the next solve starts from
  int rejected, kept, undecided;  // s == 0, s == 1, in between
  int reserved0;
};
struct GraphReweightArgs {
  int mode;                       // kGraphReweight*
  double mu, c2;                  // c2: noise_chi2
  const double* w0;               // [m][6] the base weights
  double* w;                      // [m][6] the solver's weights: rows n-1 .. m-1 are written
  double* s;                      // [m - (n - 1)] the loop edges' scales
  double* r;                      // [m - (n - 1)] their statistics
  GraphRobustRecord* rec;
};
void launch_graph_reweight(const GraphArgs& A, const GraphReweightArgs& W, hipStream_t s);   // k_graph_reweight (A.w is not read)

// ---- PCA feature extraction (tl_feature.hip; feature_extract.cpp:47-197) -----------------------
struct FeatArgs {
  GridView g;                 // grid over the cloud itself (cell >= radius)
  const double *x, *y, *z;    // the cloud, SoA, original order
  int n;
  double radius;
  int K, min_neigh;
  double *flatness, *cvr, *sphericity, *normal;  // [n], [n], [n], [3n] AoS
  int *num_sum, *neigh;                          // [n], [n * K] (-1 padded)
};
struct FeatSelect { double cvr_submap, planar_submap_thres, planar_vertic_thres; };
void launch_pca_info(const FeatArgs& A, hipStream_t s);
struct FeatRankCtl {   // control block of the ranking (tl_feature.hip): two lists, 0 planar, 1 sphere
  unsigned long long kmin[2], kmax[2];   // order-preserving keys of the smallest / largest flatness of a list
  int hist[2][4096 + 1];                 // bucket sizes, then bucket starts (+ the list's length)
};
void launch_feat_select(const FeatArgs& A, const FeatSelect& S, unsigned long long* flags, unsigned long long* scan,
                        unsigned long long* scan_tmp, double* f2, int* idx2, FeatRankCtl* ctl, int* bkt, int* pos, double* gf, int* gi,
                        double* out, hipStream_t s);

// K3 and the minimiser
int k3_grid_for(int total_cap, int device_cus);
// one wave per chunk (small sets) vs the streaming variant (wide: blocks of eight waves, see tl_gn.hip); *grid = blocks launched = rows
void k3_plan(const int cap[kKinds], int device_cus, int* grid, bool* single, bool* wide);
void launch_k3(const CorrView& cv, GnState* st, double* partials, int grid, bool single, bool wide, bool force, hipStream_t s,
               hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// sharded contexts: the sweep whose LAST block (ticket counter) also folds the block rows into out48 and, with a
// mailbox, posts them to every rank -- the sweep of a sharded GN iteration is then 2 launches (+ the collective)
struct K3Fuse {
  int* ticket;       // zero between launches
  double* out48;     // this rank's totals (all-reduced by RCCL / the callback when there is no mailbox)
  MboxView mb;       // mb.nranks == 0: no mailbox
};
void launch_k3_fused(const CorrView& cv, GnState* st, double* partials, int grid, bool single, bool wide, bool force,
                     const K3Fuse& fuse, hipStream_t s);
// one GN iteration in ONE launch, whatever the size of the set: the sweep whose last block folds the rows and advances the
// minimiser (mailbox contexts: posts, gathers and advances) -- k3_sweep_step, tl_gn.hip.  span: see K3Step (may be null)
// iter_span (every launcher of a kernel that ends a GN iteration): the device-side period counter of tloam_gn_iter_timer, or null
void launch_k3_step(const CorrView& cv, GnState* st, double* partials, int grid, bool single, bool wide, int* ticket, unsigned long long* span,
                    const MboxView* mb_or_null, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                    unsigned long long* iter_span = nullptr);
void launch_gn_step_mbox(GnState* st, const MboxView& mb, hipStream_t s, unsigned long long* iter_span = nullptr);   // gather (rank order) + consume
void launch_mbox_allreduce(double* buf, int count, const MboxView& mb, hipStream_t s);  // buf <- sum over ranks
void launch_mbox_gather_only(double* out48, const MboxView& mb, hipStream_t s);
void launch_reduce(const double* partials, int grid, GnState* st, double* out48, hipStream_t s);
void launch_solve_init(GnState* st, hipStream_t s);                   // begin one ceres::Solve at st->x
void launch_set_eval(GnState* st, const double* se3_dev, hipStream_t s);
void launch_pose_from_x_build(GnState* st, hipStream_t s);   // st->T_cur = exp(st->x_build)
void launch_gn_step(GnState* st, const double* in48, hipStream_t s, unsigned long long* iter_span = nullptr);  // consume a reduced sweep
void launch_reduce_and_step(const double* partials, int grid, GnState* st, hipStream_t s, unsigned long long* iter_span = nullptr);
// small sets on one rank: sweep + step in ONE launch (ticket: zero between launches)
void launch_sweep_step_small(const CorrView& cv, GnState* st, double* partials, int* ticket, int grid, hipStream_t s,
                             unsigned long long* iter_span = nullptr);
// sets whose sweep is a grid of a dozen blocks: a whole ceres::Solve (up to max_sweeps evaluations) in ONE launch
// The factor set of an outer iteration prepared by the Solve launch itself (no k_prepare_small launch in front of it):
// flagb == null means "already prepared" (stepwise API, topped-up Solves).
struct SolvePrep {
  SlotView sv;
  int maxnum[kKinds];
  const int* run_build;     // device gates of the outer loop; null: always build (the frame's first iteration)
  const int* run_refresh;
};
// K4
struct WeightParams {
  double th1, th2, mu, noise_bound_sq;
  int active[kKinds];
};
// The finish of the outer iterations a one-launch Solve may run itself (device-driven loop, KITTI-size sets): every wave
// updates the weights of the factors it holds and adds their side-channel costs up, the consumer wave makes the loop
// decisions and writes the result slot; if the loop goes on with an unchanged pose the launch refreshes its correspondences
// in registers and runs the next Solve as well.  enabled == 0: the launch ends with the Solve and leaves the sums in the
// state for the finish kernel (GnState::fin_valid).
struct SolveFinish {
  int enabled;
  int have_wp;               // wp[first_iter ..] are set: the launch adds up the finish sums of its Solve(s)
  int first_iter, n_iter;    // outer iteration this launch was enqueued for; max_iterations
  double cost_threshold;     // registration.cpp:1108
  double* sums16;
  unsigned long long* iter_span;   // the lead's stepper notes the period of its GN iterations here (tloam_gn_iter_timer), or null
  WeightParams wp[kMaxOuterInLaunch];   // per outer iteration
  HostMirror hm[kMaxOuterInLaunch];
};
void launch_solve_small(const CorrView& cv, GnState* st, double* partials, int* ticket, int grid, int max_sweeps,
                        const SolvePrep* prep_or_null, int* seg_n, const SolveFinish* finish_or_null, hipStream_t s);
// (gated on st->done: see k_weights)
void launch_weights(const CorrView& cv, const SlotView& sv, const WeightParams& wp, double* partial /*[blocks*8]*/,
                    int blocks, const GnState* st, hipStream_t s);
void launch_outer_finish(const double* partial, int blocks, const int* seg_n, GnState* st_or_null, GnState* gate,
                         double* sums8, HostMirror hm, OuterCtl ctl, hipStream_t s);
void launch_outer_publish(const double* sums8, GnState* st, HostMirror hm, const unsigned long long* comm_err_or_null,
                          hipStream_t s);
// weights + finish in one launch for small single-rank sets
// KITTI-size frames, device-driven loop: the finish of outer iteration k-1 (the first sixteen blocks) and the
// correspondence search of iteration k (the other blocks, gated on GnState::spec_build) in ONE launch -- they are
// independent of each other
struct FinishSmallArgs {
  const CorrView* cv;
  const WeightParams* wp;
  const int* seg_n;
  double* sums16;
  HostMirror hm;
  OuterCtl ctl;
  double* rows;   // [16][8] hand-over rows of the sixteen finish blocks
  int* ticket;    // zero between launches
};
void launch_build_finish_small(const SlotView& sv, const GridView grids[kKinds], const BuildParams& bp, GnState* st,
                               const FinishSmallArgs& fin, hipStream_t s);
// large single-rank sets (thread-per-query search), device-driven loop: the same for k_weights + k_outer_finish -- the
// first 4 * wblocks one-wave blocks of the search launch are the finish (rows: [4 * wblocks][8] doubles)
struct FinishLargeArgs {
  const CorrView* cv;
  const WeightParams* wp;
  const int* seg_n;
  double* sums16;
  HostMirror hm;
  OuterCtl ctl;
  double* rows;
  int* ticket;
  int wblocks;
  // direct set: the weight stream the finish WRITES (every row), per kind; cv->k[].w is the one it reads.  null: compact set
  double* w_next[kKinds];
  // ... and where n_corr comes from: the per-block counts of the search that built the set solved in this iteration (blk_cnt,
  // nblk blocks) if built != 0 -- built < 0: GnState::run_build says whether it was (device-driven loop) --, else unchanged
  const int* blk_cnt;
  int nblk, built;
};
// the finish of a direct set as a launch of its own (stepwise API, the frame's last outer iteration, a topped-up Solve): the same
// one-wave blocks as the riding form, bit for bit
void launch_finish_direct(const FinishLargeArgs& fin, GnState* st, hipStream_t s);
void launch_build_finish_large(const SlotView& sv, const GridView grids[kKinds], const BuildParams& bp, GnState* st,
                               const unsigned long long* n_sorted, const double4* qrec, const FinishLargeArgs& fin, hipStream_t s,
                               const DirectSet* ds = nullptr);
void launch_weights_finish_small(const CorrView& cv, const SlotView& sv, const WeightParams& wp, const int* seg_n,
                                 double* sums16, GnState* st, HostMirror hm, OuterCtl ctl, hipStream_t s);
void launch_transform_cloud(double* aos, size_t n, const double M[16], hipStream_t s);
void launch_debug_se3(const double* x, const double* delta, int n, double* out /* 26 per item */, hipStream_t s);

// ---- the closed map's snapshot (tl_snapshot.hip): the device side of tloam_closed_map_save / _load.
// A save gathers the device-born sections into the blob's layout and forms their checksums; a load checks an uploaded blob's
// device-born sections word by word, and the slot table rebuilt from its keys.  Both work through a short list of PIECES --
// runs of 64-bit words that belong to one section -- so the launches are the same for every map; no kernel indexes by a value
// it read from a blob: every bound is a launch argument
constexpr int kSnapPieces = 12;
constexpr unsigned long long kSnapGolden = 0x9E3779B97F4A7C15ull;
constexpr long long kSnapMaxN = 1ll << 30;   // points of a build (tl_api_cmap.hip), so of a voxel
// control words: [section kind] its checksum (kinds 1 .. 9), then what k_snap_check and k_snap_table count
enum SnapCtl {
  kSnapBadFinite = 16,   // database words that are not finite doubles
  kSnapBadKey = 17,      // keys with an axis field outside [1, 2^21 - 1] or bit 63 set
  kSnapBadN = 18,        // N outside [1, 2^30]
  kSnapBadQ = 19,        // Q outside [0, N * 2^24]
  kSnapBadMiss = 20,     // M < 0
  kSnapBadSums = 21,     // Ns, Sxx, Syy or Szz < 0
  kSnapSumN = 22,        // the sum of N
  kSnapBadFind = 23,     // ids the rebuilt table does not find under their own key
  kSnapCtlWords = 24
};
enum SnapTest { kSnapTestNone = 0, kSnapTestFinite, kSnapTestKey, kSnapTestN, kSnapTestQ, kSnapTestMiss, kSnapTestSums };
struct SnapPiece {
  const unsigned long long* src;
  unsigned long long* dst;          // k_snap_pack: where the words go (null: they are in place, only summed)
  unsigned long long words;
  unsigned long long first;         // index of src[0] within its section: the checksum's i
  const long long* aux;             // kSnapTestQ: the N column, [aux_n]; word j of the piece is Q of row j % aux_n
  unsigned long long aux_n;
  int section;                      // the control word its checksum is added to
  int test;                         // k_snap_check: SnapTest
};
struct SnapPieces {
  SnapPiece piece[kSnapPieces];
  int npieces;
  unsigned long long* ctl;          // [kSnapCtlWords], zero before the launch
};
void launch_snap_pack(const SnapPieces& A, hipStream_t s);    // one launch: gather and checksum
void launch_snap_check(const SnapPieces& A, hipStream_t s);   // one launch: checksum and test
// the slot table of `T` (all slots free, at least 2 n of them) filled with ids [0, n), then every id looked up under its own
// key: two launches; a duplicated key fails the lookup of one of its ids whichever insert came first
void launch_snap_table(const VmapTable& T, size_t n, unsigned long long* ctl, hipStream_t s);
// k_surfel_solve alone (tl_surfel.hip), on sums that are already there: W.nv, min_points, voxel, sums, normal, eval, ctl[2]
void launch_surfel_solve(const SurfelWork& W, hipStream_t s);

}  // namespace tl
