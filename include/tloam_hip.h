/*
 * tloam_hip.h -- C ABI of the MI355X-native T-LOAM pose-optimisation path.
 *
 * This library replaces ONE path of the reference: LocalRegistration::scanMatching and
 * what it calls (reference: src/models/registration/registration.cpp:879-1133), i.e. the
 * four KDTreeFlann::SearchHybrid correspondence builders (:427-505, :517-559, :571-635,
 * :714-778), the three Ceres cost functors (:19-117), the SE(3) local parameterisation
 * (:162-179), ceres::Solve as configured at :1036-1047, the GNC-TLS weight update
 * (:858-876) and getFitnessScore (:257-296).  It sits behind the reference's plugin
 * boundary tloam::RegistrationInterface
 * (include/tloam/models/registration/registration_interface.hpp:40-48); the C++ adapter
 * that marshals a reference `Frame` into these calls is adapters/hip_registration.hpp and
 * the binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no torch / Eigen / Open3D types; pointers + sizes only.
 *   - every function returns TLOAM_OK (0) or a negative tloam_status; nothing throws or
 *     aborts (the reference asserts / SOPHUS_ENSUREs instead, registration.cpp:928-929,
 *     sophus/se3.hpp:497-504).
 *   - point clouds are borrowed for the duration of the call as contiguous AoS double[3]
 *     (== open3d::geometry::PointCloud2::points_.data(), PointCloud2.hpp:396) and copied
 *     to HBM as SoA.  4x4 poses are column-major doubles (== Eigen::Isometry3d::matrix()).
 *   - one context = one device + one HIP stream; not thread-safe (the reference has a
 *     single caller thread, lidar_odometry_nodelet.cpp:57-63).
 *   - se(3) vectors are (upsilon[3], omega[3]) -- translation part first, as
 *     registration.hpp:327-329.
 *   - there is NO CPU fallback: every entry point that computes needs a gfx950 device and
 *     returns TLOAM_E_HIP if none is usable.
 */
#ifndef TLOAM_HIP_H
#define TLOAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TLOAM_ABI_VERSION 8  /* 2: tloam_stats gained gn_sweeps; submap + feature entry points
                               * 3: tloam_set_source_frame / tloam_set_target_frame; tloam_stats.host_wait_us
                               * 4: tloam_get_normal_equations; tloam_comm_mailbox_*; tloam_stats.reserved0 ->
                               *    weight_range_violations (same slot), TLOAM_E_WEIGHT_RANGE is returned
                               * 5: tloam_frame_stash / tloam_frame_select (frames staged in HBM ahead of their solve)
                               * 6: tloam_k3_span, tloam_shard_ranges_frame
                               * 7: tloam_debug_raise_fault
                               * 8: tloam_get_info, tloam_gn_iter_timer, tloam_time_read_stream; a mailbox / RCCL set-up with nranks == 1
                               *    is a loop-back (the sharded forms run); a cloud holds at most 2^28 points (was 2^29) */

/* feature kinds; order = the builder order of registration.cpp:981-992 */
#define TLOAM_KIND_PLANAR 0 /* addSurfCostFactor    -> point-to-plane  */
#define TLOAM_KIND_GROUND 1 /* addGroundCostFactor  -> point-to-plane  */
#define TLOAM_KIND_EDGE 2   /* addEdgeCostFactor    -> point-to-line   */
#define TLOAM_KIND_SPHERE 3 /* addSphereCostFactor  -> point-to-point  */
#define TLOAM_NUM_KINDS 4

/* residual types of pre-built correspondence sets (tloam_set_correspondences) */
#define TLOAM_RES_PLANE 0 /* PointToPlaneErr registration.cpp:96-117  */
#define TLOAM_RES_LINE 1  /* PointToLineErr  registration.cpp:55-88   */
#define TLOAM_RES_POINT 2 /* PointToPointErr registration.cpp:19-47   */
#define TLOAM_NUM_RES 3

typedef enum tloam_status {
  TLOAM_OK = 0,
  TLOAM_E_INVALID = -1,        /* null pointer / bad enum / bad size                        */
  TLOAM_E_TOO_FEW_POINTS = -2, /* < 10 points in one of the 8 clouds (registration.cpp:928) */
  TLOAM_E_BAD_POSE = -3,       /* predict pose is not a rigid transform (sophus se3.hpp:497), or its translation is
                                  not finite (the reference goes on and returns a NaN pose)                  */
  TLOAM_E_HIP = -4,            /* HIP runtime error / no device                             */
  TLOAM_E_RCCL = -5,           /* RCCL error / librccl not loadable                         */
  TLOAM_E_NOT_READY = -6,      /* call sequence violated (e.g. outer step before begin)     */
  TLOAM_E_WEIGHT_RANGE = -7    /* a GNC weight left [0,1]: the reference's assert at :871, live in its build
                                * (CMakeLists.txt:5-6 set no NDEBUG).  Returned by tloam_sm_outer for the
                                * iteration it happened in and by tloam_scan_match AFTER the whole solve ran:
                                * result pose and stats are written, the weights are used as computed (what
                                * an NDEBUG build of the reference would do); the caller decides           */
} tloam_status;

/* The 16 keys of the `TLS:` block, config/mapping/lidar_odometry.yaml:23-39, read by
 * LocalRegistration::initConfig (registration.cpp:212-230). */
typedef struct tloam_tls_config {
  int32_t k_corr;     /* unused on the live path (only the dead PlaneToPlane builders) */
  int32_t factor_num; /* 2: planar+ground, 3: +edge, 4: +sphere (registration.hpp:144-148) */
  double edge_dist_thres;
  double edge_dir_thres;
  int32_t edge_maxnum;
  int32_t sphere_maxnum;
  double sphere_dist_thres;
  double planar_dist_thres;
  int32_t planar_maxnum;
  int32_t ground_maxnum;
  double ground_dist_thres;
  int32_t max_iterations;
  int32_t reserved0;
  double cost_threshold;
  double gnc_factor;
  double noise_bound;
  double fitness_thres;
} tloam_tls_config;

/* Fills *cfg with the shipped values of lidar_odometry.yaml:23-39. */
void tloam_default_config(tloam_tls_config* cfg);

/* What one scan_match (or one outer GNC iteration) did. */
typedef struct tloam_stats {
  int32_t outer_iterations;       /* GNC iterations executed (<= max_iterations)              */
  int32_t gn_evaluations;         /* solver evaluations (Ceres `Evaluate` calls of the minimiser) */
  int32_t gn_iterations;          /* trust-region iterations attempted (<= 4 per outer)       */
  int32_t accepted_steps;         /* ... of which accepted                                    */
  int32_t n_corr[TLOAM_NUM_KINDS];/* factors added in the LAST outer iteration, per kind      */
  int32_t converged_early;        /* 1 if the planar-cost plateau test broke the loop (:1108) */
  int32_t weight_range_violations;/* GNC weights that left [0,1] in this scan_match (the reference asserts, :871) */
  double kind_cost[TLOAM_NUM_KINDS]; /* side-channel cost sums of the last iteration (:1091-1094) */
  double mu;                      /* GNC mu after the last update (:1089)                      */
  double solver_cost;             /* Ceres-style cost 0.5*sum(rho) at the final iterate        */
  double se3[6];                  /* final tangent vector `parameters` (registration.hpp:328)  */
  int32_t gn_sweeps;              /* residual+Jacobian sweeps actually executed (K3 launches that did
                                   * work): <= gn_evaluations -- an evaluation of a point that is bit-identical
                                   * to the one just evaluated (a rejected step retried inside a halved trust
                                   * region) is served from the totals already on the device */
  int32_t host_wait_us;        /* microseconds of this scan_match the calling thread spent waiting for the device (0 in the oracle) */
} tloam_stats;

typedef struct tloam_ctx tloam_ctx;

/* ---- lifetime ------------------------------------------------------------------------ */
/* LocalRegistration::LocalRegistration(config["TLS"]) (registration.cpp:182-206). */
int tloam_create(const tloam_tls_config* cfg, int device_id, tloam_ctx** out);
void tloam_destroy(tloam_ctx* ctx);
int tloam_abi_version(void);
const char* tloam_status_string(int status);
/* text of the last HIP/RCCL error seen by this context ("" if none) */
const char* tloam_last_error(const tloam_ctx* ctx);

/* Sizes: a cloud, a correspondence set or a query batch holds at most 2^28 points (slots, cells and ranks are 32-bit integers on
 * the device, and the four kinds of a frame share one slot space); more is TLOAM_E_INVALID at the entry point. */
/* What a context is and what has happened to it -- read by the bench (so that a multi-GPU line says what it ran on), by the
 * co-residency test and by anybody who wants to know whether a context has left its fast forms. */
#define TLOAM_FALLBACK_SCAN 1   /* a single-pass look-back scan timed out: multi-launch scans from then on            */
#define TLOAM_FALLBACK_VOXEL 2  /* the voxel down-sampling's look-back timed out: start tickets from then on          */
#define TLOAM_FALLBACK_SOLVE 4  /* the one-launch Solve's in-launch hand-over timed out: one launch per GN iteration  */
typedef struct tloam_ctx_info {
  int32_t abi_version;
  int32_t device;
  int32_t device_cus;       /* hipDeviceAttributeMultiprocessorCount: what the forms that need all their blocks resident are sized by */
  int32_t comm_mode;        /* 0 one rank, 1 caller's all-reduce, 2 RCCL, 3 peer mailbox                               */
  int32_t rank, nranks;
  int32_t rccl_comm_count;  /* ncclCommCount of the context's communicator; -1: no RCCL communicator                    */
  int32_t rccl_comm_rank;   /* ncclCommUserRank; -1 likewise                                                            */
  int32_t fallbacks_taken;  /* TLOAM_FALLBACK_* bits: bounded in-launch waits that ran out and moved the context to a form
                             * that waits for nothing (knobs of the environment are not reported here)                  */
  int32_t fallback_events;  /* how many times that happened (each one cost a ~1-2 s wait and a re-run)                   */
  int32_t k3_grid;          /* blocks of the residual/Jacobian sweep over the current correspondence set (= rows it leaves) */
  int32_t k3_single;        /* 1: one wave per chunk (KITTI-size sets), 0: the streaming form                           */
  int32_t one_launch_solve; /* 1: a ceres::Solve on the current set runs as ONE launch (k_solve_all)                    */
  int32_t loopback;         /* 1: a mailbox / RCCL set-up with nranks == 1 -- the sharded launch forms run, the exchange is
                             * a loop-back                                                                               */
  int32_t direct_set;       /* 1: the frame in progress / the last one keeps its factors as a DIRECT set (large frames whose caps
                             * cannot bind: rows in the search's own order, no compaction -- DESIGN.md section 4)              */
  int32_t set_stale;        /* 1: ... and its rows will be rebuilt before a getter reads them (the loop ended beside a search
                             * that had already run)                                                                          */
  int32_t k3_wide;          /* 1: the streaming sweep goes out as blocks of EIGHT waves, one per CU (full-chip grids: half the rows
                             * for the block that folds them), 0: four waves                                                   */
} tloam_ctx_info;
int tloam_get_info(tloam_ctx* ctx, tloam_ctx_info* out);

/* The search grids of the context's LAST grid build, whichever call made it (tloam_scan_match / tloam_sm_begin,
 * tloam_set_target_frame, tloam_knn, the feature extraction) -- additive to ABI 8.  Read-only and host-side: nothing is
 * launched or waited for.  A kind that was not built has ncell = n = 0; a build that failed before its first launch leaves the
 * previous report.  Tests use it to know which build path they ran.
 * (tloam_knn keeps the grid it builds -- points, cell tables -- on the context until tloam_destroy, so a batch of queries
 * allocates nothing; a single call with a large radius over a large target pins that much memory.) */
#define TLOAM_GRID_SCAN_NONE 0        /* no build yet, or a build without a single cell                                     */
#define TLOAM_GRID_SCAN_SMALL 1       /* at most 16 Ki table entries: one block scans the 64-bit histogram                  */
#define TLOAM_GRID_SCAN_TILES 2       /* the frame-size path: 32-bit histogram, tile scan, finalize + scatter               */
#define TLOAM_GRID_SCAN_SINGLE_PASS 3 /* more than 1024 tiles, all blocks resident: one look-back launch, 64-bit histogram   */
#define TLOAM_GRID_SCAN_GENERIC 4     /* anything else: the multi-launch 64-bit scan                                         */
typedef struct tloam_grid_info {
  int32_t dim[TLOAM_NUM_KINDS][3];
  int32_t n[TLOAM_NUM_KINDS];      /* target points in the kind's grid                                                      */
  int64_t ncell[TLOAM_NUM_KINDS];
  double cell[TLOAM_NUM_KINDS];    /* edge of a cell: >= radius * (1 + 1e-6), grown by 1.25 per step while the kind's cells
                                    * exceed 4e6 or -- in a context whose caps admit no direct set -- max(16 Ki, 32 per point) */
  int32_t scan_path;               /* TLOAM_GRID_SCAN_*                                                                      */
  int32_t table_elem_bytes;        /* size of a histogram / scan entry on that path: 4 or 8 (0: no build)                     */
} tloam_grid_info;
int tloam_get_grid_info(tloam_ctx* ctx, tloam_grid_info* out);

/* ---- inputs: RegistrationInterface::setInputSource / setInputTarget -------------------
 * (registration.cpp:232-248).  The reference keeps shared_ptrs; here the cloud is copied
 * to HBM (AoS -> SoA on device).  In a sharded context (tloam_comm_*) every rank passes
 * the FULL cloud and the context keeps its contiguous index block.
 * Non-finite coordinates (NaN, +-inf) are taken as they are, like the reference takes them (it hands every point to nanoflann,
 * whose result set never admits a NaN / inf distance): such a SOURCE point is never matched -- it keeps its index and its
 * weight of 1 --, such a TARGET point is never anybody's neighbour and does not extend the search grid.  No status is raised;
 * the result is the reference's (tests/test_gpu_parity.py::test_non_finite_points_are_never_matched). */
int tloam_set_source(tloam_ctx* ctx, int kind, const double* xyz_aos, size_t n);
int tloam_set_target(tloam_ctx* ctx, int kind, const double* xyz_aos, size_t n);
/* The same for the four clouds of a tloam::Frame at once (registration_interface.hpp:19-38; setInputSource /
 * setInputTarget take a Frame, registration.cpp:232-248), indexed by TLOAM_KIND_*.  xyz_aos[k] may be NULL when n[k] == 0.
 * tloam_set_target_frame synchronises once per frame instead of once per cloud, then enqueues the build of the four search
 * grids over the new targets without waiting for it (the next tloam_scan_match / tloam_sm_begin uses them; until then the
 * context's search structures -- what tloam_fitness sees -- remain those of the last scanMatching).  tloam_set_source_frame does not wait for the
 * device at all: it returns when the borrowed buffers have been copied OUT (into pinned staging; one copy is enqueued on the
 * context's stream behind it), so they may be reused at once and the next call on the context is ordered behind the copy.
 * SHARDED contexts: the four source clouds of a frame must reach EVERY rank through the SAME entry point -- all four through
 * tloam_set_source_frame (the frame is cut as one line, tloam_shard_ranges_frame: a rank holds one or two kinds and builds only
 * those kinds' search grids) or each through tloam_set_source (every cloud cut by itself, tloam_shard_range) -- never a mix
 * within a frame, and the same choice on all ranks: the two rules give a rank different index blocks, and a mix leaves source
 * points unowned or owned twice.  A kind a rank holds no source points of has no search structure on that rank
 * (tloam_fitness skips it there). */
int tloam_set_source_frame(tloam_ctx* ctx, const double* const xyz_aos[4], const size_t n[4]);
int tloam_set_target_frame(tloam_ctx* ctx, const double* const xyz_aos[4], const size_t n[4]);
/* Frames staged ahead of their solve.  The reference's caller hands a Frame over and solves it at once (front_end.cpp:314,
 * :321); a caller that receives scans while the previous solve is still running -- or a replay / benchmark that wants its
 * frames resident in HBM before the clock starts -- can hand frames over early and activate them later at no cost:
 *   tloam_frame_stash(ctx, slot)   moves the clouds currently registered with the context (whatever tloam_set_source* /
 *                                  tloam_set_target* left there: eight clouds, their bounds) into slot `slot` (>= 0) of a frame
 *                                  store kept in HBM; the context is left without registered clouds.  A slot that was in
 *                                  use is overwritten.  Stashing the slot that is currently selected keeps the frame in
 *                                  that slot (including what tloam_set_* wrote since) and makes the context's own clouds
 *                                  the registered ones again (= select -1); with ANOTHER slot selected: TLOAM_E_NOT_READY.
 *   tloam_frame_select(ctx, slot)  makes the clouds of `slot` the registered ones (buffers are exchanged, nothing is copied or
 *                                  synchronised); slot -1 = back to the context's own.  While a slot is selected,
 *                                  tloam_set_source* / tloam_set_target* write into that slot's frame.
 * TLOAM_E_NOT_READY between tloam_sm_begin and tloam_sm_end, TLOAM_E_INVALID for an unknown slot. */
int tloam_frame_stash(tloam_ctx* ctx, int slot);
int tloam_frame_select(tloam_ctx* ctx, int slot);

/* ---- RegistrationInterface::scanMatching (registration.cpp:879-1133) -------------------
 * predict/result: 4x4 column-major.  omega_perturb3: the unit vector the reference draws
 * with Eigen::Vector3d::Random() when |omega| < 1e-2 (:884-886); NULL = (0,0,1).
 * scan_xyz_aos/n_scan: optional cloud transformed IN PLACE by the result pose
 * (out_result_.scan_cloud, :1126-1128); NULL/0 to skip.  stats may be NULL. */
int tloam_scan_match(tloam_ctx* ctx, const double predict_colmajor[16],
                     const double* omega_perturb3_or_null, double result_colmajor[16],
                     double* scan_xyz_aos_or_null, size_t n_scan, tloam_stats* stats);

/* The same, one outer GNC iteration at a time (tests inspect the state in between).
 * begin -> outer x N (until *done) -> end. */
int tloam_sm_begin(tloam_ctx* ctx, const double predict_colmajor[16],
                   const double* omega_perturb3_or_null);
int tloam_sm_outer(tloam_ctx* ctx, int* done, tloam_stats* stats);
int tloam_sm_end(tloam_ctx* ctx, double result_colmajor[16], tloam_stats* stats);

/* ---- RegistrationInterface::getFitnessScore (registration.cpp:257-296) ----------------- */
int tloam_fitness(tloam_ctx* ctx, double* fitness, double* rmse);

/* ---- introspection (parity tests) ------------------------------------------------------
 * Correspondences built by the last outer iteration for `kind`, in source-index order.
 * src_index[n]; a[3n] = plane normal | line point a | target point; b[3n] = line point b
 * (edge only; else untouched); d[n] = plane offset (planar/ground only); w[n] = weight
 * captured at build time; cost[n] = side-channel cost after the last sweep.  Any output
 * pointer may be NULL.  capacity = elements available; returns count via *n. */
int tloam_get_correspondences(tloam_ctx* ctx, int kind, size_t capacity, size_t* n,
                              int32_t* src_index, double* a_aos, double* b_aos, double* d,
                              double* w, double* cost);
/* current per-source-point GNC weights of `kind` (this rank's block if sharded) */
int tloam_get_weights(tloam_ctx* ctx, int kind, size_t capacity, size_t* n, double* w);
/* exact hybrid search on the device structure of `kind` (KDTreeFlann::SearchHybrid, B.2):
 * for each of nq queries (AoS) the k nearest targets with squared distance < radius^2,
 * ascending; out_idx[nq*k] (-1 padded), out_d2[nq*k], out_cnt[nq]. */
int tloam_knn(tloam_ctx* ctx, int kind, const double* queries_aos, size_t nq, double radius,
              int k, int32_t* out_idx, double* out_d2, int32_t* out_cnt);

/* ---- pre-built correspondence sets (roofline / parity of K3 and the solver) ------------
 * res_type TLOAM_RES_*: p = source point (scan frame); a = normal | line a | target;
 * b = line b (LINE only, else NULL); d = plane offset (PLANE only, else NULL); w = weights.
 * Replaces whatever the builders produced.  Sharded contexts keep their index block. */
int tloam_set_correspondences(tloam_ctx* ctx, int res_type, size_t n, const double* p_aos,
                              const double* a_aos, const double* b_aos, const double* d,
                              const double* w);
/* One residual+Jacobian sweep at se3 (K3): H = sum rho' J^T J (row-major 6x6),
 * g = sum rho' J^T r, cost = sum 0.5*log(1+|r|^2)  (Ceres evaluator + CauchyLoss(1.0)
 * corrector, registration.cpp:970).  Also refreshes the side-channel costs.  In a sharded
 * context the outputs are the all-reduced totals. */
int tloam_accumulate(tloam_ctx* ctx, const double se3[6], double H_rowmajor[36], double g[6],
                     double* cost);
/* Parity probe of the per-outer-iteration linear system: the robustified normal equations the minimiser
 * held when its last Solve returned -- H = sum rho' J^T J (row-major 6x6), g = sum rho' J^T r, and the cost
 * 0.5 sum rho, all at the ACCEPTED iterate (tloam_stats.se3).  In a sharded context: the all-reduced totals. */
int tloam_get_normal_equations(tloam_ctx* ctx, double H_rowmajor[36], double g[6], double* cost);
/* side-channel costs of the current set, per residual type (after tloam_accumulate/solve) */
int tloam_get_costs(tloam_ctx* ctx, int res_type, size_t capacity, size_t* n, double* cost);
/* One ceres::Solve as configured at registration.cpp:1036-1047 on the current set:
 * se3_inout is `parameters`.  stats->gn_* filled. */
int tloam_solve(tloam_ctx* ctx, double se3_inout[6], tloam_stats* stats);
/* Timing helper for the bench: `launches` back-to-back K3 sweeps at se3 on the context's
 * stream bracketed by HIP events; returns the mean kernel-pair time in microseconds. */
int tloam_time_accumulate(tloam_ctx* ctx, const double se3[6], int launches, double* mean_us);
/* Timing helper for the bench: `launches` back-to-back runs of the correspondence-search kernel (K1 + K2:
 * SearchHybrid + the four builders, registration.cpp:427-635, :714-778) over the source points of the last
 * scan_match -- same pose, grids and query order -- between one HIP event pair; *queries = points searched. */
int tloam_time_build(tloam_ctx* ctx, int launches, double* mean_us, int64_t* queries);
/* Sharded contexts, collective (every rank calls it with the same arguments): `launches` sweeps over this rank's
 * block of the current set, each followed -- with_exchange != 0 -- by the exchange of the 48 doubles exactly as a GN
 * iteration performs it (mailbox: posted by the sweep's last block and gathered by a one-wave kernel; RCCL / callback:
 * all-reduce), one HIP event pair around the lot.  The difference with / without is the latency the exchange adds. */
int tloam_time_sharded_sweep(tloam_ctx* ctx, const double se3[6], int launches, int with_exchange, double* mean_us);
/* accumulated HIP-event time (us) and launch count of the K3 sweeps since the last reset; the first
 * call arms the timer: each K3 dispatch then carries a HIP start/stop event pair bound to the
 * dispatch packet (hipExtLaunchKernelGGL), i.e. the elapsed time is the kernel duration itself */
int tloam_k3_timer(tloam_ctx* ctx, int reset, double* total_us, int64_t* launches,
                   double* algorithmic_bytes);
/* the same over EVERY K3 launch, including the no-op launches enqueued after a solver tolerance exit
 * (the population a kernel trace averages over) */
int tloam_k3_timer_all(tloam_ctx* ctx, double* total_us, int64_t* launches);
/* One-launch GN iterations of large sets (k3_sweep_step: sweep + row fold + minimiser step in one dispatch): the STREAMING
 * span of those launches -- first wave in to last block row out, by the device's 100 MHz wall clock, without the serial
 * tail -- accumulated on the device since the last reset; synchronises the stream.  launches counts working sweeps only
 * (a launch that finds the Solve finished returns before the span is taken). */
int tloam_k3_span(tloam_ctx* ctx, int reset, double* total_us, int64_t* launches);
/* The period of a GN iteration (sweep + reduction + exchange + 6x6 step + pose update) as the DEVICE clocks it:
 * every kernel that ends an iteration stamps the 100 MHz wall clock when its step is done, and the time between two consecutive
 * stamps of ONE Solve is added up -- launch boundaries, fold, exchange and step included; a Solve's first iteration has no stamp
 * to start from and is not counted.  The first call arms the counter (until then the kernels skip it); synchronises the stream. */
int tloam_gn_iter_timer(tloam_ctx* ctx, int reset, double* total_us, int64_t* iterations);
/* On-box bandwidth of a READ stream with the sweep's access pattern (eight fp64 streams, 16-byte loads, persistent waves, two
 * blocks per CU): `launches` passes over ~`bytes`, one HIP event pair; *gbps = bytes read / s / 1e9.  bytes >> 256 MiB: from HBM;
 * bytes = a sweep's 75 MB: from the Infinity Cache, as the sweeps of a Solve.  Allocates and frees its own buffer. */
int tloam_time_read_stream(tloam_ctx* ctx, size_t bytes, int launches, double* gbps);
/* Test aid: the DEVICE SE(3) arithmetic the minimiser step uses (vendored-Sophus restatements sophus/so3.hpp:583-619,
 * se3.hpp:761-785 exp; so3.hpp:247-290, se3.hpp:223-256 log; registration.cpp:162-173 Plus), n items.  out26 per item:
 * [0..6] exp(delta) as (qw qx qy qz tx ty tz), [7..12] log(exp(x)), [13..18] Plus(x, delta), [19..25] exp(x) (shared form). */
int tloam_debug_se3(tloam_ctx* ctx, int n, const double* x6, const double* delta6, double* out26);
/* debugging aid: raw copy of the device-resident minimiser state; returns its size in doubles */
int tloam_debug_state(tloam_ctx* ctx, double* out, int n_doubles);
/* development aid: the per-block partial rows of the last K3 launch (32 doubles per block); returns the
 * number of rows.  Columns 28..31 carry in-kernel timestamps in builds with -DTLOAM_K3_PROFILE. */
int tloam_debug_partials(tloam_ctx* ctx, double* out, int n_doubles);
/* Test hook.  A few kernels spin on blocks of their own launch (the single-pass look-back scans of 1 M-class tables, the
 * voxel down-sampling's look-back); the host only picks those forms where the device's CU count says every block is
 * resident at once, their waits are bounded (~1 s) all the same, and a wait that runs out raises a word in pinned host
 * memory: the call in progress returns TLOAM_E_HIP -- tloam_scan_match runs the frame again by itself -- and the context
 * uses the forms that wait for nothing (multi-launch scans / start tickets) from then on.  This raises the word by hand:
 * which = 0 look-back scan, 1 voxel down-sampling. */
int tloam_debug_raise_fault(tloam_ctx* ctx, int which);

/* ---- submap maintenance on the device ---------------------------------------
 * FrontEnd::updateSubmap (front_end.cpp:201-275) and the first-frame branch of updateLidarOdometry
 * (front_end.cpp:283-304) restated on the device, so that the four target clouds never leave HBM between
 * frames: Transform (PointCloud2.cpp:71-75) -> += (:96-132) -> Crop (:551-559) -> VoxelDownSample (:358-403).
 * The result is installed as the registration target (the reference's setInputTarget(submap),
 * front_end.cpp:267) without a host round trip.  Quirk kept: the sphere submap is rebuilt from the PLANAR
 * frame buffer (front_end.cpp:221 iterates submap_planar_buffer).  Voxels are emitted in order of first
 * occurrence (the reference's order is std::unordered_map's, i.e. unspecified). */
typedef struct tloam_submap_config {
  int32_t planar_frame_size;        /* lidar_odometry.yaml:13  (3)   */
  int32_t sphere_frame_size;        /* lidar_odometry.yaml:12  (3)   */
  double edge_crop_box_length;      /* lidar_odometry.yaml:16  (100) */
  double ground_crop_box_length;    /* lidar_odometry.yaml:17  (100) */
  double edge_down_sample_submap;   /* lidar_odometry.yaml:9   (0.3) */
  double ground_down_sample_submap; /* lidar_odometry.yaml:7   (0.45)*/
  double ground_down_sample;        /* lidar_odometry.yaml:6   (0.3), first frame only (front_end.cpp:287) */
} tloam_submap_config;
void tloam_submap_default_config(tloam_submap_config* cfg);
/* first frame (front_end.cpp:283-304): edge += edge cloud; ground += ground cloud->VoxelDownSample(
 * ground_down_sample); planar / sphere += the submap selections; setInputTarget(submap). */
int tloam_submap_init(tloam_ctx* ctx, const tloam_submap_config* cfg, const double* planar_submap_xyz, size_t n_planar,
                      const double* sphere_submap_xyz, size_t n_sphere, const double* edge_xyz, size_t n_edge,
                      const double* ground_xyz, size_t n_ground);
/* every later frame (front_end.cpp:201-275) with lidar_odom_pose = pose_colmajor: planar/sphere frame
 * buffers, edge/ground accumulate -> crop around the pose's translation -> voxel grid; setInputTarget.
 * The pose is taken as Open3D's Transform takes a 4x4 (no orthogonality test on this path: a scaled rotation or a projective
 * last row is applied as it stands); a NaN or an infinity anywhere in it is TLOAM_E_BAD_POSE and leaves the submap as it was
 * (the reference would go on with NaN clouds).  TLOAM_E_NOT_READY before tloam_submap_init. */
int tloam_submap_update(tloam_ctx* ctx, const double pose_colmajor[16], const double* planar_submap_xyz,
                        size_t n_planar, const double* sphere_submap_xyz, size_t n_sphere,
                        const double* edge_scan_xyz, size_t n_edge, const double* ground_scan_xyz, size_t n_ground);
/* the target cloud of `kind` as the device holds it (AoS out); n receives the size even when capacity is
 * too small (then nothing is copied and TLOAM_E_INVALID is returned) */
int tloam_get_target(tloam_ctx* ctx, int kind, size_t capacity, size_t* n, double* xyz_aos);


/* ---- PCA feature extraction on the device ------------------------------------
 * featureExtract::calculatePCAInfo (src/models/feature_extraction/feature_extract.cpp:47-122) and
 * featureExtract::extractPlanarSphere (:133-197): hybrid k-NN (r, K) of every point in its own cloud,
 * 3x3 covariance from nine cumulants, ascending eigen decomposition, cvr / flatness / sphericity, then the
 * planar / sphere candidate lists ranked by flatness (descending; ties by ascending index -- the reference's
 * std::sort is unstable there).  Quirks kept: the sphere lists are ranked by FLATNESS (:162) and hold sort
 * RANKS, not point indices (:186,:188).  K <= 20. */
typedef struct tloam_feature_config {
  double radius;               /* feature.yaml: radius 0.2 */
  int32_t K;                   /* 20 */
  int32_t min_neigh;           /* 10 */
  int32_t planar_num;          /* 500 */
  int32_t sphere_num;          /* 300 */
  double cvr_scan;             /* 0.25 */
  double cvr_submap;           /* 0.15 */
  double planar_scan_thres;    /* 0.75 */
  double planar_submap_thres;  /* 0.65 */
  double planar_vertic_thres;  /* 0.25 */
} tloam_feature_config;
void tloam_feature_default_config(tloam_feature_config* cfg);
/* per-point PCAInfo (feature_extract.hpp:33-39); any output pointer may be NULL.  Points that are skipped
 * (no more than min_neigh neighbours) keep the value-initialised zeros of the reference; neigh_index is
 * n x K, padded with -1.  radius >= 0 and 3 <= K <= 20, else TLOAM_E_INVALID (assert(r_ >= 0.0 && K_ >= 3),
 * feature_extract.cpp:55): a radius of exactly 0 finds nobody, an infinite one is plain k-NN; a cloud without a single finite
 * point has no search structure and every point keeps the zeros. */
int tloam_pca_info(tloam_ctx* ctx, const tloam_feature_config* cfg, const double* xyz_aos, size_t n,
                   double* flatness, double* cvr, double* sphericity, double* normal_aos, int32_t* num_sum,
                   int32_t* neigh_index);
/* the four index lists of extractPlanarSphere; each output array must hold n entries */
int tloam_extract_planar_sphere(tloam_ctx* ctx, const tloam_feature_config* cfg, const double* xyz_aos, size_t n,
                                int32_t* planar_scan_index, size_t* n_planar_scan, int32_t* planar_submap_index,
                                size_t* n_planar_submap, int32_t* sphere_scan_index, size_t* n_sphere_scan,
                                int32_t* sphere_submap_index, size_t* n_sphere_submap);

/* ---- segmentation node on the device (additive to ABI 8) -----------------------------------------
 * Segmentation::spinOnce (src/models/segmentation/segmentation.cpp:40-93): near / non-finite filter, rings, height split,
 * regional ground fit, DCVC clustering, edge / general extraction -- one raw scan in, what the node publishes out, as index
 * lists into the caller's array in the reference's output order (DESIGN.md section 11 declares the orders the reference
 * leaves open, and its one deviation: DCVC clusters are the connected components of its neighbour edges taken as
 * undirected).  Only sensor_model 64 and quadrant 4 are supported (TLOAM_E_INVALID otherwise). */
typedef struct tloam_seg_config {
  /* velodyne: */
  int32_t sensor_model;        /* 64 */
  int32_t reserved0;
  double scan_period;          /* 0.1 (unused by the stage) */
  double sensor_height;        /* 1.73 */
  double vertical_res;         /* 0.4 */
  double init_angle;           /* -24.9 */
  double sensor_min_range;     /* 1.0 */
  double sensor_max_range;     /* 120.0 */
  double near_dis;             /* 3.0 (points closer than near_dis^2 = 9 m are dropped, :485) */
  /* groundSeg: */
  int32_t quadrant;            /* 4 */
  int32_t num_sec;             /* 3 */
  double dis;                  /* 0.3 */
  int32_t max_iter;            /* 3 */
  int32_t ground_seed_num;     /* 20 */
  int32_t ring_min_num;        /* 131 */
  int32_t reserved1;
  /* DCVC: */
  double start_r;              /* 0.35 */
  double delta_r;              /* 0.0004 */
  double delta_p;              /* 1.2 */
  double delta_a;              /* 1.2 */
  int32_t min_seg;             /* 80 */
  int32_t reserved2;
} tloam_seg_config;
void tloam_seg_default_config(tloam_seg_config* cfg);
/* One scan (AoS, firing order).  Every output may be NULL; the index arrays hold up to n entries, boxes up to
 * box_capacity x 6 doubles (centre xyz, dimensions xyz per kept cluster, in label order; *n_boxes is the cluster count).
 * ring[n]: beam id per input point, -1 where the first filter removed it.  object_index: object_scan before clustering.
 * segmented_label: the 1-based rank of the point's cluster.  The context counts its calls: the first one starts DCVC's
 * minPolar / maxPolar at 5.0, every later one at 0.0 (the reference's header value, then resetParams).
 * TLOAM_E_TOO_FEW_POINTS when object_scan is empty or no cluster survives (the node publishes nothing): the counts of the
 * stages that completed are written, the rest are 0; the call still counts as a frame. */
int tloam_segment(tloam_ctx* ctx, const tloam_seg_config* cfg, const double* xyz_aos, size_t n, int32_t* ring,
                  int32_t* ground_index, size_t* n_ground, int32_t* object_index, size_t* n_object,
                  int32_t* segmented_index, int32_t* segmented_label, size_t* n_segmented, int32_t* edge_index,
                  size_t* n_edge, int32_t* general_index, size_t* n_general, double* boxes, size_t box_capacity,
                  size_t* n_boxes);

/* ---- per-scan voxel grid and the whole odometry frame on the device (additive to ABI 8) ----------
 * tloam_voxel_down_sample: PointCloud2::VoxelDownSample (PointCloud2.cpp:358-403) of one cloud -- bounds = the cloud's
 * min / max -+ voxel / 2, every occupied voxel emits the mean of its points (summed in index order), voxels in order of first
 * occurrence (the order the submap path declares).  *n_out receives the size even when capacity is too small (then nothing is
 * copied and TLOAM_E_INVALID is returned).  voxel <= 0 and "voxel_size is too small" (a voxel index beyond 2^21 on an axis)
 * are TLOAM_E_INVALID, as in tloam_submap_*. */
int tloam_voxel_down_sample(tloam_ctx* ctx, double voxel, const double* xyz_aos, size_t n, double* out_aos, size_t capacity,
                            size_t* n_out);

/* FrontEnd (front_end.cpp:181-199, :278-337) fed by Segmentation::spinOnce: the stage configurations of the shipped yaml files
 * (segmentation.yaml, feature.yaml, lidar_odometry.yaml) and the one key the frame adds, edge_down_sample
 * (lidar_odometry.yaml:8).  The per-scan ground voxel is submap.ground_down_sample (lidar_odometry.yaml:6). */
typedef struct tloam_odom_config {
  tloam_seg_config seg;
  tloam_feature_config feature;
  tloam_submap_config submap;
  double edge_down_sample;     /* 0.1 */
} tloam_odom_config;
void tloam_odom_default_config(tloam_odom_config* cfg);

/* What one tloam_odometry_frame did.  Cloud sizes are those of the frame's stages (0 where a stage did not run).
 * h2d_bytes / d2h_bytes / host_syncs count the copy commands and host waits of the frame's own stages around the scan match
 * (the match's own traffic is that of tloam_scan_match and is not counted): DESIGN.md section 12. */
typedef struct tloam_odom_stats {
  tloam_stats match;           /* the scan match of the frame (zero on the first frame) */
  int64_t frame;               /* frames accepted since the reset before this one: 0 = the first frame */
  int64_t n_ground, n_edge, n_general;     /* segmentation: /ground_points, /edge_points, /general_points */
  int64_t n_edge_ds, n_ground_ds;          /* processCloud's VoxelDownSample of edge (edge_down_sample) and ground */
  int64_t n_planar_scan, n_sphere_scan, n_planar_submap, n_sphere_submap;   /* extractPlanarSphere's selections */
  int64_t h2d_bytes, d2h_bytes, host_syncs;
} tloam_odom_stats;

/* FrontEnd::setInitPose plus a fresh odometry state: the next frame is the first one.  cfg NULL: the defaults; init NULL:
 * identity.  TLOAM_E_INVALID for a configuration a stage refuses or a non-finite init pose. */
int tloam_odometry_reset(tloam_ctx* ctx, const tloam_odom_config* cfg, const double init_pose_colmajor[16]);
/* One raw scan (AoS, firing order) -> the pose of FrontEnd::updateLidarOdometry.  First frame after a reset: segment, PCA,
 * tloam_submap_init(planar submap selection, sphere submap selection, raw edge, raw ground); the pose is the init pose.  Later
 * frames: segment, processCloud (voxel ground / edge, PCA, selections), source frame, scan match from the constant-velocity
 * prediction, tloam_submap_update.  Only the raw scan crosses to the device; every other cloud stays in HBM.
 * TLOAM_E_TOO_FEW_POINTS: segmentation published nothing, or a cloud the frame hands on (the four source clouds and four
 * targets of the match; on the first frame the four submap clouds) has fewer than 10 points -- the frame is skipped and the
 * odometry state (poses, submap, frame index) is unchanged.  TLOAM_E_WEIGHT_RANGE as tloam_scan_match: pose and stats are
 * written and the frame counts.  TLOAM_E_NOT_READY before tloam_odometry_reset; TLOAM_E_INVALID on a context with nranks > 1.
 * Afterwards tloam_get_target / tloam_fitness / tloam_get_correspondences / tloam_get_weights describe this frame. */
int tloam_odometry_frame(tloam_ctx* ctx, const double* xyz_aos, size_t n, double pose_out_colmajor[16],
                         tloam_odom_stats* stats);

/* ---- the global map and the registered scan of the odometry frame (additive to ABI 8) --------------
 * FrontEnd::updateSubmap's mapping branch (front_end.cpp:269-274): with mapping on, every later frame appends
 * VoxelDownSample(raw.Transform(pose), voxel) to a map kept in HBM (the first frame returns at :304, before updateSubmap, and
 * appends nothing).  Voxels in order of first occurrence, means summed in index order (as tloam_voxel_down_sample); non-finite
 * returns are left out.  A frame whose transformed scan puts a voxel index beyond 2^21 on an axis appends nothing and counts in
 * overflow_frames; its pose is not affected.  DESIGN.md section 13. */
typedef struct tloam_map_config {
  int32_t enabled;         /* mapping_flag (lidar_odometry.yaml:21): 0 */
  int32_t reserved0;
  double voxel;            /* 1.0 (front_end.cpp:272) */
  int64_t reserve_points;  /* points of HBM reserved when enabled; 0 = 2^21 (48 MiB); the map grows past it by doubling */
} tloam_map_config;
void tloam_map_default_config(tloam_map_config* cfg);
/* cfg NULL: the defaults.  Empties the map; the configuration persists across tloam_odometry_reset.  Allowed between frames.
 * voxel <= 0 (or not finite) or reserve_points < 0: TLOAM_E_INVALID.  Disabling releases the map's device memory. */
int tloam_map_configure(tloam_ctx* ctx, const tloam_map_config* cfg);

typedef struct tloam_map_info {
  int64_t n_points;                /* points in the map */
  int64_t n_frames;                /* frames that appended since the last reset / configure */
  int64_t last_first, last_count;  /* the newest appending frame's span in the map */
  int64_t capacity_points;         /* points the map holds before it grows */
  int64_t overflow_frames;         /* frames whose scan left the voxel grid: appended nothing */
} tloam_map_info;
int tloam_map_get_info(tloam_ctx* ctx, tloam_map_info* info);
/* points [first, first + count) of the map, AoS.  A range beyond n_points: TLOAM_E_INVALID. */
int tloam_map_read(tloam_ctx* ctx, size_t first, size_t count, double* out_aos);
/* The raw scan of the last accepted frame transformed by its lidar_odom_pose (front_end.cpp:84-86, /raw_cloud) -- identity on
 * the first frame, whatever the init pose (front_end.hpp:106).  With mapping on it is what the map stage transformed; with
 * mapping off the resident scan is transformed now.  *n receives the size even when capacity is too small (then nothing is
 * copied and TLOAM_E_INVALID is returned).  TLOAM_E_NOT_READY before the first accepted frame, and once the scan is no longer
 * resident: a later call on the context (tloam_segment, a skipped frame) has overwritten the segmentation's input buffer and
 * the map stage holds no transformed copy of it. */
int tloam_registered_scan(tloam_ctx* ctx, size_t capacity, size_t* n, double* out_aos);
/* Every map call on a context with nranks > 1: TLOAM_E_INVALID, as the frame. */

/* ---- the merged voxel map of the odometry frame (additive to ABI 8; nothing in the reference) --------------
 * One voxel grid for the whole run, origin o and voxel v fixed by the configuration; each occupied voxel keeps the count N and
 * the int64 sums Q of the quantised offsets of every return that ever fell in it.  The frames that add are those that append
 * to the tloam_map_* map when it is on (accepted later frames); their input is the registered scan (tloam_registered_scan's
 * doubles), non-finite returns left out.  Per point and axis: s = (p - o) / v, i = (int64) floor(s),
 * q = (int64) floor((s - i) * 2^24 + 0.5) in [0, 2^24].  A frame with |i| >= 2^20 on an axis for any finite point adds
 * nothing and counts in overflow_frames; its pose is not affected.  Centroid per axis:
 * c = o + v * ((double) i + ((double) Q / (double) N) * 2^-24) -- within v * 2^-25 of the mean before its last rounding.
 * Voxel ids in order of creation; a frame's new voxels in order of their smallest point index in its scan.  DESIGN.md 14. */
typedef struct tloam_voxel_map_config {
  int32_t enabled;          /* 0 */
  int32_t reserved0;
  double voxel;             /* v: 1.0 */
  double origin[3];         /* o: (0, 0, 0) */
  int64_t reserve_voxels;   /* voxels of HBM reserved when enabled; 0 = 2^20; grows past it by doubling */
} tloam_voxel_map_config;
void tloam_voxel_map_default_config(tloam_voxel_map_config* cfg);
/* cfg NULL: the defaults.  Empties the map; the configuration persists across tloam_odometry_reset (which empties the map).
 * voxel <= 0 or not finite, a non-finite origin or reserve_voxels < 0: TLOAM_E_INVALID.  Disabling releases its device memory. */
int tloam_voxel_map_configure(tloam_ctx* ctx, const tloam_voxel_map_config* cfg);

typedef struct tloam_voxel_map_info {
  int64_t n_voxels;          /* occupied voxels */
  int64_t n_points;          /* returns in them: the sum of N */
  int64_t n_frames;          /* frames that added since the last reset / configure */
  int64_t last_new;          /* voxels the newest adding frame created */
  int64_t capacity_voxels;   /* voxels the map holds before it grows */
  int64_t overflow_frames;   /* frames whose scan left the grid: added nothing */
} tloam_voxel_map_info;
int tloam_voxel_map_get_info(tloam_ctx* ctx, tloam_voxel_map_info* info);
/* voxels [first, first + count) in id order: centroids AoS and counts N.  Either output may be NULL.  A range beyond n_voxels:
 * TLOAM_E_INVALID. */
int tloam_voxel_map_read(tloam_ctx* ctx, size_t first, size_t count, double* centroids_aos, int64_t* counts);
/* The voxels whose centroid lies in [lo, hi] on every axis (inclusive) and whose N >= min_count, in id order.  *n receives the
 * size even when capacity is too small (then nothing is copied and TLOAM_E_INVALID is returned).  Either output may be NULL. */
int tloam_voxel_map_read_box(tloam_ctx* ctx, const double lo[3], const double hi[3], int64_t min_count, size_t capacity,
                             size_t* n, double* centroids_aos, int64_t* counts);
/* Every voxel map call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- deskew of the odometry frame's scan under constant velocity (additive to ABI 8) ---------------
 * A spinning sensor sweeps for one scan_period; every return is in the sensor frame of its own firing time.  With deskew on, a
 * frame corrects its scan with the motion xi = log(step), step = last_pose^-1 * lidar_odom_pose as stored when the previous
 * frame was accepted (identity until the second frame has been accepted): return i, at sweep time s_i (in frame intervals,
 * relative to the pose's instant), becomes p'_i = exp(s_i xi) p_i.
 *   azimuth mode:  s_i = wrap_[0,2pi)(direction * (atan2(y, x) - start_azimuth)) / 2pi - ref_fraction
 *   timed mode:    s_i = t_i / cfg.seg.scan_period, t_i in seconds relative to the pose's instant (tloam_odometry_frame_timed)
 * A return with a non-finite coordinate, or with s_i == 0, is copied bit for bit.  A frame whose step is bitwise the identity
 * corrects nothing and equals a frame with deskew off.  Segmentation runs on the raw scan; its index lists take the corrected
 * coordinates, and so do the registered scan, the global map and the merged voxel map.  DESIGN.md 15. */
typedef struct tloam_deskew_config {
  int32_t enabled;         /* 0 */
  int32_t time_source;     /* 0 azimuth, 1 per-point times (tloam_odometry_frame_timed) */
  int32_t direction;       /* +1 counter-clockwise seen from +z (the order the q4 -> q1 ring step implies), -1 clockwise */
  int32_t reserved0;
  double start_azimuth;    /* rad: 0 */
  double ref_fraction;     /* azimuth mode: the sweep fraction the pose describes: 0 */
} tloam_deskew_config;
void tloam_deskew_default_config(tloam_deskew_config* cfg);
/* cfg NULL: the defaults.  Non-finite values, direction not +-1, an unknown time_source: TLOAM_E_INVALID.  Persists across
 * tloam_odometry_reset; clears the info below. */
int tloam_deskew_configure(tloam_ctx* ctx, const tloam_deskew_config* cfg);

typedef struct tloam_deskew_info {
  int64_t frames_deskewed;       /* accepted frames whose scan was corrected, since the last reset / configure */
  int64_t last_frame;            /* the frame number of the last of them (tloam_odom_stats.frame), -1 none */
  double last_twist[6];          /* its xi = (upsilon, omega), Sophus order */
  double last_max_shift;         /* its max |p' - p| over the finite returns, m */
  double next_motion_colmajor[16];   /* the step the next frame takes xi from */
} tloam_deskew_info;
int tloam_deskew_get_info(tloam_ctx* ctx, tloam_deskew_info* info);

/* tloam_odometry_frame with per-point times t_sec[n] (seconds, relative to the pose's instant); deskew must be configured with
 * time_source 1.  A non-finite time or |t_i / scan_period| > 2 refuses the frame with TLOAM_E_INVALID and leaves the odometry
 * state unchanged.  t_sec NULL, or deskew off / in azimuth mode: TLOAM_E_INVALID; so is tloam_odometry_frame in timed mode. */
int tloam_odometry_frame_timed(tloam_ctx* ctx, const double* xyz_aos, const double* t_sec, size_t n,
                               double pose_out_colmajor[16], tloam_odom_stats* stats);
/* The correction alone, on the device, with the frame's kernel: motion is the step (a rigid transform; xi = its log), t_sec NULL
 * in azimuth mode.  cfg->enabled is not looked at.  In timed mode a bad time is TLOAM_E_INVALID (out_aos then undefined). */
int tloam_deskew_scan(tloam_ctx* ctx, const tloam_deskew_config* cfg, double scan_period, const double motion_colmajor[16],
                      const double* xyz_aos, const double* t_sec, size_t n, double* out_aos);
/* Every deskew call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- place recognition: Scan Context keyframes and loop search on the device (additive to ABI 8) ----
 * Off by default; when off, every frame, stat, map and launch is what it is without it.  With it on, an accepted odometry frame
 * is a keyframe when it is the first since the reset / configure, or when its returned pose has moved >= kf_dist or turned
 * >= kf_angle (the angle of the relative rotation) from the last keyframe's pose.  A keyframe stores the Scan Context
 * descriptor of the scan the frame used (the deskewed copy when deskew corrected it), both keys, the pose and the frame number
 * (tloam_odom_stats.frame), and is searched against keyframes 0 .. q - exclude_recent: the num_candidates nearest ring keys,
 * then every column shift of each; the best pair (min d, ties to the lower shift, then the lower keyframe) with d < dist_thres
 * is a loop record.  Descriptor: n_rings x n_sectors fp64, row-major by ring; bin = max(z + height_offset) over the finite
 * returns with 0 < r < max_radius (r = sqrt(x*x + y*y)), ring = floor(r / (max_radius / n_rings)), sector =
 * floor((atan2(y, x) + pi) / (2 pi / n_sectors)), both clamped; an empty bin is 0.0.  The frame's work is enqueued after its
 * last wait and not waited for: host_syncs and d2h_bytes do not change.  DESIGN.md 16. */
typedef struct tloam_place_config {
  int32_t enabled;           /* 0 */
  int32_t n_rings;           /* 20, in [1, 64] */
  int32_t n_sectors;         /* 60, in [2, 360] */
  int32_t num_candidates;    /* 10, in [1, 32] */
  int32_t exclude_recent;    /* 50, >= 1: keyframe q is searched against 0 .. q - exclude_recent */
  int32_t reserved0;
  double max_radius;         /* m: 80 */
  double height_offset;      /* m: 2.0, added to z (finite) */
  double kf_dist;            /* m: 1.0 */
  double kf_angle;           /* rad: 0.2 */
  double dist_thres;         /* 0.30 (measured): a loop when the best d is below it */
  int64_t reserve_keyframes; /* 0: the default room (1024); the database doubles when full */
} tloam_place_config;
void tloam_place_default_config(tloam_place_config* cfg);
/* cfg NULL: the defaults.  Empties the database (so does tloam_odometry_reset; the configuration persists across it).
 * Non-finite or non-positive max_radius / kf_dist / kf_angle / dist_thres, a non-finite height_offset, a count out of its
 * range, enabled not 0 / 1, reserve_keyframes < 0: TLOAM_E_INVALID. */
int tloam_place_configure(tloam_ctx* ctx, const tloam_place_config* cfg);

typedef struct tloam_place_info {
  int64_t n_keyframes;
  int64_t n_loops;           /* read from the device: this call waits for the work in flight */
  int64_t last_keyframe_frame; /* the frame number of the last keyframe, -1 none */
  int64_t capacity_keyframes;
} tloam_place_info;
int tloam_place_get_info(tloam_ctx* ctx, tloam_place_info* info);

typedef struct tloam_place_loop {
  int64_t query_keyframe, query_frame;
  int64_t match_keyframe, match_frame;
  int32_t shift;             /* the candidate's column (j + shift) mod n_sectors matches the query's column j */
  int32_t reserved0;
  double dist;               /* d of the pair */
  double yaw;                /* shift * 2 pi / n_sectors wrapped to (-pi, pi]: the query's heading relative to the match's */
} tloam_place_loop;

/* Keyframes [first, first + count): frame numbers [count], poses [16 count] column-major, ring keys [n_rings count], sector keys
 * [n_sectors count], descriptors [n_rings n_sectors count].  Any output may be NULL.  Out of range: TLOAM_E_INVALID. */
int tloam_place_read_keyframes(tloam_ctx* ctx, size_t first, size_t count, int64_t* frames, double* poses_colmajor,
                               double* ring_keys, double* sector_keys, double* descriptors);
/* Loop records [first, first + count) in the order they were found; the range is checked against n_loops. */
int tloam_place_read_loops(tloam_ctx* ctx, size_t first, size_t count, tloam_place_loop* loops);
/* One scan (AoS, sensor frame) with a pose the caller supplies: described, added as a keyframe whatever the keyframe policy
 * says, and searched, as a frame's keyframe is.  Place recognition must be enabled.  keyframe_out (may be NULL): its id. */
int tloam_place_add_scan(tloam_ctx* ctx, const double* xyz_aos, size_t n, const double pose_colmajor[16], int64_t frame_id,
                         int64_t* keyframe_out);
/* The descriptor [n_rings n_sectors] and keys of one scan under cfg (NULL: the context's configuration; cfg->enabled is not
 * looked at).  The database is not touched.  Any output may be NULL. */
int tloam_place_describe(tloam_ctx* ctx, const tloam_place_config* cfg, const double* xyz_aos, size_t n, double* descriptor,
                         double* ring_key, double* sector_key);
/* Every place recognition call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- loop verification: keyframe clouds and a two-stage TLS match (additive to ABI 8) ----------------
 * Off by default; when off, every frame, stat, map, place record and launch is what it is without it.  With it on, every keyframe
 * of the odometry frame also keeps eight clouds (AoS fp64, sensor frame) in one device arena: side 0, by kind, the four clouds its
 * frame gave the match (none on the first frame), side 1 the four its frame gave the submap (planar / sphere selections, edge /
 * ground: raw on the first frame, down-sampled later).  They are gathered by one launch after the frame's last wait; host_syncs
 * and the byte counts of a frame do not change.  A verification of (query q, match m): the target clouds of keyframes
 * [m - window, m + window] clamped to [0, q - 1], ascending, moved into m's frame by rigid_inverse(P_m) * P_k and put end to end
 * per kind; the source is q's source clouds.  A coarse match (the `coarse` TLS configuration) from the initial guess, then a fine
 * one (the context's own configuration) from its result, both on private child contexts: nothing of the context's registered
 * clouds, grids or results changes.  Score: every source point moved by the fine pose, its nearest target of the same kind;
 * inliers are those closer than inlier_dist, overlap = inliers / points, rmse = sqrt(sum d^2 / inliers).  Accepted when both
 * matches return TLOAM_OK, overlap >= min_overlap and rmse <= max_rmse.  DESIGN.md 17. */
typedef struct tloam_loop_config {
  int32_t enabled;           /* 0 */
  int32_t window;            /* 2: target keyframes m - window .. m + window (>= 0) */
  int32_t init_mode;         /* 0: Rz(loop record's yaw), zero translation; 1: rigid_inverse(P_m) * P_q from the stored poses */
  int32_t reserved0;
  double inlier_dist;        /* m (measured) */
  double min_overlap;        /* (measured) */
  double max_rmse;           /* m (measured) */
  int64_t reserve_points;    /* 0: the default arena (2^20 points); it doubles when full */
  tloam_tls_config coarse;   /* the coarse stage's TLS configuration: the shipped one with wider distance thresholds */
} tloam_loop_config;
void tloam_loop_default_config(tloam_loop_config* cfg);
/* cfg NULL: the defaults.  Empties the keyframe database, its clouds and the constraints (so does tloam_odometry_reset; the
 * configuration persists across it).  Non-finite or non-positive inlier_dist / min_overlap / max_rmse, min_overlap > 1,
 * window < 0, an unknown init_mode, enabled not 0 / 1, reserve_points < 0, a coarse configuration out of range:
 * TLOAM_E_INVALID. */
int tloam_loop_configure(tloam_ctx* ctx, const tloam_loop_config* cfg);

typedef struct tloam_loop_info {
  int64_t n_constraints;
  int64_t n_accepted;
  int64_t arena_points;      /* points the keyframe clouds take */
  int64_t arena_capacity_points;
} tloam_loop_info;
int tloam_loop_get_info(tloam_ctx* ctx, tloam_loop_info* info);

typedef struct tloam_loop_constraint {
  int64_t query_keyframe, query_frame;
  int64_t match_keyframe, match_frame;
  int32_t status;            /* TLOAM_OK, the first failing stage's status, or TLOAM_E_NOT_READY (a side without clouds) */
  int32_t accepted;
  double rel_pose_colmajor[16];   /* match <- query: the fine stage's result */
  double init_colmajor[16];       /* the initial guess of the coarse stage */
  tloam_stats coarse, fine;
  double overlap, rmse;
  int64_t inliers, points;
  double dist, yaw;          /* the loop record's (0 for a pair) */
} tloam_loop_constraint;

/* Keyframe clouds from the caller (for tloam_place_add_scan keyframes, or hosts with their own front end); verification must be
 * on.  src / tgt: four clouds each by kind (AoS); a NULL side leaves that side as it is.  Keyframe out of range: TLOAM_E_INVALID. */
int tloam_place_set_keyframe_clouds(tloam_ctx* ctx, int64_t keyframe, const double* const src_aos[4], const size_t n_src[4],
                                    const double* const tgt_aos[4], const size_t n_tgt[4]);
/* One stored cloud (side 0 source, 1 target; kind TLOAM_KIND_*).  *n is its size even when capacity is too small (then nothing is
 * copied and TLOAM_E_INVALID is returned).  out may be NULL to ask for the size. */
int tloam_place_read_keyframe_clouds(tloam_ctx* ctx, int64_t keyframe, int side, int kind, size_t capacity, size_t* n,
                                     double* out_aos);
/* Verifies, in order, every loop record not verified yet, and appends one constraint each; *n_verified (may be NULL): how many. */
int tloam_loop_verify_pending(tloam_ctx* ctx, int64_t* n_verified);
/* One pair (0 <= match < query < keyframes) from the caller's initial guess (NULL: rigid_inverse(P_m) * P_q); not appended. */
int tloam_loop_verify_pair(tloam_ctx* ctx, int64_t query, int64_t match, const double init_colmajor_or_null[16],
                           tloam_loop_constraint* out);
/* Constraints [first, first + count). */
int tloam_loop_read_constraints(tloam_ctx* ctx, size_t first, size_t count, tloam_loop_constraint* out);
/* Every loop verification call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- pose-graph optimisation of the keyframes (additive to ABI 8) -------------------------------------
 * Runs only when called: with it never called, every frame, stat, map, place record, constraint and launch is what it is
 * without it.  Nodes: N rigid poses P_0 .. P_{N-1}, node 0 fixed.  Edges (i, j, Z, w[6]): Z the measured rigid_inverse(P_i) * P_j,
 * w six inverse variances in tangent order (upsilon, omega).  Edges 0 .. N-2 are the chain, edge k = (k, k + 1); the loops
 * follow.  Residual e = log(rigid_inverse(Z) * rigid_inverse(P_i) * P_j), cost = sum w[a] e[a]^2, update P_n <- P_n * exp(d_n),
 * Jacobians J_j = I, J_i = -Ad(rigid_inverse(P_j) * P_i).  Plain Gauss-Newton; each step's normal equations are solved by
 * conjugate gradients preconditioned with the chain, matrix-free over the edges, in one launch.  An iteration ends the run when
 * its new cost is not finite (the step is dropped), else when max |d| < step_tol (the step is kept), else when the new cost is
 * above the previous one (the step is dropped), else after max_iterations.  Reductions have a fixed order: two runs give the
 * same bits.  DESIGN.md 18. */
typedef struct tloam_graph_config {
  int32_t max_iterations;    /* 30, in [1, 1000]: Gauss-Newton iterations */
  int32_t max_cg_iterations; /* 20000, in [1, 10^6]: conjugate-gradient iterations of one Gauss-Newton step */
  double step_tol;           /* 1e-7 (>= 0, finite; below it the cost no longer resolves a step: DESIGN.md 18) */
  double cg_tol;             /* 1e-10: a solve ends at r^T M^-1 r <= cg_tol^2 r_0^T M^-1 r_0 (>= 0, finite) */
  double odom_sigma_t;       /* m   per keyframe step: 0.05 (margin unmeasured) */
  double odom_sigma_r;       /* rad per keyframe step: 0.005 */
  double loop_sigma_t;       /* m:   0.05 (section 17's measured worst case) */
  double loop_sigma_r;       /* rad: 0.01 */
} tloam_graph_config;
void tloam_graph_default_config(tloam_graph_config* cfg);
/* cfg NULL: the defaults.  Persists across tloam_odometry_reset.  Drops the corrected poses (so do tloam_odometry_reset,
 * tloam_place_configure and tloam_loop_configure).  A count out of its range, a negative or non-finite tolerance, a non-finite
 * or non-positive sigma: TLOAM_E_INVALID. */
int tloam_graph_configure(tloam_ctx* ctx, const tloam_graph_config* cfg);

typedef struct tloam_graph_edge {
  int64_t i, j;
  double rel_pose_colmajor[16];   /* Z: node j in node i's frame */
  double weight[6];               /* inverse variances (upsilon, omega), >= 0; a chain edge's > 0 */
} tloam_graph_edge;

#define TLOAM_GRAPH_STOP_NOT_RUN 0    /* one node or no loop edge: the input poses are the result */
#define TLOAM_GRAPH_STOP_STEP 1       /* max |d| < step_tol */
#define TLOAM_GRAPH_STOP_ITERATIONS 2 /* max_iterations */
#define TLOAM_GRAPH_STOP_COST 3       /* the new cost was not finite or above the previous one: that step was not applied */
#define TLOAM_GRAPH_STOP_CG_LIMIT 4   /* as STEP or ITERATIONS, but the last step's linear solve ended on max_cg_iterations */
typedef struct tloam_graph_info {
  int64_t n_nodes, n_edges, n_loop_edges;
  int32_t iterations;        /* Gauss-Newton iterations run */
  int32_t stop_reason;       /* TLOAM_GRAPH_STOP_* */
  int32_t reverted;          /* 1: the last step was dropped (stop_reason COST) */
  int32_t reserved0;
  int64_t cg_iterations;     /* all steps together */
  double initial_cost, final_cost;
  double last_step;          /* max |d| of the last step computed */
  double last_cg_residual;   /* sqrt(r^T M^-1 r / r_0^T M^-1 r_0) at the end of the last solve */
} tloam_graph_info;

/* The caller's graph; touches nothing else in the context.  poses_in / poses_out: [16 n_nodes] column-major (may be the same
 * storage).  cfg NULL: the context's configuration.  An index out of range, i == j, a chain that is not (k, k + 1) in order, a
 * non-rigid or non-finite pose, a negative or non-finite weight, a chain weight of 0, n_nodes < 1: TLOAM_E_INVALID.  One node or
 * no loop edge: the solver is not run, poses_out holds poses_in's bits.  Node 0's output is its input's bits.  info may be NULL. */
int tloam_graph_solve(tloam_ctx* ctx, const tloam_graph_config* cfg, size_t n_nodes, const double* poses_in_colmajor, size_t n_edges,
                      const tloam_graph_edge* edges, double* poses_out_colmajor, tloam_graph_info* info);
/* The context's graph: nodes the keyframes' stored poses, chain edge k with Z = rigid_inverse(P_k) * P_{k+1} and the odometry
 * weights (1 / sigma^2), one loop edge (match_keyframe, query_keyframe, rel_pose_colmajor) with the loop weights per constraint
 * with accepted != 0, in their order.  Place recognition must be on (else TLOAM_E_INVALID).  Fewer than two keyframes or no
 * accepted constraint: TLOAM_OK, corrected = stored.  Pending loop records are not verified here.  The stored keyframe poses,
 * the odometry state and both maps are not changed.  info may be NULL. */
int tloam_graph_optimize(tloam_ctx* ctx, tloam_graph_info* info);
/* Corrected poses of keyframes [first, first + count), [16 count] column-major, as of the last tloam_graph_optimize
 * (TLOAM_E_NOT_READY before it; keyframes added since are out of range: TLOAM_E_INVALID). */
int tloam_graph_read_poses(tloam_ctx* ctx, size_t first, size_t count, double* poses_colmajor);
/* P'_k * rigid_inverse(P_k) * pose_in for a pose taken near keyframe k (-1: the last corrected one), on the host. */
int tloam_graph_correct_pose(tloam_ctx* ctx, int64_t keyframe, const double pose_in_colmajor[16], double pose_out_colmajor[16]);
/* Every graph call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- robust mode of the pose graph: GNC-TLS on the loop edges (additive to ABI 8) ---------------------------------
 * Off by default: with it off or never configured, every call, bit, launch and byte is what it is without it.  A loop edge that
 * joins two places which only look alike passes verification and, as a plain quadratic term, bends every corrected pose.  The
 * robust mode carries the front end's truncated least squares to the loop edges by graduated non-convexity.  Each loop edge e
 * (edges N-1 .. m-1) has a scale s_e in [0, 1], at first 1; the chain is never scaled; a solve's weights are s_e * w_e.  Its
 * statistic is r_e = sum_a w_e[a] e_e[a]^2 at the current poses with the caller's weights (a ascending); c2 = noise_chi2.
 *   1. the solve above from the input poses, all s = 1;  2. r;  3. max r <= c2: done -- the plain solve's bits, no outer
 *   iteration (ALL_INLIERS);  4. else mu = c2 / (2 max r - c2);  5. outer iteration t = 1 .. max_outer: lo = mu / (mu + 1) c2,
 *   hi = (mu + 1) / mu c2; s_e = 1 where r_e <= lo, 0 where r_e >= hi or r_e is not finite, else sqrt(c2 mu (mu + 1) / r_e) - mu
 *   (held to [0, 1]); the solve above from the current poses with the scaled weights; r at its result; every s_e 0 or 1: done
 *   (BINARY); else mu *= mu_factor;  6. max_outer used up: OUTER_LIMIT, the last poses and scales stand.
 * An inner solve that ends on TLOAM_GRAPH_STOP_COST keeps the poses before its dropped step and the outer loop goes on.  A
 * rejected edge stays rejected only while r_e >= hi: nothing re-admits an edge after the run.  A true edge can end rejected (a
 * second self-consistent fixed point).  Costs one launch and one small read per outer iteration, and two more of
 * each per run, on top of the inner solves'.  Reductions have a fixed order: two runs give the same bits. */
typedef struct tloam_graph_robust_config {
  int32_t enabled;     /* 0 */
  int32_t max_outer;   /* 100, in [1, 10000] */
  double noise_chi2;   /* 36 (> 0, finite): an inlier's largest r.  6 sigma in one component; 16.81 is the 99 % point of
                          chi-squared with 6 degrees of freedom and rejected true edges on the test graphs */
  double mu_factor;    /* 1.4 (> 1, finite): the usual GNC value; 2.0 made the same decisions in half the outer iterations */
} tloam_graph_robust_config;
void tloam_graph_robust_default_config(tloam_graph_robust_config* cfg);
/* cfg NULL: the defaults (off).  Persists across tloam_odometry_reset.  Drops the corrected poses, as tloam_graph_configure
 * does.  A value out of its range: TLOAM_E_INVALID. */
int tloam_graph_robust_configure(tloam_ctx* ctx, const tloam_graph_robust_config* cfg);

#define TLOAM_GRAPH_ROBUST_STOP_OFF 0          /* the mode is off: the plain solve */
#define TLOAM_GRAPH_ROBUST_STOP_ALL_INLIERS 1  /* max r <= noise_chi2 after the plain solve (or the solver was not run) */
#define TLOAM_GRAPH_ROBUST_STOP_BINARY 2       /* every scale is 0 or 1 */
#define TLOAM_GRAPH_ROBUST_STOP_OUTER_LIMIT 3  /* max_outer */
typedef struct tloam_graph_robust_info {
  int32_t outer_iterations;
  int32_t stop_reason;                 /* TLOAM_GRAPH_ROBUST_STOP_* */
  int64_t gn_iterations;               /* all inner solves together, the first included */
  int64_t cg_iterations;
  int64_t rejected, kept, undecided;   /* loop edges with s == 0, s == 1, in between, at the end */
  double mu_first, mu_last;            /* mu of the first and of the last outer iteration (0: there was none) */
  double max_chi2_first;               /* max r after the plain solve */
} tloam_graph_robust_info;

/* tloam_graph_solve with the robust mode: the same validation.  rcfg NULL: the context's robust configuration; a value out of
 * its range: TLOAM_E_INVALID.  info describes the last inner solve, except that initial_cost is the first solve's.
 * loop_scale_out / loop_chi2_out: [n_edges - (n_nodes - 1)], the loop edges' final s and r (r at poses_out); either may be
 * NULL, so may info and rinfo.  With enabled == 0 it is tloam_graph_solve bit for bit: no further launch or read, the scales
 * are 1 and r, which nothing computed, is NaN. */
int tloam_graph_solve_robust(tloam_ctx* ctx, const tloam_graph_config* cfg, const tloam_graph_robust_config* rcfg, size_t n_nodes,
                             const double* poses_in_colmajor, size_t n_edges, const tloam_graph_edge* edges,
                             double* poses_out_colmajor, tloam_graph_info* info, tloam_graph_robust_info* rinfo,
                             double* loop_scale_out, double* loop_chi2_out);
/* tloam_graph_optimize runs the robust algorithm when the context's robust configuration is enabled; tloam_graph_read_poses,
 * tloam_graph_correct_pose and tloam_closed_map_build(pose_source = 1) then use its poses.
 * Loop edges [first, first + count) of the last tloam_graph_optimize: the index of the edge's constraint as
 * tloam_loop_read_constraints numbers them, its scale and its r (any of the three may be NULL).  TLOAM_E_NOT_READY before an
 * optimise; after a non-robust one every scale is 1 and r is NaN. */
int tloam_graph_read_loop_scales(tloam_ctx* ctx, size_t first, size_t count, int64_t* constraint_index, double* scale, double* chi2);
/* Of the last tloam_graph_optimize (TLOAM_E_NOT_READY before it). */
int tloam_graph_get_robust_info(tloam_ctx* ctx, tloam_graph_robust_info* out);
/* Every robust graph call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- the closed map: the keyframe clouds merged under corrected poses (additive to ABI 8) ----------------------
 * A third map beside tloam_map_* and tloam_voxel_map_*.  Runs only when called: with it never called, every frame, stat, map,
 * place record, constraint, corrected pose and launch is what it is without it.  Input: the context's keyframes 0 .. K-1 with
 * their stored clouds (loop verification must be on, else TLOAM_E_INVALID).  cloud_mask has bit side * 4 + kind set for every
 * cloud slot that takes part; a keyframe's input is its selected clouds end to end in ascending slot order, points in stored
 * order.  A keyframe without points in the selected slots adds nothing (empty_keyframes).  Per point: the world point is the
 * keyframe's pose applied as tloam_registered_scan applies it; quantisation, key, N, Q and centroid are tloam_voxel_map_*'s
 * (above), non-finite world points left out.  A keyframe with |i| >= 2^20 on an axis for any finite point adds nothing
 * (overflow_keyframes); the others are not affected.  Voxel ids in order of the smallest global point index, global meaning
 * keyframes ascending, then the concatenation above.  The sums are int64: two builds, or two contexts, give the same bits.
 * DESIGN.md 19. */
typedef struct tloam_closed_map_config {
  double voxel;             /* v: 1.0 */
  double origin[3];         /* o: (0, 0, 0) */
  int32_t cloud_mask;       /* 0xF0: side 1, the four clouds the keyframe's frame gave the submap */
  int32_t reserved0;
  int64_t reserve_voxels;   /* voxels of HBM the first build reserves; 0 = 2^20; grows past it inside a build */
} tloam_closed_map_config;
void tloam_closed_map_default_config(tloam_closed_map_config* cfg);
/* cfg NULL: the defaults.  Empties the closed map (so do tloam_odometry_reset, tloam_place_configure and tloam_loop_configure;
 * tloam_graph_configure and a later tloam_graph_optimize do not: the closed map says which poses it was built with); the
 * configuration persists across tloam_odometry_reset.  voxel <= 0 or not finite, a non-finite origin, a mask of 0 or with bits
 * beyond 8, reserve_voxels < 0: TLOAM_E_INVALID. */
int tloam_closed_map_configure(tloam_ctx* ctx, const tloam_closed_map_config* cfg);

#define TLOAM_CLOSED_MAP_POSES_STORED 0     /* the stored keyframe poses */
#define TLOAM_CLOSED_MAP_POSES_CORRECTED 1  /* the corrected poses of the last tloam_graph_optimize */
#define TLOAM_CLOSED_MAP_POSES_CALLER 2     /* the caller's */
typedef struct tloam_closed_map_info {
  int64_t n_keyframes;         /* K of the last build */
  int64_t added_keyframes;     /* K - empty_keyframes - overflow_keyframes */
  int64_t empty_keyframes;     /* no point in the selected slots */
  int64_t overflow_keyframes;  /* a finite point left the grid: added nothing */
  int64_t n_voxels;            /* occupied voxels */
  int64_t n_points;            /* points in them: the sum of N */
  int64_t capacity_voxels;     /* voxels the rows hold before they grow */
  int32_t pose_source;         /* of the last build */
  int32_t launches;            /* kernel launches of the last build: the same for every K, span count and point count */
} tloam_closed_map_info;
int tloam_closed_map_get_info(tloam_ctx* ctx, tloam_closed_map_info* info);
/* Builds the closed map from all keyframes at once, replacing the previous one.  pose_source 0: the stored poses; 1: the
 * corrected poses (TLOAM_E_NOT_READY before any tloam_graph_optimize; a keyframe added since that optimise takes
 * tloam_graph_correct_pose(ctx, -1, P_k, ...), bit for bit); 2: poses_colmajor [16 n_poses] (n_poses != K, a non-finite or
 * non-rigid pose: TLOAM_E_INVALID).  A refused call leaves the previous closed map as it was.  A build that fails
 * (TLOAM_E_HIP: an allocation, a bounded wait of a kernel running out) leaves the closed map empty.  Nothing else in the
 * context changes.  info may be NULL. */
int tloam_closed_map_build(tloam_ctx* ctx, int pose_source, const double* poses_colmajor_or_null, size_t n_poses,
                           tloam_closed_map_info* info_or_null);
/* As tloam_voxel_map_read / tloam_voxel_map_read_box, on the closed map.  TLOAM_E_NOT_READY without a built closed map. */
int tloam_closed_map_read(tloam_ctx* ctx, size_t first, size_t count, double* centroids_aos, int64_t* counts);
int tloam_closed_map_read_box(tloam_ctx* ctx, const double lo[3], const double hi[3], int64_t min_count, size_t capacity,
                              size_t* n, double* centroids_aos, int64_t* counts);
/* The poses keyframes [first, first + count) were built with, [16 count] column-major.  A range beyond n_keyframes:
 * TLOAM_E_INVALID; TLOAM_E_NOT_READY without a built closed map. */
int tloam_closed_map_read_poses(tloam_ctx* ctx, size_t first, size_t count, double* poses_colmajor);
/* Every closed map call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- the closed map extended in place by the keyframes added since its build (additive to ABI 8) -----------------
 * With it never called, every call, bit and launch is what it is without it.  The call takes keyframes [K, n_kf): K the map's
 * info.n_keyframes, n_kf the context's keyframes -- the ones added since the build, the load or the last extend, by the odometry
 * frame or by tloam_place_add_scan + tloam_place_set_keyframe_clouds.  pose_source 0: their stored poses; 1: the build's rule for
 * the same keyframes (TLOAM_E_NOT_READY before any tloam_graph_optimize); 2: poses_colmajor [16 (n_kf - K)], of the new keyframes
 * only (n_poses != n_kf - K, a non-finite or non-rigid pose: TLOAM_E_INVALID).
 * Rows: every rule of the build holds for the new keyframes (mask, concatenation, non-finite points, a keyframe with a point
 * beyond the grid, an empty keyframe).  A point whose voxel is in the map adds to its N and Q; the others create voxels, with ids
 * from the old n_voxels upward in order of the smallest index among the new points.  Rows, ids, n_voxels and n_points are then
 * those of a build over all n_kf keyframes under the same poses, bit for bit; info.n_keyframes becomes n_kf, the keyframe counts
 * grow by the new keyframes', pose_source becomes the call's, launches stays the build's, tloam_closed_map_read_poses sees the new
 * keyframes.  The sums are integers per voxel and ids are handed out in order of the smallest global index, which a later
 * keyframe can only append to: this is a rebuild, not an approximation of one.
 * Surfels (when the map has them): the new points' thirteen integers are added (to zero for a new id) and every voxel a new point
 * fell in is solved again: sums, normals, variances and the surfel info equal a full pass after a full build.
 * Carve (when the map is carved): M of a new id starts at 0; the rays of the NEW keyframes (the carve configuration's ray_mask)
 * are walked through the map as extended and their misses added; old rays are not walked again:
 * M_ext = [M_before, 0 ...] + carve(V_ext, new keyframes only).  This is deliberately not a full carve's M: a voxel that appeared
 * with the new keyframes is not held to account for rays cast before it existed, and an old ray was tested against the centroid
 * its voxel had then.  carve_info: n_keyframes becomes n_kf; n_rays, skipped_rays, steps and tested grow by the call's; misses
 * and voxels_missed are those of the stored M.  A later tloam_closed_map_carve replaces them with the full semantics.
 * The localiser's voxel records go stale (the next localise or diff reports prepared) and the diff's counts are dropped.  Place,
 * loop and graph state and the clouds are not written.  A detached map (loaded without its clouds) extends like any other -- only
 * the new keyframes' clouds are read -- and stays detached.
 * Refused, with every byte left as it was: no built map (TLOAM_E_NOT_READY); nranks > 1, keyframe clouds off, fewer keyframes
 * than the map was built from, a bad pose_source or bad poses, n_points that would pass 2^30 (TLOAM_E_INVALID).  n_kf == K is
 * TLOAM_OK and changes nothing.  A call that fails after its first launch (TLOAM_E_HIP: an allocation, a bounded wait running
 * out) leaves the closed map empty, as a failed build does.  The staging is sized by the new points alone (a table of the power of
 * two >= 2 n and a slot per point) and freed with the call.  DESIGN.md 27. */
typedef struct tloam_closed_map_extend_info {
  int64_t first_keyframe;      /* K before the call */
  int64_t n_keyframes;         /* n_kf - K: the keyframes the call took */
  int64_t added_keyframes;     /* of them: n_keyframes - empty_keyframes - overflow_keyframes */
  int64_t empty_keyframes;
  int64_t overflow_keyframes;
  int64_t points;              /* points added to the rows */
  int64_t new_voxels;          /* voxels created */
  int64_t touched_voxels;      /* voxels a new point fell in, the new ones included */
  int64_t rays;                /* carved maps: the call's rays, and of them ... */
  int64_t skipped_rays;
  int64_t steps;
  int64_t tested;
  int64_t misses;
  int64_t solved_voxels;       /* maps with surfels: the map's solved voxels after the call */
  int32_t grown;               /* 1: the rows were reallocated inside the call */
  int32_t launches;            /* kernel launches of the call: they depend on surfels, carve and grown alone */
} tloam_closed_map_extend_info;
int tloam_closed_map_extend(tloam_ctx* ctx, int pose_source, const double* poses_colmajor_or_null, size_t n_poses,
                            tloam_closed_map_extend_info* info_or_null);
/* Of the last successful extend since the map was built or loaded; zero when there was none. */
int tloam_closed_map_get_extend_info(tloam_ctx* ctx, tloam_closed_map_extend_info* info);

/* ---- the carve of the closed map: per voxel, the rays that passed through it (additive to ABI 8) ----------------
 * A lidar return also says that nothing was between the sensor and the point.  A carve counts, per occupied voxel of the built
 * closed map, the rays of the build's keyframes 0 .. K-1 that passed through it: M beside N.  Runs only when called; nothing
 * of the closed map or the context is changed, and tloam_closed_map_read / _read_box still return every voxel.
 * Rays: the points of the clouds selected by ray_mask (the bits of cloud_mask; 0: the build's mask), keyframes ascending, slots
 * ascending, points in stored order.  A ray runs from O, the translation of the keyframe's pose, to E, the point under that
 * pose.  It is skipped when E is not finite, when its length L is 0 or > max_range, or when the cell of O or E has
 * |i| >= 2^20 on an axis.  The cells it visits are those of a walk through the grid from the cell of O, the cell of E left
 * out; a visited cell that is a voxel of the closed map with centroid C is missed when the foot of C on the ray lies at
 * 0 <= t < 1 - end_margin / L and C is within radius of the ray.  All sums are integers: two carves, or two contexts, give the
 * same bits.  DESIGN.md 21 states the arithmetic. */
typedef struct tloam_closed_map_carve_config {
  double max_range;    /* 60.0 m: longer rays are skipped */
  double end_margin;   /* 1.0 m in front of the return in which nothing is missed */
  double radius;       /* 0.25 m: the largest distance from a centroid to a ray that misses it; +inf allowed */
  int32_t ray_mask;    /* 0: the closed map's cloud_mask */
  int32_t reserved0;
} tloam_closed_map_carve_config;
void tloam_closed_map_carve_default_config(tloam_closed_map_carve_config* cfg);
/* cfg NULL: the defaults.  Drops the counts (not the closed map); persists across tloam_odometry_reset.  max_range not > 0 or
 * not finite, end_margin < 0 or not finite, radius not > 0 (NaN too), a mask with bits beyond 8: TLOAM_E_INVALID, and the
 * counts stay. */
int tloam_closed_map_carve_configure(tloam_ctx* ctx, const tloam_closed_map_carve_config* cfg);
typedef struct tloam_closed_map_carve_info {
  int64_t n_keyframes;     /* K of the closed map carved */
  int64_t n_rays;          /* the points of the selected clouds, skipped ones included */
  int64_t skipped_rays;
  int64_t steps;           /* cells visited */
  int64_t tested;          /* of them, voxels of the closed map */
  int64_t misses;          /* the sum of M */
  int64_t voxels_missed;   /* voxels with M > 0 */
  int32_t launches;        /* kernel launches of the carve: the same for every K, mask and ray count */
  int32_t reserved0;
} tloam_closed_map_carve_info;
/* Of the last carve; zero when there are no counts. */
int tloam_closed_map_get_carve_info(tloam_ctx* ctx, tloam_closed_map_carve_info* info);
/* Counts M for the built closed map, replacing the previous counts.  TLOAM_E_NOT_READY without a built closed map.  Whatever
 * empties or replaces the closed map drops the counts; keyframes added since the build cast no rays.  info may be NULL. */
int tloam_closed_map_carve(tloam_ctx* ctx, tloam_closed_map_carve_info* info_or_null);
/* M of voxels [first, first + count) in id order.  TLOAM_E_NOT_READY without counts. */
int tloam_closed_map_read_misses(tloam_ctx* ctx, size_t first, size_t count, int64_t* misses);
/* tloam_closed_map_read_box's rule, order and capacity convention, a voxel additionally left out when
 * M >= min_miss && (double) M > miss_ratio * (double) N.  lo and hi both NULL: the whole map.  TLOAM_E_NOT_READY without counts. */
int tloam_closed_map_read_carved(tloam_ctx* ctx, const double* lo_or_null, const double* hi_or_null, int64_t min_count,
                                 int64_t min_miss, double miss_ratio, size_t capacity, size_t* n, double* centroids_aos,
                                 int64_t* counts, int64_t* misses);
/* Every carve call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- the surfels of the closed map: per voxel a normal and three variances (additive to ABI 8) --------------------
 * The closed map knows where surfaces are; a surfel pass adds how they face.  Per occupied voxel of the built closed map it
 * gathers the second moments of the points that fell in it and solves them for a normal and the variances along the three
 * principal axes.  Runs only when called; nothing of the closed map, of a carve's counts or of the context is changed.
 * Points: exactly the build's -- the clouds of the build's cloud_mask of keyframes 0 .. K-1, keyframes ascending, slots
 * ascending, stored order, each under the pose the build used; a point that is not finite under its pose is left out, and a
 * keyframe with a finite point at |i| >= 2^20 adds nothing.  A point whose cell is not a voxel of the map (its clouds were
 * re-attached since the build) adds nothing and is counted in orphan_points.
 * Per point, integers: r = q >> 8 of the voxel map's q (2^-16 of a voxel), w_a = round-half-up of ((O_a - E_a) / v) * 256
 * clamped to +-2^30, with E the point and O the translation of its keyframe's pose.  Per voxel thirteen int64 sums:
 * Ns, R_a = sum r_a, S_ab = sum r_a r_b (xx xy xz yy yz zz), W_a = sum w_a -- the same bits in any order, pass and context.
 * Per voxel with Ns >= min_points, in fp64: the mean m = R / Ns, the covariance c_ab = S_ab / Ns - m_a m_b, its eigenvalues
 * ascending and the eigenvector n of the smallest, turned so that n . W >= 0 (towards where it was seen from); the variances are
 * the eigenvalues in m^2.  A voxel of fewer points is unsolved: n and the variances are zero.  Collinear or coincident points
 * are solved as they come; tloam_closed_map_read_surfels_box's gate is what rejects them.  DESIGN.md 22 states the arithmetic. */
typedef struct tloam_closed_map_surfel_config {
  int32_t min_points;   /* 5: a voxel of fewer points is not solved; >= 3 */
  int32_t reserved0;
} tloam_closed_map_surfel_config;
void tloam_closed_map_surfel_default_config(tloam_closed_map_surfel_config* cfg);
/* cfg NULL: the defaults.  Drops the surfels (not the closed map or the carve's counts); persists across tloam_odometry_reset.
 * min_points < 3: TLOAM_E_INVALID, and the surfels stay. */
int tloam_closed_map_surfel_configure(tloam_ctx* ctx, const tloam_closed_map_surfel_config* cfg);
typedef struct tloam_closed_map_surfel_info {
  int64_t n_keyframes;     /* K of the closed map */
  int64_t n_points;        /* points summed: the sum of Ns */
  int64_t orphan_points;   /* points whose cell is not a voxel of the map */
  int64_t solved_voxels;   /* voxels with Ns >= min_points */
  int32_t launches;        /* kernel launches of the pass: the same for every K, mask and point count */
  int32_t reserved0;
} tloam_closed_map_surfel_info;
/* Of the last pass; zero when there are no surfels. */
int tloam_closed_map_get_surfel_info(tloam_ctx* ctx, tloam_closed_map_surfel_info* info);
/* Gathers and solves the surfels of the built closed map, replacing the previous ones.  TLOAM_E_NOT_READY without a built closed
 * map.  Whatever empties or replaces the closed map drops the surfels; keyframes added since the build add nothing.  The first
 * pass allocates 152 bytes per voxel of the closed map's capacity.  info may be NULL. */
int tloam_closed_map_surfels(tloam_ctx* ctx, tloam_closed_map_surfel_info* info_or_null);
/* The thirteen sums of voxels [first, first + count) in id order, out[13 * count]: Ns, Rx Ry Rz, Sxx Sxy Sxz Syy Syz Szz,
 * Wx Wy Wz.  TLOAM_E_NOT_READY without surfels. */
int tloam_closed_map_read_moments(tloam_ctx* ctx, size_t first, size_t count, int64_t* out);
/* Normals [3 count], variances ascending [3 count] (m^2) and Ns [count] of voxels [first, first + count) in id order; any of
 * the three may be NULL.  TLOAM_E_NOT_READY without surfels. */
int tloam_closed_map_read_surfels(tloam_ctx* ctx, size_t first, size_t count, double* normals_aos, double* evals_aos,
                                  int64_t* counts);
/* tloam_closed_map_read_carved's rule (N >= min_count, the box; lo and hi both NULL: the whole map), order and capacity
 * convention, a voxel kept only when it is solved, ev2 > 0, ev0 <= max_sigma * max_sigma (max_sigma = +inf allowed) and
 * (ev1 - ev0) >= min_planarity * ev2.  counts: Ns.  Any output may be NULL.  TLOAM_E_NOT_READY without surfels. */
int tloam_closed_map_read_surfels_box(tloam_ctx* ctx, const double* lo_or_null, const double* hi_or_null, int64_t min_count,
                                      double max_sigma, double min_planarity, size_t capacity, size_t* n, double* centroids_aos,
                                      double* normals_aos, double* evals_aos, int64_t* counts);
/* Every surfel call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- localisation of a scan in the closed map: point-to-plane Gauss-Newton on the surfels (additive to ABI 8) ------
 * The closed map with surfels is a localisation target: a voxel whose surfel passes the gate of
 * tloam_closed_map_read_surfels_box (solved, ev2 > 0, ev0 <= max_sigma^2, ev1 - ev0 >= min_planarity * ev2) is a plane through
 * the voxel's centroid c with the surfel's normal n.  Runs only when called; nothing of the closed map, of a carve's counts, of
 * the surfels or of the context's odometry is changed.
 * Per point p of the scan (sensor frame) and pose matrix M: E = M p (rows accumulated left to right, as the closed map's build);
 * a point that is not finite there is left out; its cell i by the closed map's quantisation, a point with |i| >= 2^20 on an
 * axis is unmatched; of the 27 cells i + (dx, dy, dz) -- dz outermost, dx innermost, each from -1 to 1 -- the eligible voxel
 * with the smallest D = |E - c|^2 under a strict < (the first visited wins a tie); r = n . (E - c); the point is used when it
 * is matched and |r| <= tau.  Over the used points with unit weights J = [n, E x n], H = sum J^T J, g = sum J^T r,
 * cost = sum r^2 / 2.  The sums are formed without floating-point atomics, in an order fixed by the point index alone: two
 * calls, and two contexts, return the same bits.
 * Iteration k = 0 ..: the state is a unit quaternion and a translation, M = its matrix; tau_k = max(min_residual,
 * max_residual0 * shrink^k); H d = -g by a 6 x 6 Cholesky; the state becomes exp(d) * state (d = (translation, rotation), the
 * convention of tloam_se3_exp); converged when |d[0:3]| < step_tol_t and |d[3:6]| < step_tol_r.  An iteration is degenerate when
 * used < min_matches, a sum is not finite, or a Cholesky pivot is not > min_pivot_ratio * H_kk: the call then ends with status
 * DEGENERATE and pose_out = prior, bit for bit.  DESIGN.md 23 states the arithmetic. */
typedef struct tloam_closed_map_localise_config {
  double max_residual0;     /* 1.0: tau of iteration 0 (m); > 0 */
  double shrink;            /* 0.7: tau's factor per iteration; in (0, 1] */
  double min_residual;      /* 0.1: tau's floor (m); >= 0 */
  double max_sigma;         /* +inf: the gate's largest sqrt(ev0) (m); >= 0 */
  double min_planarity;     /* 0.05: the gate's smallest (ev1 - ev0) / ev2; finite */
  double step_tol_t;        /* 1e-6 (m); >= 0 */
  double step_tol_r;        /* 1e-7 (rad); >= 0 */
  double min_pivot_ratio;   /* 1e-9; in [0, 1) */
  int32_t max_iterations;   /* 20; 1 .. 64 */
  int32_t min_matches;      /* 50; >= 1 */
} tloam_closed_map_localise_config;
void tloam_closed_map_localise_default_config(tloam_closed_map_localise_config* cfg);
/* cfg NULL: the defaults.  A value out of its range (NaN too): TLOAM_E_INVALID, and the old configuration stays.  Persists across
 * tloam_odometry_reset.  Changes nothing of the closed map, the carve or the surfels. */
int tloam_closed_map_localise_configure(tloam_ctx* ctx, const tloam_closed_map_localise_config* cfg);
enum { TLOAM_LOCALISE_CONVERGED = 0, TLOAM_LOCALISE_MAX_ITERATIONS = 1, TLOAM_LOCALISE_DEGENERATE = 2 };
typedef struct tloam_closed_map_localise_info {
  int32_t status;       /* TLOAM_LOCALISE_* */
  int32_t iterations;   /* executed, the degenerate one included */
  int64_t matched;      /* of the last executed sweep */
  int64_t used;
  double rms;           /* sqrt(2 cost / used) of the last executed sweep (0 when used == 0) */
  int32_t launches;     /* sweep and step launches of the call: 2 max_iterations, the same for every input */
  int32_t prepared;     /* 1: the call rebuilt the cached voxel records (one more launch) */
} tloam_closed_map_localise_info;
typedef struct tloam_closed_map_localise_record {   /* one executed iteration */
  double pose_colmajor[16];   /* the pose the sweep ran at (before the step) */
  double tau;
  double cost;
  double d[6];                /* the step (translation, rotation); zero for the degenerate iteration */
  int64_t matched;
  int64_t used;
} tloam_closed_map_localise_record;
/* Localises points_aos (n points, sensor frame) from `prior` (column-major, a rigid transform).  TLOAM_E_NOT_READY without a
 * built closed map with surfels; TLOAM_E_INVALID for n == 0, a NULL argument or a prior that is not a rigid transform; a refused
 * call leaves everything as it was.  One wait: the scan is uploaded and max_iterations pairs of launches are enqueued; a pair
 * behind the last executed iteration returns on entry.  info may be NULL. */
int tloam_closed_map_localise(tloam_ctx* ctx, const double* points_aos, size_t n, const double* prior_colmajor,
                              double* pose_out_colmajor, tloam_closed_map_localise_info* info_or_null);
/* The executed iterations of the last tloam_closed_map_localise on this context; *n is set to their number even when capacity
 * is too small (then nothing is copied and TLOAM_E_INVALID is returned).  records may be NULL to ask for the size. */
int tloam_closed_map_localise_log(tloam_ctx* ctx, size_t capacity, size_t* n, tloam_closed_map_localise_record* records);
/* One sweep at the given matrix (a rigid transform, used as it stands) and tau (>= 0, +inf allowed), no step: per point the
 * matched voxel's id (-1: none) and r (0 where unmatched), either NULL; out28 = H's upper triangle by rows (21), g (6), cost;
 * counts2 = matched, used.  Errors as tloam_closed_map_localise. */
int tloam_closed_map_linearise(tloam_ctx* ctx, const double* points_aos, size_t n, const double* pose_colmajor, double tau,
                               int32_t* ids_or_null, double* residuals_or_null, double* out28, int64_t* counts2);
/* Every localisation call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- several hypotheses of one scan, and relocalisation without a prior (additive to ABI 8) -----------
 * tloam_closed_map_localise_batch localises ONE scan from B priors (B in 1 .. 32) in one set of launches: one upload of the
 * scan, the voxel records rebuilt when stale, max_iterations pairs of launches for all hypotheses together (the hypothesis is a
 * grid dimension of the sweep and a workgroup of the step), one wait.  Hypothesis h returns the pose, the info and the log of
 * tloam_closed_map_localise called alone with priors[h], bit for bit: both forms run one device body, and a hypothesis's sums
 * are formed in the single call's order -- lane, wave, block by point index -- whatever B is.  A hypothesis that has ended
 * leaves its launches on entry; infos[h].launches is 2 max_iterations for every h and every input.
 * *best_out: among the hypotheses whose status is not DEGENERATE the largest `used`; on a tie the smaller cost (sum r^2 / 2 of
 * the last executed sweep); then the lower index; -1 when every hypothesis is degenerate (every poses_out[h] is then its prior,
 * bit for bit).
 * Errors as tloam_closed_map_localise, checked over all B priors before anything is touched; B == 0 or B > 32:
 * TLOAM_E_INVALID.  A refused call leaves the last single call's log and the last batch's logs as they were.  Memory is
 * grow-only: B * ceil(n / 256) * 256 bytes of partial sums, B blocks of state words, B * 64 log records. */
int tloam_closed_map_localise_batch(tloam_ctx* ctx, const double* points_aos, size_t n, const double* priors_colmajor /*[16 B]*/,
                                    size_t B, double* poses_out_colmajor /*[16 B]*/,
                                    tloam_closed_map_localise_info* infos /*[B]*/, int32_t* best_out);
/* The executed iterations of hypothesis `hypothesis` of the last tloam_closed_map_localise_batch (or of the last
 * tloam_closed_map_relocalise, which runs on the same storage) on this context; capacity convention of
 * tloam_closed_map_localise_log.  TLOAM_E_INVALID for a hypothesis the last batch did not have. */
int tloam_closed_map_localise_batch_log(tloam_ctx* ctx, size_t hypothesis, size_t capacity, size_t* n,
                                        tloam_closed_map_localise_record* records);

/* tloam_closed_map_relocalise: scan in, pose out, no prior, one wait.  Needs place recognition enabled (the keyframe database)
 * and a built closed map with surfels.
 * 1. The scan's descriptor and ring key are those of tloam_place_describe under the context's place configuration.
 * 2. The candidates are keyframes 0 .. K-1 of the closed map's last build (tloam_closed_map_info.n_keyframes; no
 *    exclude_recent): the min(num_candidates, K) nearest in ring key, ties to the lower keyframe, each with its best column
 *    shift and distance d by the rules and the arithmetic of the loop search.  The query is not added to the database, and no
 *    loop record is written.
 * 3. Hypothesis h: yaw_h as tloam_place_loop.yaw; prior_h = P_build[keyframe_h] * Rz(yaw_h), P_build the pose the build used
 *    (tloam_closed_map_read_poses) -- the candidate's column j + shift matches the query's column j, so the query's heading
 *    is the keyframe's plus yaw.  Formed on the device.  A candidate whose d is not < max_dist is `skipped`: never swept, its
 *    pose is its prior, its localise info is zero but for status = DEGENERATE, launches and prepared.
 * 4. All hypotheses go through the batched localiser under the context's localise configuration: hypothesis h has the bits of
 *    tloam_closed_map_localise_batch called with the priors reported.
 * 5. The pick is the batch's rule over the hypotheses not skipped.  FOUND when the winner has
 *    used >= min_used_ratio * (finite points of the scan) and rms <= max_rms; else NOT_FOUND: pose_out is not written, best = -1
 *    and the best's fields of the info are zero (keyframe -1).
 * The defaults are choices, not measurements.  info.launches: the two of the description, the two of the search, the priors and
 * 2 max_iterations -- the same for every input (the records' rebuild, when `prepared`, is one more). */
typedef struct tloam_closed_map_relocalise_config {
  int32_t num_candidates;   /* 8; 1 .. 32: keyframes localised from */
  int32_t reserved0;
  double max_dist;          /* +inf: a candidate whose Scan Context d is not < max_dist is not localised from; > 0 */
  double min_used_ratio;    /* 0.5: accepted when used >= min_used_ratio * (finite points of the scan); in [0, 1] */
  double max_rms;           /* +inf (m); > 0 */
} tloam_closed_map_relocalise_config;
enum { TLOAM_RELOCALISE_FOUND = 0, TLOAM_RELOCALISE_NOT_FOUND = 1 };
typedef struct tloam_closed_map_relocalise_info {
  int32_t status;           /* TLOAM_RELOCALISE_* */
  int32_t n_hypotheses;     /* min(num_candidates, K) */
  int32_t best;             /* index into the hypotheses; -1: none */
  int32_t launches;
  int64_t keyframe;         /* of the best, as are the fields below */
  int32_t shift;
  int32_t reserved0;
  double dist;
  double yaw;
  tloam_closed_map_localise_info localise;
} tloam_closed_map_relocalise_info;
typedef struct tloam_closed_map_relocalise_hypothesis {
  int64_t keyframe;
  int32_t shift;
  int32_t skipped;
  double dist;
  double yaw;
  double prior_colmajor[16];
  double pose_colmajor[16];
  tloam_closed_map_localise_info localise;
} tloam_closed_map_relocalise_hypothesis;
void tloam_closed_map_relocalise_default_config(tloam_closed_map_relocalise_config* cfg);
/* cfg NULL: the defaults.  A value out of its range (NaN too): TLOAM_E_INVALID, and the old configuration stays.  Persists across
 * tloam_odometry_reset. */
int tloam_closed_map_relocalise_configure(tloam_ctx* ctx, const tloam_closed_map_relocalise_config* cfg);
/* TLOAM_E_NOT_READY when place recognition is not enabled or there is no built closed map with surfels; TLOAM_E_INVALID for
 * n == 0, a NULL points or pose_out, or nranks > 1.  A refused call leaves everything as it was.  The keyframe database -- its
 * count, keys, descriptors and loop records -- the closed map and its surfels are only read.  info may be NULL. */
int tloam_closed_map_relocalise(tloam_ctx* ctx, const double* points_aos, size_t n, double* pose_out_colmajor,
                                tloam_closed_map_relocalise_info* info_or_null);
/* The hypotheses of the last tloam_closed_map_relocalise, in candidate order; capacity convention of
 * tloam_closed_map_localise_log. */
int tloam_closed_map_relocalise_hypotheses(tloam_ctx* ctx, size_t capacity, size_t* n,
                                           tloam_closed_map_relocalise_hypothesis* hypotheses);

/* ---- a scan diffed against the closed map: new points, voxels seen through (additive to ABI 8) ------
 * With the pose known (tloam_closed_map_localise), what of the scan is not in the map, and what of the map does the scan see
 * through?  A diff reads the built closed map with its surfels and writes nothing of them: it runs on a detached (loaded) map,
 * only when called, and no frame, map, carve, surfel, localisation or snapshot changes by a bit.
 * Per point p (sensor frame) and pose matrix M, used as it stands: O = (M[12], M[13], M[14]), E = M p as the localiser forms it.
 * Point side, a label per point:
 *   TLOAM_DIFF_INVALID   E is not finite, or its cell has |i| >= 2^20 on an axis.
 *   Otherwise the 27 cells i + (dx, dy, dz) in the localiser's order (dz outermost, dx innermost; a cell beyond the grid is no
 *   voxel).  An occupied voxel counts unless carve_gate is set and the carved read would leave it out
 *   (M >= min_miss && (double) M > miss_ratio * (double) N, M the stored misses).  For a voxel that counts d = E - c,
 *   D = (d_x*d_x + d_y*d_y) + d_z*d_z; two minima under a strict < (the first visited wins a tie): the nearest ELIGIBLE voxel (the
 *   localiser's gate under the current localise configuration) and the nearest voxel of any kind.
 *   TLOAM_DIFF_SURFACE   an eligible voxel was found and fabs(r) <= plane_tol, r = (n_x*d_x + n_y*d_y) + n_z*d_z
 *   TLOAM_DIFF_OCCUPIED  not SURFACE, and the nearest voxel has D <= near * near
 *   TLOAM_DIFF_NEW       every other valid point
 *   ids: the voxel that explained the point (-1: INVALID, NEW).  A valid point whose own cell is an occupied voxel adds 1 to that
 *   voxel's `hits` (ungated, whatever its label).
 * Map side: the rays are the scan's points in order, from O to E; the skip rule, the walk, the miss test and the counters are the
 * carve's (above) with max_range, end_margin and radius of THIS configuration, and a miss adds 1 to the voxel's `through`.  An
 * INVALID point is a skipped ray.
 * `through` and `hits` are int64 per voxel in id order, cleared by every call unless flags holds TLOAM_DIFF_ACCUMULATE: the call
 * then adds to what is there.  The labels are per call.  All sums are integers: two calls, and two contexts, give the same bytes.
 * The counts go with the closed map (whatever empties or replaces it, a snapshot load too); a carve or a surfel pass leaves them.
 * They are not part of a snapshot. */
#define TLOAM_DIFF_ACCUMULATE 1
enum { TLOAM_DIFF_INVALID = 0, TLOAM_DIFF_SURFACE = 1, TLOAM_DIFF_OCCUPIED = 2, TLOAM_DIFF_NEW = 3 };
typedef struct tloam_closed_map_diff_config {   /* the defaults are choices, not measurements */
  double max_range;     /* 60: a longer ray is skipped (m); > 0, finite */
  double end_margin;    /* 1.0: nothing is seen through within this of the return (m); >= 0, finite */
  double radius;        /* 0.25 (the carve's): the largest distance from a centroid to a ray that sees through it (m); > 0 */
  double plane_tol;     /* 0.1 (the localiser's min_residual): SURFACE when |r| <= plane_tol (m); >= 0, finite */
  double near;          /* 0.5: OCCUPIED when the nearest centroid of the 27 cells is within it (m); >= 0, finite.  The 27 cells
                         * hold every centroid within `near` of the point while near <= voxel */
  int64_t min_miss;     /* 3: the carve gate's M >= min_miss */
  double miss_ratio;    /* 1.0: ... && M > miss_ratio * N; not NaN */
  int32_t carve_gate;   /* 0; 1: voxels the carved read leaves out explain no point (needs a carved map) */
  int32_t reserved0;
} tloam_closed_map_diff_config;
void tloam_closed_map_diff_default_config(tloam_closed_map_diff_config* cfg);
/* cfg NULL: the defaults.  A value out of its range (NaN too): TLOAM_E_INVALID, and the old configuration stays.  Drops the
 * counts, not the closed map; persists across tloam_odometry_reset. */
int tloam_closed_map_diff_configure(tloam_ctx* ctx, const tloam_closed_map_diff_config* cfg);
typedef struct tloam_closed_map_diff_info {
  int64_t n_points;         /* of the call's scan */
  int64_t n_invalid, n_surface, n_occupied, n_new;   /* its labels */
  int64_t rays;             /* = n_points */
  int64_t skipped_rays;
  int64_t steps;            /* cells visited by the call's rays */
  int64_t tested;           /* ... of them occupied */
  int64_t through;          /* the sum of the stored `through` */
  int64_t voxels_through;   /* voxels with through > 0 */
  int64_t voxels_hit;       /* voxels with hits > 0 */
  int64_t scans;            /* scans that have gone into the stored counts */
  int32_t launches;         /* kernel launches of the call: the same for every input with equal prepared / accumulate */
  int32_t prepared;         /* 1: the call rebuilt the cached voxel records (one more launch) */
  int32_t cleared;          /* 1: the call cleared the counts first (no TLOAM_DIFF_ACCUMULATE) */
  int32_t reserved0;
} tloam_closed_map_diff_info;
/* Of the last diff; zero when there are no counts. */
int tloam_closed_map_get_diff_info(tloam_ctx* ctx, tloam_closed_map_diff_info* info);
/* Diffs points_aos (n points, sensor frame) at pose_colmajor (a rigid transform, checked as the localiser's prior).  labels [n]
 * (uint8) and ids [n] may be NULL.  TLOAM_E_NOT_READY without a built closed map with surfels, or with carve_gate set on a map
 * that is not carved; TLOAM_E_INVALID for n == 0, a NULL scan or pose, unknown flags, a pose that is not a rigid transform.  A
 * refused call leaves everything as it was.  One upload of the scan, a fixed set of launches, one wait. */
int tloam_closed_map_diff(tloam_ctx* ctx, const double* points_aos, size_t n, const double* pose_colmajor, int flags,
                          uint8_t* labels_or_null, int32_t* ids_or_null, tloam_closed_map_diff_info* info_or_null);
/* through and hits of voxels [first, first + count) in id order (either may be NULL).  TLOAM_E_NOT_READY without counts. */
int tloam_closed_map_read_diff(tloam_ctx* ctx, size_t first, size_t count, int64_t* through, int64_t* hits);
/* tloam_closed_map_read_carved's rule (the box; lo and hi both NULL: the whole map), order and capacity convention, keeping
 * exactly the voxels with through >= min_through && (double) through > gone_ratio * (double) hits.  counts: N.  Any output may
 * be NULL.  TLOAM_E_NOT_READY without counts. */
int tloam_closed_map_read_gone(tloam_ctx* ctx, const double* lo_or_null, const double* hi_or_null, int64_t min_through,
                               double gone_ratio, size_t capacity, size_t* n, double* centroids_aos, int64_t* counts,
                               int64_t* through, int64_t* hits);
/* Every diff call on a context with nranks > 1: TLOAM_E_INVALID. */

/* ---- the closed map ray-cast: predicted ranges along segments from a pose (additive to ABI 8) ------
 * From this pose, what should the sensor see?  A ray-cast reads the built closed map with its surfels and writes nothing of
 * them: it runs on a detached (loaded) map, only when called, and no frame, map, carve, surfel, diff count, localisation or
 * snapshot changes by a bit.
 * Per segment end p (sensor frame) and pose matrix M, used as it stands: the ray is the segment from O = (M[12], M[13], M[14])
 * to E = M p as the localiser forms it ("direction d out to 80 m" is the end 80 d).  The skip rule, the set-up and the stepping
 * are the carve's (above) with max_range of THIS configuration; a skipped ray has status TLOAM_RAYCAST_SKIPPED, range -1, id -1.
 * Visited: the start cell, then every cell stepped into, the END CELL INCLUDED (n + 1 cells for n steps; a segment inside one
 * cell visits that cell).  A visited cell that is a voxel COUNTS when N >= min_count and, with carve_gate set, the carved read
 * would not leave it out (left out: M >= min_miss && (double) M > miss_ratio * (double) N, M the stored misses).
 * Per counting voxel with the localiser's record {c, n, eligible} (eligible: the localiser's gate under the current localise and
 * surfel configuration), D = E - O, DD = (Dx*Dx + Dy*Dy) + Dz*Dz, L = sqrt(DD):
 *   u = c - O,  tt = ((ux*Dx + uy*Dy) + uz*Dz) / DD,  w = u - tt * D
 *   centroid test: a hit when 0 <= tt && tt <= 1 && (wx*wx + wy*wy) + wz*wz <= radius2; then t = tt
 *   plane test, used INSTEAD when planes != 0, the voxel is eligible and den = (nx*Dx + ny*Dy) + nz*Dz != 0:
 *     tp = ((nx*ux + ny*uy) + nz*uz) / den,  e = tp * D - u
 *     a hit when 0 <= tp && tp <= 1 && (ex*ex + ey*ey) + ez*ez <= radius2; then t = tp
 *   planes == 2: a counting voxel that is not eligible or has den == 0 is passed through untested (not counted in `tested`)
 *   radius = radius_cells * voxel and radius2 = radius * radius, formed on the host in that order
 * The first hit in visiting order ends the walk: status TLOAM_RAYCAST_HIT_CENTROID or _HIT_PLANE, range = t * L, id the voxel.
 * No hit by the end cell: TLOAM_RAYCAST_MISS, range -1, id -1.  All sums are integers: two calls, and two contexts, give the
 * same bytes.  Nothing is stored beyond the last info and the configuration; whatever drops the closed map clears the info. */
#define TLOAM_RAYCAST_SKIPPED 0
#define TLOAM_RAYCAST_MISS 1
#define TLOAM_RAYCAST_HIT_CENTROID 2
#define TLOAM_RAYCAST_HIT_PLANE 3
typedef struct tloam_closed_map_raycast_config {   /* the defaults are choices, not measurements */
  double max_range;     /* 120: a longer segment is skipped (m); > 0, finite */
  double radius_cells;  /* 0.75: the largest distance from the ray to a centroid (centroid test) or from the plane's crossing to
                         * the centroid (plane test), in voxel sizes; > 0, <= 2, finite */
  int64_t min_count;    /* 1: a voxel with fewer points is passed through; >= 1 */
  int64_t min_miss;     /* 3: the carve gate's M >= min_miss; >= 0 */
  double miss_ratio;    /* 1.0: ... && M > miss_ratio * N; not NaN */
  int32_t planes;       /* 1; 0: the centroid test alone, 1: the plane test where it applies, 2: the plane test alone */
  int32_t carve_gate;   /* 0; 1: voxels the carved read leaves out are passed through (needs a carved map) */
} tloam_closed_map_raycast_config;
void tloam_closed_map_raycast_default_config(tloam_closed_map_raycast_config* cfg);
/* cfg NULL: the defaults.  A value out of its range (NaN too): TLOAM_E_INVALID, and the old configuration stays.  Clears the
 * last info, not the closed map; persists across tloam_odometry_reset. */
int tloam_closed_map_raycast_configure(tloam_ctx* ctx, const tloam_closed_map_raycast_config* cfg);
typedef struct tloam_closed_map_raycast_info {
  int64_t rays;             /* n of the call */
  int64_t skipped, missed, hits_centroid, hits_plane;   /* its statuses */
  int64_t steps;            /* cells visited, the hit cell included */
  int64_t tested;           /* counting voxels that were put to a test */
  int32_t launches;         /* kernel launches of the call: 1, or 2 when prepared */
  int32_t prepared;         /* 1: the call rebuilt the cached voxel records (one more launch) */
} tloam_closed_map_raycast_info;
/* Of the last ray-cast; zero when there has been none since the closed map was last dropped. */
int tloam_closed_map_get_raycast_info(tloam_ctx* ctx, tloam_closed_map_raycast_info* info);
/* Casts the n >= 1 segments ends_aos (sensor frame) at pose_colmajor (a rigid transform, checked as the localiser's prior).
 * status_out [n] (uint8) and range_out [n] (double, metres along the segment) are written for every ray, ids_out [n] when it
 * is not NULL.  TLOAM_E_NOT_READY without a built closed map with surfels, or with carve_gate set on a map that is not carved;
 * TLOAM_E_INVALID for n == 0, a NULL ends, pose, status_out or range_out, a pose that is not a rigid transform, or nranks > 1.
 * A refused call leaves every output buffer and all stored state as it was.  One upload of the ends, one launch (two when the
 * voxel records are stale: the records stay ready for the next localise or diff), one wait. */
int tloam_closed_map_raycast(tloam_ctx* ctx, const double* ends_aos, size_t n, const double* pose_colmajor, uint8_t* status_out,
                             double* range_out, int32_t* ids_out_or_null, tloam_closed_map_raycast_info* info_or_null);

/* ---- free space for the closed map: an occupancy grid from the rays (additive to ABI 8) ------
 * A grid beside the closed map that records where rays saw THROUGH, so that a cell reads occupied, free or unknown.  Off until
 * tloam_closed_map_free_reset; nothing of the map, the carve, the surfels, a diff's counts, the localiser or the snapshot
 * changes by a bit, and the grid is not saved.  Whatever drops the closed map (a build, a load, the configures that empty it)
 * drops the grid; tloam_closed_map_extend leaves it alone: occupancy is resolved when the grid is READ, against the map as it
 * then is, so new voxels need no rewrite.
 * Storage: dense bricks of 4 x 4 x 4 cells of the map's grid (the same voxel and origin), one uint64 a brick, bit
 * ((cz & 3) << 4) | ((cy & 3) << 2) | (cx & 3) set when a ray saw through cell c; the brick of a cell is c >> 2 per axis
 * (flooring), the grid a box of bricks fixed at the reset, brick (bx, by, bz) at word ((bz - bz_lo) * nby + (by - by_lo)) * nbx
 * + (bx - bx_lo).  Cells outside the box are counted, not recorded.
 * The free condition of a ray from O to E (set-up, skip rule, visited cells and stepping are the carve's: the start cell and the
 * first n - 1 cells stepped into, the end cell never): a visited cell has an entry parameter t_in, 0 for the start cell, else
 * the tMax of the axis the step into it took, read before the step updates it; with tlim = 1.0 - end_margin / L the cell is
 * marked when t_in < tlim, whether or not the map has a voxel there.  The marked cells are a prefix of the visited ones; a ray
 * with L <= end_margin marks nothing.
 * A voxel COUNTS when N >= min_count and not (carve_gate && M >= min_miss && (double) M > miss_ratio * (double) N).
 * All sums are integers and bits are only ever set: two calls, and two contexts, give the same bytes.
 * Every call here on a context with nranks > 1: TLOAM_E_INVALID. */
#define TLOAM_OCCUPANCY_INVALID 0    /* the point is not finite, or its cell has |i| >= 2^20 */
#define TLOAM_OCCUPANCY_UNKNOWN 1
#define TLOAM_OCCUPANCY_FREE 2       /* not a counting voxel, inside the box, its bit set */
#define TLOAM_OCCUPANCY_OCCUPIED 3   /* the cell is a voxel that counts */
typedef struct tloam_closed_map_free_config {   /* the defaults are choices, not measurements */
  double max_range;     /* 60: a longer ray is skipped (m); > 0, finite */
  double end_margin;    /* 1.0: a cell entered within this distance of the ray's end is not marked (m); >= 0, finite */
  int64_t max_bytes;    /* 1 GiB: a reset whose grid needs more is refused; >= 8 */
  int64_t min_count;    /* 1: a voxel with fewer points does not count; >= 1 */
  int64_t min_miss;     /* 3: the carve gate's M >= min_miss; >= 0 */
  double miss_ratio;    /* 1.0: ... && M > miss_ratio * N; not NaN */
  int32_t ray_mask;     /* 0: the build's cloud mask; else the keyframe clouds whose points are rays (bit side * 4 + kind), <= 0xFF */
  int32_t carve_gate;   /* 0; 1: voxels the carved read leaves out do not count (needs a carved map when the grid is read) */
} tloam_closed_map_free_config;
void tloam_closed_map_free_default_config(tloam_closed_map_free_config* cfg);
/* cfg NULL: the defaults.  A value out of its range (NaN too): TLOAM_E_INVALID, and the old configuration stays.  Drops the
 * grid, not the closed map; persists across tloam_odometry_reset. */
int tloam_closed_map_free_configure(tloam_ctx* ctx, const tloam_closed_map_free_config* cfg);
typedef struct tloam_closed_map_free_info {
  int64_t lo_cells[3];      /* the box: its lowest cell per axis (a multiple of 4) ... */
  int64_t n_bricks[3];      /* ... its bricks per axis ... */
  int64_t bytes;            /* ... and 8 * n_bricks[0] * n_bricks[1] * n_bricks[2] */
  int64_t keyframes;        /* cumulative: keyframes [0, keyframes) have been walked by _free_add_keyframes */
  int64_t scans;            /* cumulative: _free_add_scan calls */
  int64_t free_cells;       /* popcount of the grid */
  int64_t bricks_nonzero;
  int64_t rays;             /* of the last add: its rays ... */
  int64_t skipped_rays;
  int64_t cells_marked;     /* ... the cells with the free condition inside the box, counted with multiplicity ... */
  int64_t cells_outside;    /* ... and the same outside the box */
  int32_t launches;         /* kernel launches of the last reset (1) or add (2) */
  int32_t reserved0;
} tloam_closed_map_free_info;
/* All zero when there is no grid. */
int tloam_closed_map_get_free_info(tloam_ctx* ctx, tloam_closed_map_free_info* info);
/* Allocates and zeroes the grid over the cells [lo_cells, hi_cells] (inclusive, rounded out to bricks), or with both NULL over
 * the auto box: over the K poses the closed map holds, per axis c_k = floor((O_k - o) / v), R = (int64) ceil(max_range / v) + 1,
 * lo = min c_k - R, hi = max c_k + R, both clamped to +-(2^20 - 1), formed on the host in double in that order (without a
 * pose: the cell 0); every non-skipped keyframe ray lies inside it.  TLOAM_E_INVALID for one NULL, lo > hi, a cell with
 * |c| >= 2^20 or a grid of more than max_bytes; TLOAM_E_NOT_READY without a built closed map.  A refused reset leaves the
 * previous grid as it was.  One launch, one wait. */
int tloam_closed_map_free_reset(tloam_ctx* ctx, const int64_t* lo_cells_or_null, const int64_t* hi_cells_or_null);
/* Walks the rays of keyframes [info.keyframes, K), K the keyframes the closed map holds: the ones the grid has not seen (after an
 * extend, the new ones).  Ray set, order, O, E and skip rule are tloam_closed_map_carve's, under ray_mask.  TLOAM_E_NOT_READY
 * without a grid, or on a map loaded without its clouds.  Two launches, one wait. */
int tloam_closed_map_free_add_keyframes(tloam_ctx* ctx, tloam_closed_map_free_info* info_or_null);
/* Walks the rays of the n >= 1 points points_aos (sensor frame) at pose_colmajor (a rigid transform, checked as the diff's): O,
 * E and ray order are tloam_closed_map_diff's.  This is how a map loaded without its clouds gains free space.  TLOAM_E_NOT_READY
 * without a grid; TLOAM_E_INVALID for n == 0, a NULL points or pose, or a bad pose; a refused call changes nothing.  Two
 * launches, one wait. */
int tloam_closed_map_free_add_scan(tloam_ctx* ctx, const double* points_aos, size_t n, const double* pose_colmajor,
                                   tloam_closed_map_free_info* info_or_null);
/* The grid's words [first, first + count) as they stand (the layout above): what a caller that keeps or ships a grid reads, and
 * what the tests compare bit for bit.  TLOAM_E_NOT_READY without a grid, TLOAM_E_INVALID for a range beyond the grid. */
int tloam_closed_map_read_free_words(tloam_ctx* ctx, size_t first, size_t count, uint64_t* words);
/* The state of n >= 1 points (pose NULL: in the map frame; else in the sensor frame of pose_colmajor): state_out [n] (uint8,
 * TLOAM_OCCUPANCY_*), ids_out [n] when not NULL (the voxel for OCCUPIED, else -1), counts_out [4] when not NULL (points per
 * state).  TLOAM_E_NOT_READY without a grid, or with carve_gate set on a map that is not carved.  One launch, one wait. */
int tloam_closed_map_occupancy(tloam_ctx* ctx, const double* points_aos, size_t n, const double* pose_colmajor_or_null,
                               uint8_t* state_out, int32_t* ids_out_or_null, int64_t* counts_out_or_null);
/* The centres o + (c + 0.5) * v of the FREE cells (a cell that is a counting voxel is left out), brick index ascending, then bit
 * ascending; lo and hi (both or neither) a metric box applied to the centres, inclusive.  *n: their number; with capacity < *n
 * nothing is written and TLOAM_E_INVALID is returned (tloam_closed_map_read_box's convention). */
int tloam_closed_map_read_free(tloam_ctx* ctx, const double* lo_or_null, const double* hi_or_null, size_t capacity, size_t* n,
                               double* centres_aos);
/* A 2-D grid over the box's x-y footprint, y outer: *nx = 4 n_bricks[0], *ny = 4 n_bricks[1], state_out [*ny * *nx] (uint8).  The
 * band is the cells floor((z_lo - o_z) / v) .. floor((z_hi - o_z) / v) clipped to the box.  A column is OCCUPIED if any band
 * cell is a counting voxel, else FREE if at least min_free >= 1 band cells are FREE, else UNKNOWN.  TLOAM_E_INVALID for
 * z_lo > z_hi, a bound that is not finite or min_free < 1; with capacity < *ny * *nx nothing is written, the size is reported
 * and TLOAM_E_INVALID is returned. */
int tloam_closed_map_free_columns(tloam_ctx* ctx, double z_lo, double z_hi, int64_t min_free, uint8_t* state_out, size_t capacity,
                                  size_t* nx, size_t* ny);

/* ---- clearance for the closed map: a truncated distance field over the free-space box, and path checks (additive to ABI 8) ----
 * A dense field over the free-space grid's box: nx = 4 n_bricks[0], ny = 4 n_bricks[1], nz = 4 n_bricks[2] cells, one uint16 a
 * cell, row-major [z][y][x], x fastest, element (x, y, z) the cell lo_cells + (x, y, z).  The value is d2, the squared distance
 * IN CELLS, between integer cell coordinates, from the cell to the nearest obstacle cell.  Truncated: with
 * R = (int) ceil(max_distance / voxel), formed on the host in double, a value <= R * R is stored exact and anything larger is
 * TLOAM_CLEARANCE_BEYOND.  R must lie in 1 .. 128.
 * Obstacle cells: the states are tloam_closed_map_occupancy's at the moment of the build, under the free configuration's
 * min_count / min_miss / miss_ratio / carve_gate.  An OCCUPIED cell is an obstacle.  With unknown_is_obstacle an UNKNOWN cell is
 * one too, and everything outside the box is unknown (the nearest outside cell of an inside cell lies in the layer next to the
 * box).  Without it nothing outside the box contributes: the values within R cells of a face of the box are then upper bounds.
 * Metric meaning: voxel * sqrt(d2) is the distance between the two cells' centres; any point of the cell is at least
 * voxel * (sqrt(d2) - sqrt(3)) from any point of the obstacle cell.  That margin is the planner's to take.
 * The field is built by tloam_closed_map_clearance_build and is dropped by whatever changes what it was built from: everything
 * that drops the free-space grid, tloam_closed_map_free_reset, tloam_closed_map_free_add_keyframes / _free_add_scan (once their
 * arguments and the grid have been accepted: whether or not the add then succeeds), a successful tloam_closed_map_extend,
 * tloam_closed_map_carve, the carve's configure, tloam_closed_map_clearance_configure.  After a drop every read of
 * the field is TLOAM_E_NOT_READY until the next build.  It is not saved in a snapshot; nothing else in the context changes by a
 * bit.  All values are integers: two builds, and two contexts, give the same bytes.
 * Every call here on a context with nranks > 1: TLOAM_E_INVALID. */
#define TLOAM_CLEARANCE_BEYOND 0xFFFF    /* no obstacle within R cells */
#define TLOAM_CLEARANCE_OUTSIDE 0xFFFE   /* a queried cell outside the box (unknown_is_obstacle 0), or an INVALID point */
#define TLOAM_CLEARANCE_SKIPPED 0        /* the segment is one ray_begin refuses (the ray-cast's skip rule, max_range = max_segment) */
#define TLOAM_CLEARANCE_CLEAR 1          /* every visited cell has d2 >= need */
#define TLOAM_CLEARANCE_BLOCKED 2        /* the walk met a cell with d2 < need */
#define TLOAM_CLEARANCE_LEFT_BOX 3       /* unknown_is_obstacle 0: the walk met a cell outside the box (status "OUTSIDE") */
typedef struct tloam_closed_map_clearance_config {   /* the defaults are choices, not measurements */
  double max_distance;          /* 4.0: the truncation (m); > 0, finite; R = ceil(max_distance / voxel) is checked at the build */
  double max_segment;           /* 120: a longer segment is skipped (m); > 0, finite */
  int64_t max_bytes;            /* 1 GiB: a build whose field (both of its buffers) needs more is refused; >= 2 */
  int32_t unknown_is_obstacle;  /* 1; 0: only OCCUPIED cells are obstacles */
  int32_t reserved0;
} tloam_closed_map_clearance_config;
void tloam_closed_map_clearance_default_config(tloam_closed_map_clearance_config* cfg);
/* cfg NULL: the defaults.  A value out of its range (NaN too): TLOAM_E_INVALID, and the old configuration stays.  Drops the
 * field, not the free-space grid; persists across tloam_odometry_reset. */
int tloam_closed_map_clearance_configure(tloam_ctx* ctx, const tloam_closed_map_clearance_config* cfg);
typedef struct tloam_closed_map_clearance_info {
  int64_t lo_cells[3];      /* the box: its lowest cell per axis ... */
  int64_t n_cells[3];       /* ... its cells per axis (nx, ny, nz) ... */
  int64_t bytes;            /* ... and what the field holds on the device: 2 buffers * 2 bytes * nx * ny * nz */
  int64_t obstacle_cells;   /* cells with d2 == 0 */
  int64_t finite_cells;     /* cells with d2 != TLOAM_CLEARANCE_BEYOND */
  int64_t sum_d2;           /* over the finite cells */
  int64_t max_d2;           /* over the finite cells (0 when there is none) */
  int32_t radius_cells;     /* R */
  int32_t launches;         /* kernel launches of the build: the same for every input */
} tloam_closed_map_clearance_info;
/* Resolves the states, runs the three passes, counts; one wait.  TLOAM_E_NOT_READY without a built map and a free-space grid, or
 * with carve_gate set on a map that is not carved; TLOAM_E_INVALID for R outside 1 .. 128 or a field of more than max_bytes.  A
 * refused build leaves the previous field as it was. */
int tloam_closed_map_clearance_build(tloam_ctx* ctx, tloam_closed_map_clearance_info* info_or_null);
/* All zero when there is no field. */
int tloam_closed_map_get_clearance_info(tloam_ctx* ctx, tloam_closed_map_clearance_info* info);
/* The field's values [first, first + count) as they stand (tloam_closed_map_read_free_words' conventions). */
int tloam_closed_map_read_clearance(tloam_ctx* ctx, size_t first, size_t count, uint16_t* d2);
/* Per point (pose NULL: in the map frame; else in the sensor frame of pose_colmajor): state_out [n] as tloam_closed_map_occupancy
 * gives it, d2_out [n] the value of the point's cell -- a cell outside the box gives 0 with unknown_is_obstacle, else
 * TLOAM_CLEARANCE_OUTSIDE; an INVALID point gives TLOAM_CLEARANCE_OUTSIDE --, distance_out [n] when not NULL
 * voxel * sqrt((double) d2), +inf for BEYOND and NaN for OUTSIDE, counts_out [4] when not NULL (points per state).  One launch,
 * one wait. */
int tloam_closed_map_clearance_points(tloam_ctx* ctx, const double* points_aos, size_t n, const double* pose_colmajor_or_null,
                                      uint8_t* state_out, uint16_t* d2_out, double* distance_out_or_null,
                                      int64_t* counts_out_or_null);
/* The batched edge check: is the segment starts[i] -> ends[i] clear for a body of `radius` (m)?  need = (int64) ceil(q * q) with
 * q = radius / voxel, formed on the host in double in that order; radius must be finite and >= 0, and need <= R * R + 1 (the
 * field cannot vouch for more than R cells): else TLOAM_E_INVALID.  The walk is the ray-cast's (set-up, skip rule and stepping,
 * max_range = max_segment): the start cell and every cell stepped into, the end cell included.  Each visited cell has the free
 * walk's t_in (0 for the start cell, else the tMax of the axis the step into it took, read before the step) and a d2 read as
 * tloam_closed_map_clearance_points reads it.  The walk stops at the first cell outside the box when unknown_is_obstacle is 0
 * (LEFT_BOX; that cell does not enter min_d2) and at the first cell with d2 < need (BLOCKED); else it runs to the end (CLEAR).
 * status_out [n]; min_d2_out [n] the minimum of d2 over the visited cells, the stopping one included (BEYOND when none entered;
 * TLOAM_CLEARANCE_OUTSIDE for SKIPPED); t_block_out [n] when not NULL the stopping cell's t_in, -1.0 for CLEAR and SKIPPED;
 * counts_out [4] when not NULL (segments per status).  need == 0 never blocks: the call then reports the path's minimum
 * clearance.  One launch, one wait. */
int tloam_closed_map_clearance_segments(tloam_ctx* ctx, const double* starts_aos, const double* ends_aos, size_t n,
                                        const double* pose_colmajor_or_null, double radius, uint8_t* status_out,
                                        uint16_t* min_d2_out, double* t_block_out_or_null, int64_t* counts_out_or_null);
/* The 2-D field over tloam_closed_map_free_columns' states (the same band, min_free, sizes and capacity convention): a column's
 * d2 to the nearest OCCUPIED (with unknown_is_obstacle: or UNKNOWN, or outside) column, under the same R.  Computed per call from
 * the free-space grid, not stored: it needs no built field.  state_out [*ny * *nx] when not NULL, d2_out [*ny * *nx].  Its two
 * layers (4 bytes a column) are held to max_bytes as the field is: more is TLOAM_E_INVALID. */
int tloam_closed_map_clearance_columns(tloam_ctx* ctx, double z_lo, double z_hi, int64_t min_free, uint8_t* state_out_or_null,
                                       uint16_t* d2_out, size_t capacity, size_t* nx, size_t* ny);

/* ---- the route through the closed map: a cost-to-go field from goals, its reads and paths (additive to ABI 8) -------
 * A dense field over the built clearance field's box (nx, ny, nz cells, row-major [z][y][x], x fastest, element (x, y, z) the
 * cell lo_cells + (x, y, z)), one uint32 a cell: the least total weight of a chain of moves from the cell to any accepted goal.
 * Traversable cells: need = (int64) ceil(q * q) with q = radius / voxel, formed on the host in double in that order
 * (tloam_closed_map_clearance_segments' need, by the same function); radius must be finite and >= 0 and need <= R * R + 1, else
 * TLOAM_E_INVALID.  A cell is traversable iff its d2 >= max(need, 1); TLOAM_CLEARANCE_BEYOND passes every need.  An UNKNOWN
 * cell is traversable or not through unknown_is_obstacle at the clearance build alone, which made its d2 zero or not.  Nothing
 * outside the box is traversable, whatever unknown_is_obstacle says.
 * Moves: 26-connected, allowed between any two traversable cells that differ by at most one on every axis, WITH NO FURTHER
 * CORNER RULE: a diagonal move is allowed when the face-adjacent cells it passes between are not traversable.  A planner
 * confirms a path with tloam_closed_map_clearance_segments.  Weights: the 3-4-5 chamfer, 3 for a face step, 4 for an edge step,
 * 5 for a vertex step.  The value is 0 at an accepted goal's cell, TLOAM_ROUTE_UNREACHED at a traversable cell no goal reaches
 * and TLOAM_ROUTE_BLOCKED at a cell that is not traversable.  A build is refused (TLOAM_E_INVALID) when
 * 5 * cells >= TLOAM_ROUTE_OUTSIDE: no cost can meet a sentinel.
 * Metric length: voxel * (double) cost / 3.0, in that order.  The 3-4-5 mask is Borgefors' ("Distance transformations in
 * arbitrary dimensions", CVGIP 27, 1984; "Distance transformations in digital images", CVGIP 34, 1986).  Over free space a
 * displacement (a >= b >= c >= 0) costs 3 a + b + c, so cost / 3 lies between 0.9428 (= (4 / 3) / sqrt(2), the face diagonal)
 * and 1.1055 (= sqrt(11 / 9), at b = c = a / 3) times the Euclidean length; with 3 and 4 alone in a plane between 0.9428 and
 * 1.0541 (= sqrt(10 / 9)).  Along the axes it is exact.  DESIGN.md section 31 has the two lines of the derivation.
 * Goals: n >= 1 points, in the map frame (pose NULL) or in the sensor frame of pose_colmajor.  A goal whose cell is traversable
 * is accepted, duplicates each counted; any other -- outside the box, an INVALID point, a cell that is not traversable -- is
 * rejected.  With no goal accepted the build is TLOAM_OK and every traversable cell is TLOAM_ROUTE_UNREACHED.
 * The field is built by tloam_closed_map_route_build and dropped with the clearance field (everything that drops it), by a
 * successful tloam_closed_map_clearance_build (the field it was built from is replaced) and by
 * tloam_closed_map_route_configure.  After a drop every read is TLOAM_E_NOT_READY until the next build.  It is not saved in a
 * snapshot; nothing else in the context changes by a bit.
 * The field is the unique fixpoint of min-plus relaxation, so every byte of it, and every info field but the four marked
 * DIAGNOSTIC below, is the same for two builds and for two contexts.  tile_updates, rounds, launches and waits depend on the
 * order in which the device's blocks saw each other's values and MAY DIFFER FROM RUN TO RUN.
 * Every call here on a context with nranks > 1: TLOAM_E_INVALID. */
#define TLOAM_ROUTE_UNREACHED 0xFFFFFFFFu   /* a traversable cell no accepted goal reaches */
#define TLOAM_ROUTE_BLOCKED 0xFFFFFFFEu     /* a cell that is not traversable */
#define TLOAM_ROUTE_OUTSIDE 0xFFFFFFFDu     /* a queried cell outside the box, or an INVALID point */
#define TLOAM_ROUTE_PATH_OUTSIDE 0          /* the start is outside the box or INVALID: no waypoint */
#define TLOAM_ROUTE_PATH_REACHED 1          /* the path ends at a cell of cost 0 */
#define TLOAM_ROUTE_PATH_UNREACHED 2        /* the start's cell is TLOAM_ROUTE_UNREACHED: no waypoint */
#define TLOAM_ROUTE_PATH_BLOCKED 3          /* the start's cell is TLOAM_ROUTE_BLOCKED: no waypoint */
#define TLOAM_ROUTE_PATH_TRUNCATED 4        /* the path has more than max_cells cells: the first max_cells are written */
typedef struct tloam_closed_map_route_config {   /* choices, not measurements */
  int64_t max_bytes;         /* 1 GiB: a build whose field and tile flags need more is refused; >= 4 */
  int32_t max_rounds;        /* 65536: a build that needs more rounds fails; >= 1 */
  int32_t rounds_per_wait;   /* 16: rounds enqueued between two waits of the host; 1 .. 1024 */
} tloam_closed_map_route_config;
void tloam_closed_map_route_default_config(tloam_closed_map_route_config* cfg);
/* cfg NULL: the defaults.  A value out of its range: TLOAM_E_INVALID, and the old configuration stays.  Drops the route field
 * only; persists across tloam_odometry_reset. */
int tloam_closed_map_route_configure(tloam_ctx* ctx, const tloam_closed_map_route_config* cfg);
typedef struct tloam_closed_map_route_info {
  int64_t lo_cells[3];         /* the box: its lowest cell per axis ... */
  int64_t n_cells[3];          /* ... its cells per axis (nx, ny, nz) ... */
  int64_t bytes;               /* ... and what the field holds on the device: 4 bytes a cell and 8 bytes a tile of flags */
  int64_t need;                /* a cell is traversable iff d2 >= max(need, 1) */
  int64_t goals_accepted;
  int64_t goals_rejected;
  int64_t traversable_cells;   /* cells whose value is not TLOAM_ROUTE_BLOCKED */
  int64_t reached_cells;       /* cells with a cost */
  int64_t sum_cost;            /* over the reached cells */
  int64_t max_cost;            /* over the reached cells (0 when there is none) */
  int64_t tile_updates;        /* DIAGNOSTIC: tiles relaxed, over all rounds */
  int32_t rounds;              /* DIAGNOSTIC: rounds that ran until one marked nothing */
  int32_t launches;            /* DIAGNOSTIC: kernel launches of the build */
  int32_t waits;               /* DIAGNOSTIC: waits of the host */
  int32_t reserved0;
} tloam_closed_map_route_info;
/* Seeds the field from the clearance field and the goals, relaxes it in rounds (rounds_per_wait launches between two waits)
 * until a round lowers nothing, counts.  TLOAM_E_NOT_READY without a built clearance field; TLOAM_E_INVALID for n == 0, a NULL
 * goals, a bad pose, a bad radius, a field and flags of more than max_bytes or 5 * cells >= TLOAM_ROUTE_OUTSIDE: a refused
 * build leaves the previous route field as it was.  A failure after the first launch drains the stream and drops the field;
 * running out of max_rounds drops the field and returns TLOAM_E_HIP, tloam_last_error naming the cap. */
int tloam_closed_map_route_build(tloam_ctx* ctx, const double* goals_aos, size_t n, const double* pose_colmajor_or_null,
                                 double radius, tloam_closed_map_route_info* info_or_null);
/* All zero when there is no field. */
int tloam_closed_map_get_route_info(tloam_ctx* ctx, tloam_closed_map_route_info* info);
/* The field's values [first, first + count) as they stand (tloam_closed_map_read_clearance's conventions). */
int tloam_closed_map_read_route(tloam_ctx* ctx, size_t first, size_t count, uint32_t* cost);
/* Per point (pose NULL: in the map frame; else in the sensor frame of pose_colmajor): cost_out [n] the value of the point's
 * cell, TLOAM_ROUTE_OUTSIDE for a cell outside the box or an INVALID point; distance_out [n] when not NULL
 * voxel * (double) cost / 3.0, +inf for UNREACHED and NaN for BLOCKED and OUTSIDE; counts_out [4] when not NULL: points reached /
 * unreached / blocked / outside.  One launch, one wait. */
int tloam_closed_map_route_points(tloam_ctx* ctx, const double* points_aos, size_t n, const double* pose_colmajor_or_null,
                                  uint32_t* cost_out, double* distance_out_or_null, int64_t* counts_out_or_null);
/* Per start a path descended from the field.  The first waypoint is the start's own cell.  From a cell of cost k > 0 the next
 * cell is the first neighbour, in the order dz outermost, then dy, then dx, each running -1, 0, 1, whose value c satisfies
 * c + w == k, w the weight of that step; the path ends at cost 0.  status_out [n] TLOAM_ROUTE_PATH_*; n_cells_out [n] the
 * waypoints written (0 for OUTSIDE, UNREACHED and BLOCKED); cost_out [n] the value of the start's cell as
 * tloam_closed_map_route_points gives it; centres_aos_out [n * max_cells * 3] the waypoint j of start i at
 * centres[i * max_cells + j], a cell's centre o + (c + 0.5) * v as tloam_closed_map_read_free forms it, entries past n_cells
 * zero.  TRUNCATED: the path has more than max_cells cells and its first max_cells are written; a whole path has at most
 * cost / 3 + 1 cells, so a caller can size max_cells from cost_out.  The walk takes at most max_cells steps and stops as
 * TRUNCATED when no neighbour satisfies the rule: a damaged field cannot make it loop.  max_cells >= 1, and
 * n * max_cells * 24 bytes is held to max_bytes: else TLOAM_E_INVALID.  One launch, one wait. */
int tloam_closed_map_route_paths(tloam_ctx* ctx, const double* starts_aos, size_t n, const double* pose_colmajor_or_null,
                                 size_t max_cells, uint8_t* status_out, int32_t* n_cells_out, uint32_t* cost_out,
                                 double* centres_aos_out);
/* The 2-D form for a ground vehicle, over tloam_closed_map_clearance_columns' layer (the same band, min_free, sizes, capacity
 * convention, R and unknown_is_obstacle): 8-connected, weights 3 and 4, a column traversable iff its d2 >= max(need, 1).  A goal
 * must be a valid point and is placed by its x and y alone.  Computed per call by the relaxation of the 3-D field with nz = 1,
 * not stored: it needs no built field and leaves a built one alone.  state_out [*ny * *nx] and d2_out [*ny * *nx] when not
 * NULL, cost_out [*ny * *nx]; info_or_null as the build's (lo_cells[2] = 0, n_cells[2] = 1).  The layers (4 bytes a column of
 * d2, then 4 bytes a column of cost and the tile flags) are held to the two max_bytes.  Descending the layer is the caller's. */
int tloam_closed_map_route_columns(tloam_ctx* ctx, double z_lo, double z_hi, int64_t min_free, const double* goals_aos, size_t n,
                                   const double* pose_colmajor_or_null, double radius, uint8_t* state_out_or_null,
                                   uint16_t* d2_out_or_null, uint32_t* cost_out, size_t capacity, size_t* nx, size_t* ny,
                                   tloam_closed_map_route_info* info_or_null);

/* ---- the frontiers of the closed map: where free space meets the unknown, clustered (additive to ABI 8) -------
 * A dense field over the free-space grid's box (nx = 4 nbx, ny, nz cells, row-major [z][y][x], x fastest, element (x, y, z) the
 * cell lo_cells + (x, y, z): the clearance's and the route's cells), one uint32 a cell.  The states are tloam_closed_map_occupancy's
 * at the moment of the build, under the free configuration's min_count, min_miss, miss_ratio and carve_gate; a built clearance
 * field is not needed.  A FRONTIER CELL is a FREE cell with at least one of its six face neighbours INSIDE THE BOX UNKNOWN; cells
 * outside the box contribute nothing, neither as unknown neighbours nor to connectivity.  The automatic box of
 * tloam_closed_map_free_reset reaches one cell beyond every ray, so no frontier is lost at its faces; A BOX GIVEN BY THE CALLER IS
 * A REGION OF INTEREST WHOSE FACES MAKE NO FRONTIER.  A CLUSTER is a 26-connected component of the frontier cells; its root is
 * the least linear index (z * ny + y) * nx + x among its cells.  A cell's value is its cluster's root when it is a frontier cell,
 * else one of the three state sentinels below: the field doubles as the dense state array of the box.  A build is refused
 * (TLOAM_E_INVALID) when cells >= TLOAM_FRONTIER_OUTSIDE (an index would meet a sentinel) or when the field and its tile flags
 * are more than max_bytes.
 * Kept clusters: those with cells >= min_cells, listed in ascending root.  Every component is counted in the info; only the kept
 * ones are listed, costed and indexed.  A cluster's centroid is the caller's: o + (lo_cells + sum / cells + 0.5) * v per axis, in
 * double, in that order (sum and cells converted to double first).
 * The field is built by tloam_closed_map_frontier_build and dropped by everything that drops the clearance field because the
 * grid or the map's counting voxels changed (tloam_closed_map_free_configure, _free_reset, _free_add_keyframes, _free_add_scan,
 * a successful tloam_closed_map_extend, whatever drops the carve or the closed map) and by tloam_closed_map_frontier_configure;
 * the clearance's and the route's configure and build leave it alone.  After a drop every read is TLOAM_E_NOT_READY until the
 * next build.  It is not saved in a snapshot; nothing else in the context changes by a bit.
 * The labelling by least index is the unique fixpoint of a min-propagation, so every byte of every output, and every info field
 * but the four marked DIAGNOSTIC below, is the same for two builds and for two contexts.
 * Every call here on a context with nranks > 1: TLOAM_E_INVALID. */
#define TLOAM_FRONTIER_FREE 0xFFFFFFFFu       /* a FREE cell that is no frontier cell */
#define TLOAM_FRONTIER_UNKNOWN 0xFFFFFFFEu    /* an UNKNOWN cell */
#define TLOAM_FRONTIER_OCCUPIED 0xFFFFFFFDu   /* an OCCUPIED cell */
#define TLOAM_FRONTIER_OUTSIDE 0xFFFFFFFCu    /* a queried cell outside the box, or an INVALID point */
#define TLOAM_FRONTIER_ALL 0xFFFFFFFFu        /* tloam_closed_map_read_frontier_cells: the cells of every kept cluster */
typedef struct tloam_closed_map_frontier_config {   /* choices, not measurements */
  int64_t max_bytes;         /* 1 GiB: a build whose field, tile flags and cluster table need more is refused; >= 4 */
  int32_t min_cells;         /* 8: a cluster of fewer cells is counted but not kept; >= 1 */
  int32_t reach;             /* 2: tloam_closed_map_frontier_costs looks this many cells around a cluster's cells; 0 .. 4 */
  int32_t max_rounds;        /* 65536: a build that needs more rounds fails; >= 1 */
  int32_t rounds_per_wait;   /* 16: rounds enqueued between two waits of the host; 1 .. 1024 */
} tloam_closed_map_frontier_config;
void tloam_closed_map_frontier_default_config(tloam_closed_map_frontier_config* cfg);
/* cfg NULL: the defaults.  A value out of its range: TLOAM_E_INVALID, and the old configuration stays.  Drops the frontier field
 * only; persists across tloam_odometry_reset. */
int tloam_closed_map_frontier_configure(tloam_ctx* ctx, const tloam_closed_map_frontier_config* cfg);
typedef struct tloam_closed_map_frontier_cluster {   /* 64 bytes */
  int64_t sum[3];            /* the sums of the cells' box-local x, y, z */
  int32_t lo[3];             /* the inclusive box of the cluster in absolute cells: its lowest ... */
  int32_t hi[3];             /* ... and its highest cell per axis */
  uint32_t root;             /* the least linear index among the cluster's cells: its label in the field */
  uint32_t cells;
  uint32_t unknown_faces;    /* (cell, face) pairs of the cluster that face an UNKNOWN cell: the size of the opening */
  uint32_t reserved;         /* 0 */
} tloam_closed_map_frontier_cluster;
typedef struct tloam_closed_map_frontier_info {
  int64_t lo_cells[3];         /* the box: its lowest cell per axis ... */
  int64_t n_cells[3];          /* ... its cells per axis (nx, ny, nz) ... */
  int64_t bytes;               /* ... and what the field holds on the device: 4 bytes a cell and 8 bytes a tile of flags */
  int64_t free_cells;          /* cells in state FREE, frontier cells among them (the grid's own free_cells is a popcount that
                                  includes bits under counting voxels) */
  int64_t unknown_cells;
  int64_t occupied_cells;      /* the three sum to the box */
  int64_t frontier_cells;
  int64_t clusters;            /* all components */
  int64_t clusters_kept;       /* those with cells >= min_cells */
  int64_t cells_kept;          /* the frontier cells of the kept clusters */
  int64_t largest;             /* the cells of the largest component (0 when there is none) */
  int64_t unknown_faces;       /* over all frontier cells */
  int64_t tile_updates;        /* DIAGNOSTIC: tiles relaxed, over all rounds */
  int32_t rounds;              /* DIAGNOSTIC: rounds that ran until one marked nothing */
  int32_t launches;            /* DIAGNOSTIC: kernel launches of the build */
  int32_t waits;               /* DIAGNOSTIC: waits of the host */
  int32_t reserved0;
} tloam_closed_map_frontier_info;
/* Resolves the states of the box, marks the frontier cells, labels them in rounds (rounds_per_wait launches between two waits)
 * until a round lowers nothing, counts and gathers the clusters.  TLOAM_E_NOT_READY exactly where
 * tloam_closed_map_clearance_build has it: no built map, no grid, or the gate on and not carved.  TLOAM_E_INVALID for a box the
 * contract above refuses: a refused build leaves the previous field as it was.  A failure after the first launch drains the
 * stream and drops the field; running out of max_rounds drops the field and returns TLOAM_E_HIP, tloam_last_error naming the cap,
 * and so does a cluster table (136 bytes a component) that does not fit under max_bytes beside the field once the roots are
 * counted. */
int tloam_closed_map_frontier_build(tloam_ctx* ctx, tloam_closed_map_frontier_info* info_or_null);
/* All zero when there is no field. */
int tloam_closed_map_get_frontier_info(tloam_ctx* ctx, tloam_closed_map_frontier_info* info);
/* The field's values [first, first + count) as they stand (tloam_closed_map_read_route's conventions). */
int tloam_closed_map_read_frontier(tloam_ctx* ctx, size_t first, size_t count, uint32_t* label);
/* The kept clusters in ascending root.  *n_out: their number, always; more than capacity: TLOAM_E_INVALID and nothing written;
 * clusters_out NULL: the number alone (tloam_closed_map_read_box's capacity convention). */
int tloam_closed_map_frontier_clusters(tloam_ctx* ctx, size_t capacity, tloam_closed_map_frontier_cluster* clusters_out,
                                       size_t* n_out);
/* The centres o + (c + 0.5) * v of the frontier cells of the kept cluster of root `root_or_all`, or with TLOAM_FRONTIER_ALL of
 * every kept cluster, in ascending linear index; roots_out [n] when not NULL the root of each.  The same capacity convention.  A
 * root that is not a kept cluster's: *n_out = 0 and TLOAM_OK. */
int tloam_closed_map_read_frontier_cells(tloam_ctx* ctx, uint32_t root_or_all, size_t capacity, double* centres_aos_out,
                                         uint32_t* roots_out_or_null, size_t* n_out);
/* Per point (pose NULL: in the map frame; else in the sensor frame of pose_colmajor): label_out [n] the value of the point's
 * cell, TLOAM_FRONTIER_OUTSIDE for a cell outside the box or an INVALID point; cluster_out [n] when not NULL the index of the
 * cell's cluster in the kept list, else -1; counts_out [5] when not NULL: points frontier / free / unknown / occupied / outside.
 * One launch, one wait. */
int tloam_closed_map_frontier_points(tloam_ctx* ctx, const double* points_aos, size_t n, const double* pose_colmajor_or_null,
                                     uint32_t* label_out, int32_t* cluster_out_or_null, int64_t* counts_out_or_null);
/* The join with the route: TLOAM_E_NOT_READY without a frontier field or without a route field (both lie over the grid's box).
 * Per kept cluster the minimum, over its cells c and over the cells u of the box with max |u - c| <= reach per axis whose route
 * value is a cost (below TLOAM_ROUTE_OUTSIDE), of the key (cost(u) << 32) | linear(u): cost_out [n] the key's high half,
 * approach_aos_out [3 n] when not NULL the centre of the key's cell; TLOAM_ROUTE_UNREACHED and three NaN when there is none.
 * reach is there because with unknown_is_obstacle = 1 a frontier cell has d2 = 1 and is BLOCKED for any body wider than a voxel:
 * the nearest cell the body can stand in is a few cells back.  THE ROUTE'S MOVES ARE SYMMETRIC: a route built from the robot's
 * cell as the one goal gives the robot's cost to every cluster.  Computed per call, not stored; the capacity convention of
 * tloam_closed_map_frontier_clusters.  One launch, one wait. */
int tloam_closed_map_frontier_costs(tloam_ctx* ctx, size_t capacity, uint32_t* cost_out, double* approach_aos_out_or_null,
                                    size_t* n_out);
/* The 2-D form over tloam_closed_map_free_columns' layer (the same band and min_free): the same kernels with nz = 1, so 4 face
 * neighbours and 8-connectivity remain; sum[2] = 0 and lo[2] = hi[2] = the box's lowest z cell.  label_out [ny * nx] (16 nbx nby
 * values: the caller sizes it from the grid's info) when not NULL; the kept clusters by the capacity convention above;
 * info_or_null as the build's (n_cells[2] = 1).  Computed per call, not stored: it needs no built field and leaves a built one
 * alone.  No cost join: the caller's. */
int tloam_closed_map_frontier_columns(tloam_ctx* ctx, double z_lo, double z_hi, int64_t min_free, uint32_t* label_out_or_null,
                                      size_t capacity, tloam_closed_map_frontier_cluster* clusters_out, size_t* n_out,
                                      tloam_closed_map_frontier_info* info_or_null);

/* ---- the view gain of the closed map: the unknown cells seen from candidate poses (additive to ABI 8) -------
 * How much would be learnt from a pose: a sensor's firing pattern cast through the box from the pose, the DISTINCT UNKNOWN cells
 * its rays cross before an OCCUPIED cell or the box stops them, counted.  THE STATE SOURCE is the built frontier field
 * (tloam_closed_map_frontier_build), its values at the moment of the call: a value below TLOAM_FRONTIER_OUTSIDE is a frontier
 * label and counts as free, TLOAM_FRONTIER_FREE is free, TLOAM_FRONTIER_UNKNOWN unknown, TLOAM_FRONTIER_OCCUPIED occupied; a cell
 * outside the box is outside.  Without a frontier field every call here but the configuration's and the info's is
 * TLOAM_E_NOT_READY.  Nothing is stored beyond the configuration and the last info; whatever drops the frontier field clears the
 * info; the frontier field, the route, the clearance, the grid, the map and the snapshot do not change by a bit.
 * A VIEW is a pose matrix M_v (column-major, finite and rigid) and the segment ends p_r in the sensor frame, shared by all
 * views.  Ray (v, r) runs from O = (M_v[12], M_v[13], M_v[14]) to E = M_v p_r, formed as the ray-cast forms it; skip rule, set-up
 * and stepping are the ray-cast's (the carve's) under THIS configuration's max_range.  VISITED are the start cell, then every cell
 * stepped into, THE END CELL INCLUDED (n + 1 cells, the ray-cast's convention).  Per visited cell, in visiting order, the first
 * rule that applies decides: outside the box -- the walk ends, the ray counts in rays_left_box; OCCUPIED -- the walk ends, the
 * ray counts in rays_occupied; UNKNOWN -- the cell's bit is set in the view's window, unknown_visits is incremented, the walk
 * goes on: UNKNOWN SPACE IS TRANSPARENT, the usual optimistic model (a ray is not stopped by what is not known to be there);
 * free, or a frontier label -- free_visits is incremented, the walk goes on.  A ray that passes its end cell counts in
 * rays_ended, a skipped ray in rays_skipped and visits nothing; steps counts the cells visited, the stopping cell included.
 * There is no special case for a bad origin: a view whose origin cell is outside the box ends every ray that is not skipped at
 * its first cell, and with a NaN translation every ray is skipped.
 * THE WINDOW: W = (int) ceil(max_range / voxel) + 1, formed on the host in double, S = 2 W + 1; the cells c with |c - c_O| <= W
 * per axis, c_O = floor((O - o) / v); a cell's bit index is ((dz * S) + dy) * S + dx with d = c - c_O + W, the bits packed in
 * ceil(S^3 / 32) 32-bit words.  Every visited cell of a ray that is not skipped lies inside it (the walk is monotone per axis
 * between the start and the end cell, |floor(s1) - floor(s0)| <= ceil(|s1 - s0|), and the + 1 absorbs the rounding of
 * (E - o) / v); a visited cell beyond it would set no bit and count in the info's beyond_window, which stays 0.
 * Two forms compute the same bytes: the LDS form, one block a view with the window in the CU's LDS, and the global form, the
 * windows of a chunk of views in device memory under max_bytes, a view's rays over several blocks.  Everything is an integer, OR
 * and sum are order-free: two calls, two contexts and the two forms give the same bytes.
 * Every call here on a context with nranks > 1: TLOAM_E_INVALID.  A refused call leaves every output buffer and all state as
 * it was. */
typedef struct tloam_closed_map_view_config {   /* choices, not measurements */
  double max_range;          /* 20: a ray longer than this is skipped, and the window is sized by it; > 0, finite */
  int64_t max_bytes;         /* 256 MiB: the global form's windows of one chunk; >= 4 */
  int32_t lds_bytes;         /* 131072: the largest window the LDS form takes; 0 up to what the device reports as the most
                                shared memory of a block less the kernel's static use */
  int32_t form;              /* 0 auto: the LDS form when the window fits lds_bytes, else the global one; 1 the LDS form: a
                                window that does not fit is TLOAM_E_INVALID at the call; 2 the global form */
} tloam_closed_map_view_config;
void tloam_closed_map_view_default_config(tloam_closed_map_view_config* cfg);
/* cfg NULL: the defaults.  A value out of its range: TLOAM_E_INVALID, and the old configuration stays.  Clears the last info
 * only; persists across tloam_odometry_reset. */
int tloam_closed_map_view_configure(tloam_ctx* ctx, const tloam_closed_map_view_config* cfg);
typedef struct tloam_closed_map_view_record {   /* 64 bytes */
  int64_t unknown_cells;     /* the popcount of the window: THE GAIN */
  int64_t unknown_visits;    /* UNKNOWN cells crossed, with multiplicity */
  int64_t free_visits;       /* free or frontier cells crossed */
  int64_t steps;             /* cells visited, the stopping cell included */
  int32_t rays_skipped;
  int32_t rays_occupied;     /* rays stopped by an OCCUPIED cell */
  int32_t rays_left_box;     /* rays stopped by leaving the box */
  int32_t rays_ended;        /* rays that passed their end cell */
  uint32_t origin_label;     /* the field's value at c_O; TLOAM_FRONTIER_OUTSIDE outside the box or for an invalid origin */
  uint32_t reserved0;        /* 0 */
  int64_t reserved1;         /* 0 */
} tloam_closed_map_view_record;
typedef struct tloam_closed_map_view_info {   /* of the last call */
  int64_t views;
  int64_t rays;                /* per view */
  int64_t window_side;         /* S */
  int64_t window_bytes;        /* 4 * ceil(S^3 / 32) */
  int64_t chunks;              /* the global form's chunks of views; 1 in the LDS form */
  int64_t steps;               /* summed over the views, as the next two */
  int64_t unknown_visits;
  int64_t unknown_cells;
  int64_t beyond_window;       /* visited cells beyond their window: 0 */
  int32_t form;                /* DIAGNOSTIC: the form that ran, 1 or 2 */
  int32_t blocks_per_view;     /* DIAGNOSTIC */
  int32_t launches;            /* DIAGNOSTIC: kernel launches of the call */
  int32_t waits;               /* DIAGNOSTIC: waits of the host */
} tloam_closed_map_view_info;
/* The gain of V >= 1 views under R >= 1 shared ends: poses_colmajor [16 V], ends_aos [3 R], gain_out [V].  NULLs, a pose that
 * is not finite and rigid, R beyond 2^28 or V * R beyond int64: TLOAM_E_INVALID; so is a window the LDS form is asked for and
 * cannot take, and a single window above max_bytes in the global form.  The ends and the poses are uploaded; the LDS form is one
 * launch, the global form per chunk of views a memset of its windows and counters and two launches (rays, count); one wait. */
int tloam_closed_map_view_gain(tloam_ctx* ctx, const double* poses_colmajor, size_t n_views, const double* ends_aos, size_t n_rays,
                               tloam_closed_map_view_record* gain_out, tloam_closed_map_view_info* info_or_null);
/* One view: the centres o + (c + 0.5) * v of the distinct UNKNOWN cells it sees, ascending in window bit index, by
 * tloam_closed_map_read_box's capacity convention (*n_out: their number, always; more than capacity: TLOAM_E_INVALID and nothing
 * written; centres_aos_out NULL: the number alone); gain_out_or_null: the view's record.  What a viewer draws. */
int tloam_closed_map_view_cells(tloam_ctx* ctx, const double* pose_colmajor, const double* ends_aos, size_t n_rays, size_t capacity,
                                double* centres_aos_out, size_t* n_out, tloam_closed_map_view_record* gain_out_or_null);
/* The explorer's one call: per kept cluster tloam_closed_map_frontier_costs' cost and approach point, and the gain of the view
 * with the identity rotation at the approach point.  TLOAM_E_NOT_READY exactly where tloam_closed_map_frontier_costs has it.  A
 * cluster without an approach point has three NaN for one: every ray of its view is skipped and its origin_label is
 * TLOAM_FRONTIER_OUTSIDE.  The capacity convention of tloam_closed_map_frontier_clusters (all three outputs NULL: the number
 * alone).  Two waits. */
int tloam_closed_map_frontier_gains(tloam_ctx* ctx, const double* ends_aos, size_t n_rays, size_t capacity,
                                    tloam_closed_map_view_record* gain_out, uint32_t* cost_out, double* approach_aos_out_or_null,
                                    size_t* n_out);
/* All zero when there has been no call since the frontier field was last dropped. */
int tloam_closed_map_get_view_info(tloam_ctx* ctx, tloam_closed_map_view_info* info);

/* ---- the closed map's snapshot: a built closed map out of a context and into a fresh one (additive to ABI 8) ------
 * A memory blob; the library opens no files.  It holds, exactly, everything a context needs to answer every read of the closed
 * map and every localisation in it with the bytes of the context that saved: the place, loop, closed map, carve and surfel
 * configurations (every reserve_* / reserved field written as 0), the three infos (capacity_voxels written as 0), the keyframe
 * database (frame, stored pose, ring key, sector key, descriptor of all keyframes), the build's poses, the rows in id order
 * (key, N, Qx, Qy, Qz), the miss counts when carved, the thirteen sums when surfels exist, and with TLOAM_SNAPSHOT_CLOUDS the
 * keyframes' eight clouds.  NOT saved: normals and variances (a pure function of the sums: recomputed at load, the same bits),
 * the localiser's voxel records (rebuilt lazily as ever), table sizes and capacities, place loop records, verified constraints
 * and corrected graph poses (the mapping session's working state), the localise and relocalise configurations (the querying
 * session's business).  Nothing in the blob depends on capacity, table size or allocation history: two saves give the same
 * bytes, and a save from a loaded context gives the blob it was loaded from.
 * Format version 1, little-endian, every section 8-byte aligned: a 416-byte header (magic "TLCMSNP1", version, flags, the
 * blob's bytes, the header's checksum, the counts, the grid, and a table of nine (kind, offset, bytes, checksum) entries, one
 * per section kind in ascending order, an absent section with 0 bytes), then the sections end to end.  The checksum of m 64-bit
 * words w_i is sum_i mix64(w_i + 0x9E3779B97F4A7C15 * (i + 1)) mod 2^64, mix64 the splitmix64 finaliser; the header's own is
 * over the header with that field zero.  DESIGN.md 25 has the table.
 * A blob is untrusted input: tloam_closed_map_load checks all of it -- header, table, configurations, poses and counts on the
 * host, checksums, keys, row and sum ranges, descriptors and the rebuilt slot table on the device -- before anything in the
 * context changes; a refused load is TLOAM_E_INVALID, tloam_last_error names the section and the test, and the context is as it
 * was, byte for byte.  A load replaces the state tloam_place_configure empties (keyframes, loop constraints, corrected poses,
 * closed map) and the five configurations.  Loaded without clouds the map is DETACHED: tloam_closed_map_build, _carve and
 * _surfels return TLOAM_E_NOT_READY and leave it as it is, until tloam_closed_map_configure, tloam_place_configure,
 * tloam_loop_configure or tloam_odometry_reset empty it as they always do (a carve or surfel configure drops its section as
 * always, and a detached map cannot gather it again).  Loaded with clouds nothing is detached. */
#define TLOAM_SNAPSHOT_CLOUDS 1   /* also the keyframes' eight clouds: the loaded map can be re-built, re-carved, re-surfelled */
#define TLOAM_SNAPSHOT_FORMAT_VERSION 1
typedef struct tloam_closed_map_snapshot_info {
  int32_t format_version;
  int32_t flags;                 /* TLOAM_SNAPSHOT_* of the save */
  int64_t n_keyframes_database;  /* keyframes of the place database */
  int64_t n_keyframes_map;       /* K of the build */
  int64_t n_voxels;
  int64_t n_points;
  int32_t has_carve, has_surfels, has_clouds;
  int32_t n_rings, n_sectors;
  int32_t reserved0;
  int64_t cloud_points;          /* points of all stored clouds (0 without them) */
  double voxel;
  double origin[3];
  uint64_t bytes;                /* of the whole blob */
} tloam_closed_map_snapshot_info;
/* The size tloam_closed_map_save(flags) writes.  TLOAM_E_NOT_READY without a built closed map, TLOAM_E_INVALID for unknown flags. */
int tloam_closed_map_save_size(tloam_ctx* ctx, int flags, size_t* bytes);
/* Writes the blob.  *written: its size, also when capacity is too small (then nothing is written and TLOAM_E_INVALID is
 * returned).  Changes nothing in the context. */
int tloam_closed_map_save(tloam_ctx* ctx, int flags, void* buf, size_t capacity, size_t* written);
/* Host only, no context, no GPU: the header and the section table checked (magic, version, checksum, every section inside the
 * blob, aligned, in order, of the size the counts ask for), the counts reported.  TLOAM_E_INVALID otherwise. */
int tloam_closed_map_probe(const void* buf, size_t bytes, tloam_closed_map_snapshot_info* info);
int tloam_closed_map_load(tloam_ctx* ctx, const void* buf, size_t bytes, tloam_closed_map_snapshot_info* info_or_null);
/* Every snapshot call with a context on one with nranks > 1: TLOAM_E_INVALID. */

/* ---- multi-GPU: correspondence set sharded over ranks, one all-reduce per sweep --------
 * (nothing in the reference).  Call before set_source / set_correspondences.
 * (a) native RCCL over xGMI: unique_id = the 128 bytes of an ncclUniqueId made on rank 0
 *     by tloam_rccl_unique_id and broadcast by the launcher. */
int tloam_rccl_unique_id(void* out128);
int tloam_comm_init_rccl(tloam_ctx* ctx, int rank, int nranks, const void* unique_id128);
/* nranks == 1 in (a) and (c): the context exchanges with itself -- every launch of the sharded forms runs (fused sweep + post,
 * gather + step, the side exchanges of the caps and the cost sums), the all-reduce / the mailbox is a loop-back, and the results
 * are those of the single-rank forms bit for bit.  It is how the sharded forms are timed at shard size on ONE GPU and how a
 * one-rank RCCL communicator gets to carry the all-reduce. */
/* (b) caller-provided sum all-reduce on a DEVICE buffer of `count` doubles, enqueued on (or
 *     synchronised with) `hip_stream`; returns 0 on success.  Used by the gloo-backed tests
 *     and by hosts that already own a communicator. */
typedef int (*tloam_allreduce_fn)(void* user, double* device_buf, int count, void* hip_stream);
int tloam_comm_init_callback(tloam_ctx* ctx, int rank, int nranks, tloam_allreduce_fn fn,
                             void* user);
/* (c) one-shot peer exchange ("mailbox") over xGMI, no collective library on the data path.  Every rank calls
 *     tloam_comm_mailbox_export (64 bytes = a hipIpcMemHandle_t of its small fine-grained buffer), the launcher
 *     all-gathers the handles (rank order), every rank calls tloam_comm_init_mailbox with all of them.  A sharded
 *     GN iteration is then TWO launches: the sweep, whose last block stores the 48 doubles into every rank's
 *     buffer, and the step, which adds the ranks' rows in rank order (bit-identical on all ranks).  A peer that
 *     never posts makes the waiting kernel give up after ~2 s: TLOAM_E_RCCL from the scan_match in progress.
 *     One process per rank (HIP IPC does not open a handle in the process that made it). */
int tloam_comm_mailbox_export(tloam_ctx* ctx, void* handle64_out);
int tloam_comm_init_mailbox(tloam_ctx* ctx, int rank, int nranks, const void* handles64_by_rank);
/* contiguous index block [*lo,*hi) of n items owned by `rank` of `nranks` (pure function) */
void tloam_shard_range(size_t n, int rank, int nranks, size_t* lo, size_t* hi);
/* The blocks of a whole Frame (what tloam_set_source_frame keeps in a sharded context): the four clouds laid end to end, the
 * line cut into nranks equal pieces.  Per kind still contiguous index blocks in rank order; every rank the same number of
 * source points; a rank touches one or two kinds and builds only those kinds' search grids. */
void tloam_shard_ranges_frame(const size_t n[4], int rank, int nranks, size_t lo[4], size_t hi[4]);

/* ---- SE(3) helpers (host; the ~150 lines of vendored Sophus the path uses) -------------
 * se3.hpp:761-785 (exp), :223-256 (log), :497-504 (from matrix), registration.cpp:162-173 */
int tloam_se3_exp(const double se3[6], double T_colmajor[16]);
int tloam_se3_log(const double T_colmajor[16], double se3[6]);
int tloam_se3_plus(const double x[6], const double delta[6], double x_plus_delta[6]);

#ifdef __cplusplus
}
#endif
#endif /* TLOAM_HIP_H */
