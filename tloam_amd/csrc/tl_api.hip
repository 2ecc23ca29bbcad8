// tl_api.hip -- lifetime of the C ABI's context (include/tloam_hip.h): create / destroy, configuration, status strings,
// the sharding rules, the host SE(3) helpers.  The other units: tl_api_frames.hip (HBM residency, search grids),
// tl_api_match.hip (the scanMatching driver), tl_api_sets.hip (its factor set outside a frame: getters, solve, timing helpers),
// tl_api_comm.hip (multi-GPU exchange), tl_api_submap.hip, tl_api_feature.hip.
//
// There is no CPU fallback: without a usable device every computing entry point returns TLOAM_E_HIP.
#include "tl_ctx.hpp"

using namespace tl;

extern "C" {

int tloam_abi_version(void) { return TLOAM_ABI_VERSION; }

const char* tloam_status_string(int s) {
  switch (s) {
    case TLOAM_OK: return "ok";
    case TLOAM_E_INVALID: return "invalid argument";
    case TLOAM_E_TOO_FEW_POINTS: return "fewer than 10 points in a feature cloud";
    case TLOAM_E_BAD_POSE: return "predicted pose is not a rigid transform";
    case TLOAM_E_HIP: return "HIP error / no gfx950 device";
    case TLOAM_E_RCCL: return "RCCL error";
    case TLOAM_E_NOT_READY: return "call sequence violated";
    case TLOAM_E_WEIGHT_RANGE: return "GNC weight outside [0,1]";
    default: return "unknown status";
  }
}

void tloam_default_config(tloam_tls_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));  // config/mapping/lidar_odometry.yaml:23-39
  c->k_corr = 10;
  c->factor_num = 4;
  c->edge_dist_thres = 1.0;
  c->edge_dir_thres = 0.85;
  c->edge_maxnum = 1200;
  c->sphere_dist_thres = 0.5;
  c->sphere_maxnum = 200;
  c->planar_dist_thres = 0.5;
  c->planar_maxnum = 2500;
  c->ground_dist_thres = 0.5;
  c->ground_maxnum = 2000;
  c->max_iterations = 4;
  c->cost_threshold = 5e-9;
  c->gnc_factor = 11.8;
  c->noise_bound = 0.01;
  c->fitness_thres = 0.02;
}

int tloam_create(const tloam_tls_config* cfg, int device_id, tloam_ctx** out) {
  if (!cfg || !out) return TLOAM_E_INVALID;
  *out = nullptr;
  // kernel arguments in device memory (a frame is a chain of short dependent launches); only effective if this is
  // the process's first HIP call, never overrides the host's own setting
  (void)setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return TLOAM_E_HIP;
  if (hipSetDevice(device_id) != hipSuccess) return TLOAM_E_HIP;
  tloam_ctx* c = new (std::nothrow) tloam_ctx();
  if (!c) return TLOAM_E_INVALID;
  c->cfg = *cfg;
  c->device = device_id;
  if (const char* e = getenv("TLOAM_DEBUG_MAX_SWEEPS")) c->dbg_max_sweeps = atoi(e);
  c->dbg_no_build_reuse = getenv("TLOAM_NO_BUILD_REUSE") != nullptr;
  c->dbg_no_eval_reuse = getenv("TLOAM_NO_EVAL_REUSE") != nullptr;
  c->no_device_loop = getenv("TLOAM_NO_DEVICE_LOOP") != nullptr;
  c->no_persistent_solve = getenv("TLOAM_NO_PERSISTENT_SOLVE") != nullptr;
  c->no_grid_ahead = getenv("TLOAM_NO_GRID_AHEAD") != nullptr;
  c->no_direct_set = getenv("TLOAM_NO_DIRECT_SET") != nullptr;
  c->no_qbin_ride = getenv("TLOAM_NO_QBIN_RIDE") != nullptr;
  if (const char* e = getenv("TLOAM_DEBUG_FAIL_HANDOVER")) c->dbg_fail_handover = atoi(e);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess) cus = 0;
    c->device_cus = cus;
  }
  c->fused_large = getenv("TLOAM_FUSED_LARGE") != nullptr;
  if (const char* e = getenv("TLOAM_PLANNED_SWEEPS")) c->dbg_planned_sweeps = atoi(e);
  memset(&c->stats, 0, sizeof(c->stats));
  // pinned host memory: the state's mirror and a small scratch; and, device-visible, what the kernels write their results into
  // (result slots, bounding-box rows, fault words): required -- there is no copy + synchronise variant of the paths that use them
  constexpr size_t kBoxDoubles = (size_t)kKinds * 64 * 6 + 8;
  const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent;
  const bool up = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
                  c->h_state.alloc(kMirrorSlots, flags) == hipSuccess && c->h_small.alloc(4096, hipHostMallocDefault) == hipSuccess &&
                  c->h_mirror.alloc(kMirrorSlots, flags) == hipSuccess && ((uintptr_t)c->h_mirror.h & 63u) == 0 &&
                  c->h_mirror.map() == hipSuccess && c->h_bbox.alloc(kBoxDoubles, flags) == hipSuccess &&
                  c->h_bbox.map() == hipSuccess && c->h_fault.alloc(kFaultWords, flags) == hipSuccess &&
                  c->h_fault.map() == hipSuccess;
  if (up) {
    c->h_state.zero();
    c->h_mirror.zero();
    c->h_bbox.zero();
    c->h_fault.zero();
  }
  if (!up || ensure_common(c) != TLOAM_OK) {
    (void)hipGetLastError();
    tloam_destroy(c);
    return TLOAM_E_HIP;
  }
  (void)hipMemsetAsync(c->state.p, 0, sizeof(GnState), c->stream);
  (void)hipMemsetAsync(c->seg_n.p, 0, 8 * sizeof(int), c->stream);
  (void)hipStreamSynchronize(c->stream);
  *out = c;
  return TLOAM_OK;
}

// Every device and pinned buffer is freed by the struct that declares it when the context is deleted (tl_ctx.hpp); what is left to
// do by hand is what was made through other calls: the exchange's handles, the child contexts, the events and the stream.  (A frame
// slot still selected needs nothing: its clouds are in kd[], the context's own in the slot, each owned once.)
void tloam_destroy(tloam_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  tlh::comm_release(c);
  tlh::loop_release(c);
  for (auto& e : c->ev_pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->stage_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* tloam_last_error(const tloam_ctx* c) { return c ? c->last_error.c_str() : ""; }

void tloam_shard_range(size_t n, int rank, int nranks, size_t* lo, size_t* hi) {
  if (nranks < 1) nranks = 1;
  if (rank < 0) rank = 0;
  if (rank >= nranks) rank = nranks - 1;
  // contiguous index blocks keep the reference's "first N valid in index order" cap semantics
  const size_t a = (size_t)(((unsigned __int128)n * (unsigned)rank) / (unsigned)nranks);
  const size_t b = (size_t)(((unsigned __int128)n * (unsigned)(rank + 1)) / (unsigned)nranks);
  if (lo) *lo = a;
  if (hi) *hi = b;
}

// A whole Frame over the ranks: the four source clouds laid end to end (planar | ground | edge | sphere), the line cut into
// nranks equal pieces, every rank the intersection of its piece with each cloud.  Per kind that is still contiguous index
// blocks in rank order (so the cap prefix over the lower ranks' counts, registration.cpp:448/:538/:592/:735, holds as it
// is), every rank gets the same number of queries whatever the mix, and a rank touches one or two kinds instead of four:
// it builds only THOSE kinds' search grids (tloam_sm_begin) -- the target-grid build is what a sharded frame replicates.
void tloam_shard_ranges_frame(const size_t n[4], int rank, int nranks, size_t lo[4], size_t hi[4]) {
  if (nranks < 1) nranks = 1;
  if (rank < 0) rank = 0;
  if (rank >= nranks) rank = nranks - 1;
  unsigned __int128 total = 0;
  for (int k = 0; k < kKinds; ++k) total += n[k];
  const size_t a = (size_t)((total * (unsigned)rank) / (unsigned)nranks), b = (size_t)((total * (unsigned)(rank + 1)) / (unsigned)nranks);
  size_t base = 0;
  for (int k = 0; k < kKinds; ++k) {
    const size_t l = std::min(std::max(a, base), base + n[k]), h = std::min(std::max(b, base), base + n[k]);
    lo[k] = l - base;
    hi[k] = h - base;
    base += n[k];
  }
}

int tloam_get_info(tloam_ctx* c, tloam_ctx_info* out) {
  if (!c || !out) return TLOAM_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->abi_version = TLOAM_ABI_VERSION;
  out->device = c->device;
  out->device_cus = c->device_cus;
  out->comm_mode = (int32_t)c->comm;
  out->rank = c->rank;
  out->nranks = c->nranks;
  out->loopback = c->loopback ? 1 : 0;
  out->direct_set = (c->forms.set == SetForm::DIRECT && !c->prebuilt) ? 1 : 0;
  out->set_stale = c->set_stale ? 1 : 0;
  tlh::comm_rccl_info(c, &out->rccl_comm_count, &out->rccl_comm_rank);
  out->fallbacks_taken = (c->no_scan_1p ? TLOAM_FALLBACK_SCAN : 0) | (c->vox_ticket ? TLOAM_FALLBACK_VOXEL : 0) |
                         (c->persistent_solve_timed_out ? TLOAM_FALLBACK_SOLVE : 0);
  out->fallback_events = c->fallback_events;
  out->k3_grid = c->k3_grid;
  out->k3_single = c->k3_single ? 1 : 0;
  out->k3_wide = c->k3_wide ? 1 : 0;
  out->one_launch_solve = c->forms.solve == SolveForm::PERSISTENT ? 1 : 0;
  return TLOAM_OK;
}

int tloam_get_grid_info(tloam_ctx* c, tloam_grid_info* out) {
  if (!c || !out) return TLOAM_E_INVALID;
  *out = c->grid_info;
  return TLOAM_OK;
}

int tloam_debug_raise_fault(tloam_ctx* c, int which) {
  if (!c || which < 0 || which >= kFaultWords || !c->h_fault) return TLOAM_E_INVALID;
  __atomic_store_n(&c->h_fault[which], 1u, __ATOMIC_RELEASE);
  return TLOAM_OK;
}

// ---- SE(3) helpers (host) ------------------------------------------------------------------------------
int tloam_se3_exp(const double se3[6], double T[16]) {
  if (!se3 || !T) return TLOAM_E_INVALID;
  pose_to_matrix(se3_exp(se3), T);
  return TLOAM_OK;
}
int tloam_se3_log(const double T[16], double se3[6]) {
  if (!se3 || !T) return TLOAM_E_INVALID;
  Pose P;
  if (!pose_from_matrix(T, &P)) return TLOAM_E_BAD_POSE;
  se3_log(P, se3);
  return TLOAM_OK;
}
int tloam_se3_plus(const double x[6], const double delta[6], double out[6]) {
  if (!x || !delta || !out) return TLOAM_E_INVALID;
  se3_plus(x, delta, out);
  return TLOAM_OK;
}

}  // extern "C"
