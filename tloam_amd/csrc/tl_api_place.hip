// tl_api_place.hip -- C ABI of place recognition (include/tloam_hip.h: tloam_place_*), driven from tl_api_odom.hip
// (kernels in tl_place.hip).
//
// A frame with place recognition on: the keyframe database is grown at the start of the frame, before anything of the odometry
// state changes (place_frame_reserve).  When the frame has ended -- its last wait done, the stream drained -- an accepted frame
// whose returned pose passes the keyframe policy is described from the scan it used, committed into the database and searched
// against the earlier keyframes, by launches nothing waits for (place_frame_end).  The scan buffer is intact at that point in
// stream order: the next frame's upload queues behind these launches.  Only a regrowth of that buffer (a larger scan) would free
// it under them, and the next frame's reserve waits for them first.  The loop records' count stays on the device; the calls
// that read it wait.
#include <float.h>
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

constexpr size_t kPlaceDefaultReserve = 1024;     // keyframes (9.6 MiB of descriptors at 20 x 60): reserve_keyframes = 0
constexpr size_t kPlaceMaxKeyframes = (size_t)1 << 30;   // ids are 32-bit on the device

bool pos_finite(double v) { return v > 0.0 && v <= DBL_MAX; }

bool place_config_ok(const tloam_place_config& p, bool check_enabled) {
  return (!check_enabled || p.enabled == 0 || p.enabled == 1) && p.n_rings >= 1 && p.n_rings <= kPlaceMaxRings &&
         p.n_sectors >= 2 && p.n_sectors <= kPlaceMaxSectors && p.num_candidates >= 1 &&
         p.num_candidates <= kPlaceMaxCandidates && p.exclude_recent >= 1 && pos_finite(p.max_radius) &&
         std::isfinite(p.height_offset) && pos_finite(p.kf_dist) && pos_finite(p.kf_angle) && pos_finite(p.dist_thres) &&
         p.reserve_keyframes >= 0;
}

// the keyframe policy: B has moved >= kf_dist or turned >= kf_angle from A (column-major; the trace summed column by column,
// row by row -- tests/place_np.py `moved`)
bool moved(const double A[16], const double B[16], double kf_dist, double kf_angle) {
  const double dx = B[12] - A[12], dy = B[13] - A[13], dz = B[14] - A[14];
  const double dist = sqrt(dx * dx + dy * dy + dz * dz);
  double tr = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) tr = tr + A[4 * i + k] * B[4 * i + k];
  const double cs = std::min(1.0, std::max(-1.0, (tr - 1.0) * 0.5));
  return dist >= kf_dist || acos(cs) >= kf_angle;
}

// the database holds `need` keyframes: new storage of max(need, 2 cap), the keyframes so far copied device to device behind
// whatever is in flight, the old storage retired until the stream has drained.  A failure leaves the database as it was
int place_grow(tloam_ctx* c, size_t need) {
  PlaceState& P = c->place;
  if (need <= P.cap) return TLOAM_OK;
  if (!P.retired.empty()) {   // (a regrowth whose frame has not ended: not on the frame's path)
    HIPC(c, hipStreamSynchronize(c->stream));
    P.retired.release();
  }
  const size_t want = std::max(need, 2 * P.cap);
  if (want > kPlaceMaxKeyframes) {
    c->last_error = "place recognition: more than 2^30 keyframes";
    return TLOAM_E_HIP;
  }
  const size_t R = (size_t)P.cfg.n_rings, S = (size_t)P.cfg.n_sectors, keep = (size_t)P.n_kf;
  Grower g(c, P.retired);
  g.add(P.desc, want * R * S, keep * R * S);
  g.add(P.rkey, want * R, keep * R);
  g.add(P.skey, want * S, keep * S);
  g.add(P.pose, want * 16, keep * 16);
  g.add(P.frame, want, keep);
  g.add(P.loops, want, keep);   // (at most one loop per keyframe)
  g.add(P.kdist, want);
  g.add(P.taken, want);
  const int rc = g.commit("place recognition database growth: ");
  if (rc != TLOAM_OK) return rc;
  P.cap = want;
  return TLOAM_OK;
}

// keyframe q = n_kf (the database has room): described from `scan`, committed with its pose and frame number, searched.
// Enqueued only
void enqueue_keyframe(tloam_ctx* c, const double* scan, size_t n, const double pose[16], int64_t frame) {
  PlaceState& P = c->place;
  const tloam_place_config& g = P.cfg;
  const size_t R = (size_t)g.n_rings, S = (size_t)g.n_sectors, q = (size_t)P.n_kf;
  PlaceDescArgs D;
  memset(&D, 0, sizeof(D));
  D.aos = scan; D.n = (long long)n;
  D.bins = P.bins.p;
  D.desc = P.desc.p + q * R * S; D.ring_key = P.rkey.p + q * R; D.sector_key = P.skey.p + q * S;
  D.frame_out = P.frame.p + q; D.pose_out = P.pose.p + 16 * q;
  D.frame = frame;
  memcpy(D.pose, pose, sizeof(D.pose));
  D.R = g.n_rings; D.S = g.n_sectors;
  D.max_radius = g.max_radius; D.height_offset = g.height_offset;
  launch_place_describe(D, c->stream);
  PlaceState::Keyframe K;
  memset(&K, 0, sizeof(K));
  K.frame = frame;
  memcpy(K.pose, pose, sizeof(K.pose));
  P.kf.push_back(K);
  const long long m = (long long)q - g.exclude_recent + 1;   // keyframes 0 .. q - exclude_recent
  if (m > 0) {
    PlaceSearchArgs A;
    memset(&A, 0, sizeof(A));
    A.desc = P.desc.p; A.ring_key = P.rkey.p; A.frames = P.frame.p;
    A.kdist = P.kdist.p; A.taken = P.taken.p; A.cand = P.cand.p;
    A.loops = P.loops.p; A.n_loops = P.ctl.p;
    A.q = (int)q; A.m = (int)m; A.ncand = (int)std::min<long long>(g.num_candidates, m);
    A.R = g.n_rings; A.S = g.n_sectors;
    A.dist_thres = g.dist_thres;
    launch_place_search(A, c->stream);
  }
  P.n_kf++;
  P.last_kf_frame = frame;
  memcpy(P.last_pose, pose, sizeof(P.last_pose));
}

// the database and its scratch for `cfg` (place recognition just enabled): empty, `reserve` keyframes of room
int place_alloc(tloam_ctx* c, size_t reserve) {
  PlaceState& P = c->place;
  const size_t RS = (size_t)P.cfg.n_rings * P.cfg.n_sectors;
  HIPC(c, P.bins.reserve(RS));
  HIPC(c, hipMemsetAsync(P.bins.p, 0, sizeof(unsigned long long) * P.bins.cap, c->stream));
  HIPC(c, P.ctl.reserve(1));
  HIPC(c, hipMemsetAsync(P.ctl.p, 0, sizeof(unsigned long long), c->stream));
  HIPC(c, P.cand.reserve(kPlaceMaxCandidates));
  const int rc = place_grow(c, reserve);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, hipStreamSynchronize(c->stream));
  P.retired.release();
  return TLOAM_OK;
}

int64_t device_loops(tloam_ctx* c, int* rc) {   // waits for the work in flight
  *rc = TLOAM_OK;
  PlaceState& P = c->place;
  if (!P.ctl.p) return 0;
  unsigned long long n = 0;
  hipError_t e = hipMemcpyAsync(&n, P.ctl.p, sizeof(n), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    c->last_error = std::string("place recognition: reading the loop count: ") + hipGetErrorString(e);
    *rc = TLOAM_E_HIP;
    return 0;
  }
  return (int64_t)n;
}

}  // namespace

namespace tlh {

bool place_config_valid(const tloam_place_config& cfg) { return place_config_ok(cfg, true); }
size_t place_default_reserve() { return kPlaceDefaultReserve; }

// the start of a frame: room for one more keyframe, before anything of the odometry state changes.  A failure leaves the frame
// undone
int place_frame_reserve(tloam_ctx* c, size_t n) {
  PlaceState& P = c->place;
  P.pend.nspan = 0;
  if (!P.cfg.enabled) return TLOAM_OK;
  if (P.in_flight && (c->seg.aos.cap < 3 * n || (c->deskew.cfg.enabled && c->deskew.aos.cap < 3 * n)))
    HIPC(c, hipStreamSynchronize(c->stream));   // (the last keyframe's launches read the scan buffer this frame regrows)
  P.in_flight = false;
  return place_grow(c, (size_t)P.n_kf + 1);
}

// the frame has ended (the stream has drained): storage a regrowth replaced is freed; an accepted frame that is a keyframe is
// described, committed and searched by launches nothing waits for
void place_frame_end(tloam_ctx* c, bool accepted, int64_t frame, const double pose[16], const double* scan, size_t n) {
  PlaceState& P = c->place;
  P.retired.release();
  P.in_flight = false;
  if (!accepted || !P.cfg.enabled || P.cap < (size_t)P.n_kf + 1) return;
  if (P.n_kf > 0 && !moved(P.last_pose, pose, P.cfg.kf_dist, P.cfg.kf_angle)) return;
  enqueue_keyframe(c, scan, n, pose, frame);
  P.in_flight = true;
  if (P.pend.nspan != 8) return;
  // loop verification on: the frame's eight clouds into the arena (room was made at the frame's reserve), ONE launch behind the
  // place launches, reading buffers the next frame rewrites only after its first wait
  PlaceState::Keyframe& K = P.kf.back();
  for (int j = 0; j < 8; ++j) {
    K.off[j] = P.arena_used + 3 * (size_t)P.pend.start[j];
    K.n[j] = (size_t)(P.pend.start[j + 1] - P.pend.start[j]);
    P.pend.s[j].dst = P.arena.p + K.off[j];
  }
  launch_place_clouds(P.pend, c->stream);
  P.arena_used += 3 * (size_t)P.pend.start[8];
  P.pend.nspan = 0;
}

bool place_clouds_on(const tloam_ctx* c) { return c->place.cfg.enabled && c->loop.cfg.enabled; }

// the arena holds arena_used + need doubles: new storage of max(that, 2 cap), the clouds so far copied device to device behind
// whatever is in flight, the old storage retired until the stream has drained.  A failure leaves the arena as it was
int arena_grow(tloam_ctx* c, size_t need) {
  PlaceState& P = c->place;
  if (P.arena_used + need <= P.arena.cap) return TLOAM_OK;
  const int64_t rp = c->loop.cfg.reserve_points;
  const size_t first = 3 * (rp > 0 ? (size_t)rp : ((size_t)1 << 20));
  const size_t want = std::max(P.arena_used + need, P.arena.cap ? 2 * P.arena.cap : first);
  Grower g(c, P.retired);
  g.add(P.arena, want, P.arena_used);
  return g.commit("keyframe cloud arena growth: ");
}

// after the frame's wait 3 (the sizes are on the host, nothing waits): room for the frame's eight clouds, should it be a keyframe
int place_clouds_reserve(tloam_ctx* c, const size_t n[8]) {
  if (!place_clouds_on(c)) return TLOAM_OK;
  size_t all = 0;
  for (int j = 0; j < 8; ++j) all += 3 * n[j];
  return arena_grow(c, all);
}

// the frame's eight spans (dst filled in at the commit); rows counted from the first span's
void place_clouds_note(tloam_ctx* c, const LoopSpan spans[8]) {
  if (!place_clouds_on(c)) return;
  LoopSpanArgs& A = c->place.pend;
  A.start[0] = 0;
  for (int j = 0; j < 8; ++j) {
    A.s[j] = spans[j];
    A.s[j].rigid = 0;
    A.start[j + 1] = A.start[j] + spans[j].n;
  }
  A.nspan = 8;
}

}  // namespace tlh

extern "C" {

void tloam_place_default_config(tloam_place_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->n_rings = 20;
  cfg->n_sectors = 60;
  cfg->num_candidates = 10;
  cfg->exclude_recent = 50;
  cfg->max_radius = 80.0;   // inside synth_hdl64's enclosing wall (90 m): DESIGN.md 16
  cfg->height_offset = 2.0;
  cfg->kf_dist = 1.0;
  cfg->kf_angle = 0.2;
  cfg->dist_thres = 0.30;   // measured: DESIGN.md 16
  cfg->reserve_keyframes = 0;
}

int tloam_place_configure(tloam_ctx* c, const tloam_place_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_place_config want = cfg_or_default(cfg, tloam_place_default_config);
  if (!place_config_ok(want, true)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  PlaceState& P = c->place;
  P = PlaceState();   // (empty: a new layout, or off -- the frame's memory is then what it was without place recognition)
  c->loop.clear();   // (the constraints name keyframes that are gone)
  c->graph.drop();   // (so do the corrected poses)
  c->cmap.drop();    // (and the closed map was built from them)
  P.cfg = want;
  if (!want.enabled) return TLOAM_OK;
  const int rc = place_alloc(c, want.reserve_keyframes > 0 ? (size_t)want.reserve_keyframes : kPlaceDefaultReserve);
  if (rc != TLOAM_OK) {
    P = PlaceState();
    P.cfg = want;
    P.cfg.enabled = 0;
    return rc;
  }
  return TLOAM_OK;
}

int tloam_place_get_info(tloam_ctx* c, tloam_place_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  const PlaceState& P = c->place;
  memset(info, 0, sizeof(*info));
  HIPC(c, hipSetDevice(c->device));
  int rc;
  info->n_loops = device_loops(c, &rc);
  if (rc != TLOAM_OK) return rc;
  info->n_keyframes = P.n_kf;
  info->last_keyframe_frame = P.last_kf_frame;
  info->capacity_keyframes = (int64_t)P.cap;
  return TLOAM_OK;
}

int tloam_place_read_keyframes(tloam_ctx* c, size_t first, size_t count, int64_t* frames, double* poses_colmajor,
                               double* ring_keys, double* sector_keys, double* descriptors) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  PlaceState& P = c->place;
  const size_t nk = (size_t)P.n_kf;
  if (first > nk || count > nk - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  const size_t R = (size_t)P.cfg.n_rings, S = (size_t)P.cfg.n_sectors;
  HIPC(c, hipSetDevice(c->device));
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  if (frames) HIPC(c, hipMemcpyAsync(frames, P.frame.p + first, sizeof(int64_t) * count, D2H, c->stream));
  if (poses_colmajor) HIPC(c, hipMemcpyAsync(poses_colmajor, P.pose.p + 16 * first, sizeof(double) * 16 * count, D2H, c->stream));
  if (ring_keys) HIPC(c, hipMemcpyAsync(ring_keys, P.rkey.p + R * first, sizeof(double) * R * count, D2H, c->stream));
  if (sector_keys) HIPC(c, hipMemcpyAsync(sector_keys, P.skey.p + S * first, sizeof(double) * S * count, D2H, c->stream));
  if (descriptors)
    HIPC(c, hipMemcpyAsync(descriptors, P.desc.p + R * S * first, sizeof(double) * R * S * count, D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_place_read_loops(tloam_ctx* c, size_t first, size_t count, tloam_place_loop* loops) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  int rc;
  const size_t nl = (size_t)device_loops(c, &rc);
  if (rc != TLOAM_OK) return rc;
  if (first > nl || count > nl - first) return TLOAM_E_INVALID;
  if (count == 0 || !loops) return TLOAM_OK;
  HIPC(c, hipMemcpyAsync(loops, c->place.loops.p + first, sizeof(tloam_place_loop) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_place_add_scan(tloam_ctx* c, const double* xyz, size_t n, const double pose[16], int64_t frame_id,
                         int64_t* keyframe_out) {
  if (!c || !pose || c->nranks > 1 || (n > 0 && !xyz) || n > kMaxPoints || n > (size_t)INT32_MAX / 3) return TLOAM_E_INVALID;
  PlaceState& P = c->place;
  if (!P.cfg.enabled) return TLOAM_E_INVALID;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(pose[i])) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (not a frame: whatever is in flight may read the buffers replaced below)
  P.retired.release();
  P.in_flight = false;
  int rc = place_grow(c, (size_t)P.n_kf + 1);
  if (rc != TLOAM_OK) return rc;
  if (n > 0) {
    HIPC(c, P.s_aos.reserve(3 * n));
    HIPC(c, hipMemcpyAsync(P.s_aos.p, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  }
  const int64_t q = P.n_kf;
  enqueue_keyframe(c, P.s_aos.p, n, pose, frame_id);
  HIPC(c, hipStreamSynchronize(c->stream));
  P.retired.release();
  if (keyframe_out) *keyframe_out = q;
  return TLOAM_OK;
}

int tloam_place_describe(tloam_ctx* c, const tloam_place_config* cfg, const double* xyz, size_t n, double* descriptor,
                         double* ring_key, double* sector_key) {
  if (!c || c->nranks > 1 || (n > 0 && !xyz) || n > kMaxPoints || n > (size_t)INT32_MAX / 3) return TLOAM_E_INVALID;
  PlaceState& P = c->place;
  const tloam_place_config g = cfg ? *cfg : P.cfg;
  if (!place_config_ok(g, false)) return TLOAM_E_INVALID;
  const size_t R = (size_t)g.n_rings, S = (size_t)g.n_sectors;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (the bins and the upload buffer may be replaced)
  P.in_flight = false;
  const size_t had = P.bins.cap;
  HIPC(c, P.bins.reserve(R * S));
  if (P.bins.cap != had) HIPC(c, hipMemsetAsync(P.bins.p, 0, sizeof(unsigned long long) * P.bins.cap, c->stream));
  HIPC(c, P.s_desc.reserve(R * S)); HIPC(c, P.s_rkey.reserve(R)); HIPC(c, P.s_skey.reserve(S));
  if (n > 0) {
    HIPC(c, P.s_aos.reserve(3 * n));
    HIPC(c, hipMemcpyAsync(P.s_aos.p, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  }
  PlaceDescArgs D;
  memset(&D, 0, sizeof(D));
  D.aos = P.s_aos.p; D.n = (long long)n;
  D.bins = P.bins.p; D.desc = P.s_desc.p; D.ring_key = P.s_rkey.p; D.sector_key = P.s_skey.p;
  D.R = g.n_rings; D.S = g.n_sectors;
  D.max_radius = g.max_radius; D.height_offset = g.height_offset;
  launch_place_describe(D, c->stream);
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  if (descriptor) HIPC(c, hipMemcpyAsync(descriptor, P.s_desc.p, sizeof(double) * R * S, D2H, c->stream));
  if (ring_key) HIPC(c, hipMemcpyAsync(ring_key, P.s_rkey.p, sizeof(double) * R, D2H, c->stream));
  if (sector_key) HIPC(c, hipMemcpyAsync(sector_key, P.s_skey.p, sizeof(double) * S, D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

}  // extern "C"
