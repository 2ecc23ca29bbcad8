// tl_api_deskew.hip -- C ABI of the odometry frame's deskew (include/tloam_hip.h: tloam_deskew_*), driven from tl_api_odom.hip
// (the kernel is in tl_deskew.hip).
//
// A frame with deskew on: its times (timed mode) follow the scan's upload (deskew_frame_upload); after the segmentation's launches
// the correction runs into a grow-only copy of the scan, which every later stage of the frame reads instead of the segmentation's
// input (deskew_frame_launch, frame_scan); the refused-time flag is read together with the segmentation's control block, at the
// frame's first wait.  xi = log(step) is formed here, once per frame, and handed to the kernel as arguments.  A frame whose step
// is bitwise the identity runs no correction (in timed mode its times are still checked, by the same kernel writing nothing else).
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

constexpr double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

bool deskew_config_ok(const tloam_deskew_config& d) {
  return (d.enabled == 0 || d.enabled == 1) && (d.time_source == 0 || d.time_source == 1) &&
         (d.direction == 1 || d.direction == -1) && std::isfinite(d.start_azimuth) && std::isfinite(d.ref_fraction);
}

bool is_identity(const double M[16]) { return memcmp(M, kIdentity, sizeof(kIdentity)) == 0; }

// xi = log(motion); false when the motion is not a rigid transform (tl_se3.hpp pose_from_matrix)
bool motion_log(const double M[16], double xi[6]) {
  Pose P;
  if (!pose_from_matrix(M, &P)) return false;
  se3_log(P, xi);
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(xi[k])) return false;
  return true;
}

DeskewArgs args_of(const tloam_deskew_config& d, double period, const double xi[6]) {
  DeskewArgs A;
  memset(&A, 0, sizeof(A));
  for (int k = 0; k < 6; ++k) A.xi[k] = xi[k];
  A.period = period;
  A.direction = (double)d.direction;
  A.start = d.start_azimuth;
  A.ref = d.ref_fraction;
  return A;
}

}  // namespace

namespace tlh {

// after the scan's upload (segment_begin has counted the upload): the frame's buffers sized, its times uploaded
int deskew_frame_upload(tloam_ctx* c, const double* t_sec, size_t n, tloam_odom_stats* st) {
  DeskewState& D = c->deskew;
  D.active = false;
  D.timed = false;
  if (!D.cfg.enabled) return TLOAM_OK;
  HIPC(c, D.ctl.reserve(3));
  D.timed = D.cfg.time_source == 1;
  if (D.timed) {
    HIPC(c, D.t.reserve(n));
    HIPC(c, hipMemcpyAsync(D.t.p, t_sec, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    st->h2d_bytes += (int64_t)(sizeof(double) * n);
  }
  const OdomState& O = c->odom;
  if (!is_identity(O.step) && motion_log(O.step, D.xi)) {
    HIPC(c, D.aos.reserve(3 * n));
    D.active = true;
  }
  return TLOAM_OK;
}

// after the segmentation's launches, before the frame's first wait: the correction (or, timed with no motion, the check of the
// times), and the enqueued read of the refused-time flag into *bad_host (timed mode; 0 otherwise)
int deskew_frame_launch(tloam_ctx* c, size_t n, unsigned long long* bad_host, tloam_odom_stats* st) {
  DeskewState& D = c->deskew;
  *bad_host = 0;
  if (!D.active && !D.timed) return TLOAM_OK;
  const double zero_xi[6] = {0, 0, 0, 0, 0, 0};
  DeskewArgs A = args_of(D.cfg, c->odom.cfg.seg.scan_period, D.active ? D.xi : zero_xi);
  A.in = c->seg.aos.p;
  A.n = (long long)n;
  if (D.active) {
    A.out = D.aos.p;
    A.max_shift = D.ctl.p + D.slot;
    HIPC(c, hipMemsetAsync(A.max_shift, 0, sizeof(unsigned long long), c->stream));
  }
  if (D.timed) {
    A.t = D.t.p;
    A.bad = D.ctl.p + 2;
    HIPC(c, hipMemsetAsync(A.bad, 0, sizeof(unsigned long long), c->stream));
  }
  launch_deskew(A, c->stream);
  if (D.timed) {
    HIPC(c, hipMemcpyAsync(bad_host, A.bad, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    st->d2h_bytes += (int64_t)sizeof(unsigned long long);
  }
  return TLOAM_OK;
}

// the frame has drained the stream: an accepted deskewed frame becomes the info's last one
void deskew_frame_end(tloam_ctx* c, bool accepted, int64_t frame) {
  DeskewState& D = c->deskew;
  if (accepted && D.active) {
    D.frames++;
    D.last_frame = frame;
    memcpy(D.last_twist, D.xi, sizeof(D.xi));
    D.committed = D.slot;
    D.slot ^= 1;
  }
  D.active = false;
  D.timed = false;
}

}  // namespace tlh

extern "C" {

void tloam_deskew_default_config(tloam_deskew_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->direction = 1;
}

int tloam_deskew_configure(tloam_ctx* c, const tloam_deskew_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_deskew_config want = cfg_or_default(cfg, tloam_deskew_default_config);
  if (!deskew_config_ok(want)) return TLOAM_E_INVALID;
  // (the buffers stay: the registered scan of the last frame may be the deskewed copy)
  c->deskew.cfg = want;
  c->deskew.clear();
  return TLOAM_OK;
}

int tloam_deskew_get_info(tloam_ctx* c, tloam_deskew_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  const DeskewState& D = c->deskew;
  memset(info, 0, sizeof(*info));
  info->frames_deskewed = D.frames;
  info->last_frame = D.last_frame;
  memcpy(info->last_twist, D.last_twist, sizeof(D.last_twist));
  memcpy(info->next_motion_colmajor, c->odom.ready ? c->odom.step : kIdentity, sizeof(kIdentity));
  if (D.committed >= 0) {   // read here, not inside the frame
    unsigned long long bits = 0;
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipMemcpyAsync(&bits, D.ctl.p + D.committed, sizeof(bits), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    memcpy(&info->last_max_shift, &bits, sizeof(bits));
  }
  return TLOAM_OK;
}

int tloam_deskew_scan(tloam_ctx* c, const tloam_deskew_config* cfg, double scan_period, const double motion[16],
                      const double* xyz, const double* t_sec, size_t n, double* out) {
  if (!c || !cfg || !motion || c->nranks > 1) return TLOAM_E_INVALID;
  if (!deskew_config_ok(*cfg) || !(scan_period > 0.0) || !std::isfinite(scan_period)) return TLOAM_E_INVALID;
  const bool timed = cfg->time_source == 1;
  if (n > 0 && (!xyz || !out || (timed && !t_sec))) return TLOAM_E_INVALID;
  if (n > kMaxPoints || n > (size_t)INT32_MAX / 3) return TLOAM_E_INVALID;
  const bool identity = is_identity(motion);
  double xi[6] = {0, 0, 0, 0, 0, 0};
  if (!identity && !motion_log(motion, xi)) return TLOAM_E_INVALID;
  if (n == 0) return TLOAM_OK;
  if (identity && !timed) {   // no kernel, as in the frame
    memcpy(out, xyz, sizeof(double) * 3 * n);
    return TLOAM_OK;
  }
  DeskewState& D = c->deskew;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, D.s_in.reserve(3 * n)); HIPC(c, D.s_ctl.reserve(2));
  if (!identity) HIPC(c, D.s_out.reserve(3 * n));
  if (timed) HIPC(c, D.s_t.reserve(n));
  DeskewArgs A = args_of(*cfg, scan_period, xi);
  A.in = D.s_in.p;
  A.n = (long long)n;
  A.out = identity ? nullptr : D.s_out.p;
  A.max_shift = identity ? nullptr : D.s_ctl.p;
  HIPC(c, hipMemsetAsync(D.s_ctl.p, 0, 2 * sizeof(unsigned long long), c->stream));
  HIPC(c, hipMemcpyAsync(D.s_in.p, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  if (timed) {
    A.t = D.s_t.p;
    A.bad = D.s_ctl.p + 1;
    HIPC(c, hipMemcpyAsync(D.s_t.p, t_sec, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  }
  launch_deskew(A, c->stream);
  unsigned long long bad = 0;
  if (timed) HIPC(c, hipMemcpyAsync(&bad, D.s_ctl.p + 1, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
  if (!identity) HIPC(c, hipMemcpyAsync(out, D.s_out.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (bad) {
    c->last_error = "tloam_deskew_scan: a time is not finite or more than two sweeps from the pose's instant";
    return TLOAM_E_INVALID;
  }
  if (identity) memcpy(out, xyz, sizeof(double) * 3 * n);
  return TLOAM_OK;
}

}  // extern "C"
