// tl_api_map.hip -- C ABI of the odometry frame's global map and registered scan (include/tloam_hip.h: tloam_map_*,
// tloam_registered_scan): FrontEnd::spinOnce's /raw_cloud (front_end.cpp:84-86) and updateSubmap's mapping branch
// (:269-274), driven from tl_api_odom.hip (kernels in tl_map.hip).
//
// A later frame with mapping on: the map's storage is grown at the start of the frame, before anything of the odometry state
// changes (map_frame_reserve); after the scan match, the map's voxel job (tl_map.hip) appends the frame's voxels at the map's
// current end, its emit kernel posting the count to a pinned segment (map_stage_launch); the host reads it after the
// frame's last wait, which already follows it in the stream (map_stage_collect); an accepted frame commits it (map_frame_end).
#include <float.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

constexpr size_t kMapDefaultReserve = (size_t)1 << 21;   // points (48 MiB of SoA doubles): tloam_map_config.reserve_points = 0

bool map_config_ok(const tloam_map_config& m) {
  return m.voxel > 0.0 && m.voxel <= DBL_MAX && m.reserve_points >= 0;   // "[VoxelDownSample] voxel_size <= 0." (PointCloud2.cpp:361-363)
}

// the storage holds `need` points: new arrays of max(need, 2 cap), the points so far copied device to device behind whatever is
// in flight, the old arrays retired until the frame has drained the stream (map_frame_end)
int map_grow(tloam_ctx* c, size_t need) {
  MapState& M = c->map;
  MapState::Points& P = M.pts;
  if (need <= P.cap) return TLOAM_OK;
  if (!M.retired.empty()) {   // (a regrowth whose frame has not ended: not on the frame's path)
    HIPC(c, hipStreamSynchronize(c->stream));
    M.retired.release();
  }
  const size_t want = std::max(need, 2 * P.cap);
  Grower g(c, M.retired);
  for (DBuf<double>* a : {&P.x, &P.y, &P.z}) g.add(*a, want, (size_t)M.n_points);
  const int rc = g.commit("global map growth: ");
  if (rc != TLOAM_OK) return rc;
  P.cap = std::min(std::min(P.x.cap, P.y.cap), P.z.cap);
  return TLOAM_OK;
}

}  // namespace

namespace tlh {

// the start of a later frame: the map holds what this frame can append (at most one voxel per point), the voxel job's scratch
// holds the scan.  Nothing of the odometry state has changed yet: a failure here leaves the frame undone
int map_frame_reserve(tloam_ctx* c, size_t n) {
  MapState& M = c->map;
  M.pending_seq = 0;
  M.have_count = false;
  if (!M.cfg.enabled) return TLOAM_OK;
  int rc = map_grow(c, (size_t)M.n_points + n);
  if (rc != TLOAM_OK) return rc;
  const size_t m = std::max<size_t>(n, 1), cap = voxel_table_size(m), blocks = (m + 256) / 256 + 1;
  if (M.wx.cap < m || M.wy.cap < m || M.wz.cap < m) M.xf_seq = 0;   // (the last registered scan goes with the old scratch)
  HIPC(c, M.wx.reserve(m)); HIPC(c, M.wy.reserve(m)); HIPC(c, M.wz.reserve(m));
  HIPC(c, M.min_partial.reserve(3 * blocks)); HIPC(c, M.vmin.reserve(8)); HIPC(c, M.counts.reserve(8));
  if (!M.ctl.p) {   // [1] the ticket of k_map_front: zero between launches, so zero before the first
    HIPC(c, M.ctl.reserve(8));
    HIPC(c, hipMemsetAsync(M.ctl.p, 0, 8 * sizeof(int), c->stream));
  }
  HIPC(c, M.keys.reserve(cap + 1)); HIPC(c, M.head.reserve(cap + 1)); HIPC(c, M.first.reserve(cap + 1));
  HIPC(c, M.count.reserve(cap + 1)); HIPC(c, M.bigslot.reserve(cap + 1));
  HIPC(c, M.leader.reserve(blocks + 1));
  HIPC(c, M.slot_of_pt.reserve(m)); HIPC(c, M.next.reserve(m)); HIPC(c, M.members.reserve(m));
  HIPC(c, M.bigq.reserve((size_t)map_big_max(m))); HIPC(c, M.bigfill.reserve((size_t)map_big_max(m)));
  return TLOAM_OK;
}

// after the scan match: global_map += raw.Transform(pose).VoxelDownSample(voxel) (:269-274) on the scan resident in seg.aos,
// the means written at the map's end (map_frame_reserve made room for n).  Enqueued only
int map_stage_launch(tloam_ctx* c, const double pose[16], size_t n) {
  MapState& M = c->map;
  if (!M.cfg.enabled) return TLOAM_OK;
  MapVoxWork W;
  memset(&W, 0, sizeof(W));
  W.x = M.wx.p; W.y = M.wy.p; W.z = M.wz.p;
  W.n = n;
  W.voxel = M.cfg.voxel;
  W.lo = -DBL_MAX; W.hi = DBL_MAX;   // no crop; a non-finite return is in no voxel
  W.mask = voxel_table_size(std::max<size_t>(n, 1)) - 1;
  W.min_partial = M.min_partial.p; W.vmin = M.vmin.p;
  W.keys = M.keys.p; W.head = M.head.p; W.first = M.first.p; W.count = M.count.p; W.bigslot = M.bigslot.p;
  W.slot_of_pt = M.slot_of_pt.p; W.next = M.next.p; W.members = M.members.p;
  W.leader = M.leader.p; W.ctl = M.ctl.p; W.bigq = M.bigq.p; W.bigfill = M.bigfill.p;
  W.big_max = map_big_max(std::max<size_t>(n, 1));
  const size_t at = (size_t)M.n_points;
  W.ox = M.pts.x.p + at; W.oy = M.pts.y.p + at; W.oz = M.pts.z.p + at;
  W.n_out = M.counts.p;
  W.host_seg = M.seg.dev;
  W.host_seq = ++M.seq;
  W.use_ticket = (c->vox_ticket || (long long)(n + 256) / 256 > (long long)map_emit_resident_blocks(c->device_cus)) ? 1 : 0;
  W.fault = c->h_fault.dev + kFaultVoxEmit;
  MapFrontArgs A;
  memset(&A, 0, sizeof(A));
  A.aos = frame_scan(c); A.n = n;   // (the deskewed copy when the frame corrected its scan)
  for (int k = 0; k < 16; ++k) A.M[k] = pose[k];
  launch_map_voxel(A, W, c->stream);
  M.pending_seq = W.host_seq;
  M.xf_seq = c->seg.aos_seq;
  M.xf_n = n;
  return TLOAM_OK;
}

// after the frame's last wait (the submap's sizes, posted by a kernel behind the map stage's): the map stage's count and overflow
// flag are in pinned memory already -- read, not waited for
int map_stage_collect(tloam_ctx* c, tloam_odom_stats* st) {
  MapState& M = c->map;
  unsigned long long pay[7];
  int rc = collect_segment(c, M.seg, M.pending_seq, st, pay, [&](unsigned long long w[7]) -> int {
    unsigned long long count = 0;
    int ov = 0;
    HIPC(c, hipMemcpyAsync(&count, M.counts.p, sizeof(count), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(&ov, M.ctl.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    w[0] = count;
    w[2] = ov;
    return (int)(sizeof(count) + sizeof(int));
  });
  if (rc != TLOAM_OK) return rc < 0 ? rc : TLOAM_OK;   // (1: nothing pending)
  rc = check_device_faults(c);   // (k_map_emit's bounded look-back)
  if (rc != TLOAM_OK) return rc;
  M.have_count = true;
  M.new_points = (int64_t)pay[0];
  M.overflowed = pay[2] != 0;
  return TLOAM_OK;
}

// the frame has ended (the stream has drained): storage a regrowth replaced is freed; an accepted frame's voxels join the map
void map_frame_end(tloam_ctx* c, bool accepted) {
  MapState& M = c->map;
  M.retired.release();
  if (accepted && M.have_count) {
    if (M.overflowed) {
      M.overflow_frames++;   // "[VoxelDownSample] voxel_size is too small." (PointCloud2.cpp:370-372): appends nothing here
    } else {
      M.last_first = M.n_points;
      M.last_count = M.new_points;
      M.n_points += M.new_points;
      M.n_frames++;
    }
  }
  M.have_count = false;
  M.pending_seq = 0;
}

}  // namespace tlh

extern "C" {

void tloam_map_default_config(tloam_map_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->enabled = 0;      // mapping_flag (lidar_odometry.yaml:21)
  cfg->voxel = 1.0;      // front_end.cpp:272
  cfg->reserve_points = 0;
}

int tloam_map_configure(tloam_ctx* c, const tloam_map_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_map_config want = cfg_or_default(cfg, tloam_map_default_config);
  if (!map_config_ok(want)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  MapState& M = c->map;
  M.clear();
  if (!want.enabled) {   // mapping off: the frame's memory is what it was without the map
    const unsigned long long seq = M.seq;
    M = MapState();   // (every buffer and the segment freed)
    M.seq = seq;
    M.cfg = want;
    return TLOAM_OK;
  }
  HIPC(c, M.seg.alloc());
  const size_t reserve = want.reserve_points > 0 ? (size_t)want.reserve_points : kMapDefaultReserve;
  if (M.pts.cap < reserve) {   // (the map is empty: nothing to copy)
    M.pts = MapState::Points();
    const int rc = map_grow(c, reserve);
    if (rc != TLOAM_OK) return rc;
    M.retired.release();
  }
  M.cfg = want;
  return TLOAM_OK;
}

int tloam_map_get_info(tloam_ctx* c, tloam_map_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  const MapState& M = c->map;
  info->n_points = M.n_points;
  info->n_frames = M.n_frames;
  info->last_first = M.last_first;
  info->last_count = M.last_count;
  info->capacity_points = (int64_t)M.pts.cap;
  info->overflow_frames = M.overflow_frames;
  return TLOAM_OK;
}

int tloam_map_read(tloam_ctx* c, size_t first, size_t count, double* out) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const MapState& M = c->map;
  const size_t np = (size_t)M.n_points;
  if (first > np || count > np - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!out) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, c->misc.reserve(3 * count));
  launch_soa_to_aos(M.pts.x.p + first, M.pts.y.p + first, M.pts.z.p + first, count, c->misc.p, c->stream);
  HIPC(c, hipMemcpyAsync(out, c->misc.p, sizeof(double) * 3 * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_registered_scan(tloam_ctx* c, size_t capacity, size_t* n, double* out) {
  if (n) *n = 0;
  if (!c || !n || c->nranks > 1) return TLOAM_E_INVALID;
  const OdomState& O = c->odom;
  const MapState& M = c->map;
  if (!O.ready || !O.reg_valid) return TLOAM_E_NOT_READY;
  // the map stage's transform of that very scan (mapping on), else the scan itself if it is still the segmentation's input
  const bool from_map = M.xf_seq != 0 && M.xf_seq == O.reg_seq && M.wx.p;
  const bool from_seg = c->seg.aos_seq == O.reg_seq && c->seg.aos.p;
  if (!from_map && !from_seg) return TLOAM_E_NOT_READY;
  const size_t m = O.reg_n;
  *n = m;
  if (m == 0) return TLOAM_OK;
  if (capacity < m || !out) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, c->misc.reserve(3 * m));
  if (from_map) launch_soa_to_aos(M.wx.p, M.wy.p, M.wz.p, m, c->misc.p, c->stream);
  else launch_transform_aos(O.reg_deskewed ? c->deskew.aos.p : c->seg.aos.p, m, O.reg_pose, c->misc.p, c->stream);
  HIPC(c, hipMemcpyAsync(out, c->misc.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

}  // extern "C"
