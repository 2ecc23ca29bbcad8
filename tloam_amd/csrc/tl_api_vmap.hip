// tl_api_vmap.hip -- C ABI of the odometry frame's merged voxel map (include/tloam_hip.h: tloam_voxel_map_*), driven from
// tl_api_odom.hip at the points where the append map's stage runs (kernels in tl_vmap.hip).
//
// A later frame with the voxel map on: the persistent map is grown at the start of the frame, before anything of the odometry
// state changes (vmap_frame_reserve); after the scan match the frame is staged in a table of its own and its new voxels are
// numbered, the counts posted to a pinned segment (vmap_stage_launch); the host reads them after the frame's last wait
// (vmap_stage_collect); an accepted frame's staging is committed by a launch the host does not wait for (vmap_frame_end).
#include <float.h>
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

constexpr size_t kVmapDefaultReserve = (size_t)1 << 20;   // voxels (40 MiB of rows, 8 MiB of table): reserve_voxels = 0
constexpr size_t kVmapMaxVoxels = (size_t)1 << 30;        // ids are 32-bit

bool vmap_config_ok(const tloam_voxel_map_config& m) {
  return m.voxel > 0.0 && m.voxel <= DBL_MAX && std::isfinite(m.origin[0]) && std::isfinite(m.origin[1]) &&
         std::isfinite(m.origin[2]) && m.reserve_voxels >= 0;
}

// the map holds `need` voxels: new rows of max(need, 2 cap) with the voxels so far copied device to device behind whatever is in
// flight, a new table (load <= 1/2) rebuilt from the id-ordered keys -- ids and order never change --, the old storage retired
// until the frame has drained the stream (vmap_frame_end).  A failure leaves the map as it was
int vmap_grow(tloam_ctx* c, size_t need) {
  VmapState& V = c->vmap;
  VoxelRowStore& R = V.rows;
  if (need <= R.cap) return TLOAM_OK;
  if (!V.retired.empty()) {   // (a regrowth whose frame has not ended: not on the frame's path)
    HIPC(c, hipStreamSynchronize(c->stream));
    V.retired.release();
  }
  const size_t want = std::max(need, 2 * R.cap);
  if (want > kVmapMaxVoxels) {
    c->last_error = "voxel map: more than 2^30 voxels";
    return TLOAM_E_HIP;
  }
  size_t tsize = 1024;
  while (tsize < 2 * want) tsize <<= 1;
  const size_t nv = (size_t)V.n_voxels;
  Grower g(c, V.retired);
  g.add(R.key, want, nv);
  for (DBuf<long long>* a : {&R.n, &R.qx, &R.qy, &R.qz}) g.add(*a, want, nv);
  if (int* t = g.add(R.tab, tsize)) g.check(hipMemsetAsync(t, 0xff, sizeof(int) * tsize, c->stream));
  const int rc = g.commit("voxel map growth: ");
  if (rc != TLOAM_OK) return rc;
  R.cap = want;
  R.tmask = tsize - 1;
  V.tab_dirty = false;
  launch_vmap_rehash(R.table(), nv, c->stream);
  return TLOAM_OK;
}

VmapStageWork stage_work(tloam_ctx* c) {   // the staged frame's buffers, as k_vmap_commit reads them
  VmapState& V = c->vmap;
  VmapStageWork W;
  memset(&W, 0, sizeof(W));
  W.fmask = V.fmask;
  W.fkey = V.fkey.p; W.flead = V.flead.p; W.fsum = V.fsum.p; W.fid = V.fid.p; W.slot_of_pt = V.slot_of_pt.p;
  W.pmask = V.rows.tmask; W.ptab = V.rows.tab.p; W.pkey = V.rows.key.p;
  W.base = V.n_voxels;
  W.look = V.look.p; W.ctl = V.ctl.p;
  W.voxel = V.cfg.voxel;
  for (int a = 0; a < 3; ++a) W.origin[a] = V.cfg.origin[a];
  return W;
}

}  // namespace

namespace tlh {

// the start of a later frame: the map holds what this frame can add (at most one new voxel per point), the staging holds the
// scan.  Nothing of the odometry state has changed yet: a failure here leaves the frame undone
int vmap_frame_reserve(tloam_ctx* c, size_t n) {
  VmapState& V = c->vmap;
  V.pending_seq = 0;
  V.have_count = false;
  if (!V.cfg.enabled) return TLOAM_OK;
  int rc = vmap_grow(c, (size_t)V.n_voxels + n);
  if (rc != TLOAM_OK) return rc;
  if (V.tab_dirty) {
    HIPC(c, hipMemsetAsync(V.rows.tab.p, 0xff, sizeof(int) * (size_t)(V.rows.tmask + 1), c->stream));
    V.tab_dirty = false;
  }
  const size_t m = std::max<size_t>(n, 1), T = voxel_table_size(m), blocks = (m + 256) / 256 + 1;
  if (V.fkey.cap < T || V.fsum.cap < 4 * T || V.flead.cap < T || V.fid.cap < T || V.slot_of_pt.cap < m || V.look.cap < blocks + 1 ||
      V.ctl.cap < 8)
    HIPC(c, hipStreamSynchronize(c->stream));   // (the last frame's commit may still read the staging that is replaced)
  HIPC(c, V.fkey.reserve(T)); HIPC(c, V.fsum.reserve(4 * T)); HIPC(c, V.flead.reserve(T)); HIPC(c, V.fid.reserve(T));
  HIPC(c, V.slot_of_pt.reserve(m)); HIPC(c, V.look.reserve(blocks + 1)); HIPC(c, V.ctl.reserve(8));
  return TLOAM_OK;
}

// after the scan match, beside the append map's stage: the registered scan (the append map's transform when that map is on,
// else transformed here with the same expression) staged, its new voxels numbered.  Enqueued only
int vmap_stage_launch(tloam_ctx* c, const double pose[16], size_t n) {
  VmapState& V = c->vmap;
  if (!V.cfg.enabled) return TLOAM_OK;
  V.fmask = voxel_table_size(std::max<size_t>(n, 1)) - 1;
  VmapStageWork W = stage_work(c);
  const MapState& M = c->map;
  if (M.cfg.enabled) { W.sx = M.wx.p; W.sy = M.wy.p; W.sz = M.wz.p; }   // (map_stage_launch has just written them)
  W.aos = frame_scan(c);   // (the deskewed copy when the frame corrected its scan)
  for (int k = 0; k < 16; ++k) W.M[k] = pose[k];
  W.n = n;
  W.host_seg = V.seg.dev;
  W.host_seq = ++V.seq;
  launch_vmap_stage(W, c->stream);
  V.pending_seq = W.host_seq;
  return TLOAM_OK;
}

// after the frame's last wait: the stage's counts are in pinned memory already -- read, not waited for
int vmap_stage_collect(tloam_ctx* c, tloam_odom_stats* st) {
  VmapState& V = c->vmap;
  unsigned long long pay[7];
  const int rc = collect_segment(c, V.seg, V.pending_seq, st, pay, [&](unsigned long long p[7]) -> int {
    unsigned long long w[8];
    HIPC(c, hipMemcpyAsync(w, V.ctl.p, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    p[0] = w[4]; p[1] = w[1]; p[2] = w[0]; p[3] = w[3];
    return (int)sizeof(w);
  });
  if (rc != TLOAM_OK) return rc < 0 ? rc : TLOAM_OK;   // (1: nothing pending)
  if (pay[3]) {
    c->last_error = "voxel map: a look-back of k_vmap_emit timed out";
    return TLOAM_E_HIP;
  }
  V.have_count = true;
  V.new_voxels = (int64_t)pay[0];
  V.new_points = (int64_t)pay[1];
  V.overflowed = pay[2] != 0;
  return TLOAM_OK;
}

// the frame has ended (the stream has drained): storage a regrowth replaced is freed; an accepted frame's staging is committed
// by a launch nothing waits for (later frames and reads are behind it on the stream), an unaccepted one's dropped
void vmap_frame_end(tloam_ctx* c, bool accepted) {
  VmapState& V = c->vmap;
  V.retired.release();
  if (accepted && V.have_count) {
    if (V.overflowed) {
      V.overflow_frames++;   // a finite point beyond 2^20 voxels of the origin: the frame adds nothing
    } else {
      launch_vmap_commit(stage_work(c), V.rows.table(), c->stream);
      V.n_voxels += V.new_voxels;
      V.n_points += V.new_points;
      V.last_new = V.new_voxels;
      V.n_frames++;
    }
  }
  V.have_count = false;
  V.pending_seq = 0;
}

int voxel_rows_read(tloam_ctx* c, const VoxelRows& R, size_t first, size_t count, double* centroids_aos, int64_t* counts) {
  if (first > R.nv || count > R.nv - first) return TLOAM_E_INVALID;
  if (count == 0 || (!centroids_aos && !counts)) return TLOAM_OK;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (the scratch may be replaced)
  HIPC(c, R.rd_c.reserve(3 * count)); HIPC(c, R.rd_n.reserve(count));
  VmapReadArgs A = R.base;
  A.first = first; A.count = count;
  A.out_c = R.rd_c.p; A.out_n = R.rd_n.p;
  launch_vmap_read(A, c->stream);
  if (centroids_aos)
    HIPC(c, hipMemcpyAsync(centroids_aos, R.rd_c.p, sizeof(double) * 3 * count, hipMemcpyDeviceToHost, c->stream));
  if (counts) HIPC(c, hipMemcpyAsync(counts, R.rd_n.p, sizeof(int64_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

}  // namespace tlh

extern "C" {

void tloam_voxel_map_default_config(tloam_voxel_map_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->enabled = 0;
  cfg->voxel = 1.0;
  cfg->origin[0] = cfg->origin[1] = cfg->origin[2] = 0.0;
  cfg->reserve_voxels = 0;
}

int tloam_voxel_map_configure(tloam_ctx* c, const tloam_voxel_map_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const tloam_voxel_map_config want = cfg_or_default(cfg, tloam_voxel_map_default_config);
  if (!vmap_config_ok(want)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));
  VmapState& V = c->vmap;
  V.clear();
  if (!want.enabled) {   // off: the frame's memory is what it was without the voxel map
    const unsigned long long seq = V.seq;
    V = VmapState();   // (every buffer and the segment freed)
    V.seq = seq;
    V.cfg = want;
    return TLOAM_OK;
  }
  HIPC(c, V.seg.alloc());
  const size_t reserve = want.reserve_voxels > 0 ? (size_t)want.reserve_voxels : kVmapDefaultReserve;
  if (V.rows.cap < reserve) {   // (the map is empty: nothing to copy)
    V.rows = VoxelRowStore();
    const int rc = vmap_grow(c, reserve);
    if (rc != TLOAM_OK) return rc;
    HIPC(c, hipStreamSynchronize(c->stream));
    V.retired.release();
  }
  V.cfg = want;
  return TLOAM_OK;
}

int tloam_voxel_map_get_info(tloam_ctx* c, tloam_voxel_map_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  const VmapState& V = c->vmap;
  info->n_voxels = V.n_voxels;
  info->n_points = V.n_points;
  info->n_frames = V.n_frames;
  info->last_new = V.last_new;
  info->capacity_voxels = (int64_t)V.rows.cap;
  info->overflow_frames = V.overflow_frames;
  return TLOAM_OK;
}

int tloam_voxel_map_read(tloam_ctx* c, size_t first, size_t count, double* centroids_aos, int64_t* counts) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  return voxel_rows_read(c, voxel_rows_of(c->vmap, (size_t)c->vmap.n_voxels, "voxel map"), first, count, centroids_aos, counts);
}

int tloam_voxel_map_read_box(tloam_ctx* c, const double lo[3], const double hi[3], int64_t min_count, size_t capacity, size_t* n,
                             double* centroids_aos, int64_t* counts) {
  if (n) *n = 0;
  if (!c || !lo || !hi || !n || c->nranks > 1) return TLOAM_E_INVALID;
  return voxel_rows_read_box(c, voxel_rows_of(c->vmap, (size_t)c->vmap.n_voxels, "voxel map"), lo, hi, min_count, capacity, n,
                             centroids_aos, counts, "k_vmap_box", {},
                             [&](const VmapReadArgs& A) { launch_vmap_read_box(A, c->stream); });
}

}  // extern "C"
