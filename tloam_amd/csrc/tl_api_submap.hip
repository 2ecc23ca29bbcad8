// tl_api_submap.hip -- C ABI of the device-resident submap (include/tloam_hip.h: tloam_submap_*, tloam_get_target):
// FrontEnd::updateSubmap (front_end.cpp:201-275) and the first-frame branch (:283-304) driven on the device
// (kernels in tl_submap.hip).  The result is written straight into the SoA target arrays of the context.
#include "tl_ctx.hpp"

using namespace tl;

namespace {
int submap_reserve_work(tloam_ctx* c, size_t n) {
  SubmapState& S = c->submap;
  const size_t m = std::max<size_t>(n, 1), cap = voxel_table_size(m);
  HIPC(c, S.min_partial.reserve(256 * 6)); HIPC(c, S.vmin.reserve(8)); HIPC(c, S.counts.reserve(8));
  if (!S.overflow.p) {   // [0] overflow flag, [1] the ticket of k_vox_min2: zero between launches, so zero before the first
    HIPC(c, S.overflow.reserve(8));
    HIPC(c, hipMemsetAsync(S.overflow.p, 0, 8 * sizeof(int), c->stream));
  }
  HIPC(c, S.keys.reserve(cap + 1)); HIPC(c, S.cnt.reserve(cap + 1));
  HIPC(c, S.slot_of_pt.reserve(m)); HIPC(c, S.urank.reserve(m)); HIPC(c, S.members.reserve(m));
  HIPC(c, S.leader.reserve(m + 1)); HIPC(c, S.leader_scan.reserve(2));   // (two control words: tl_common.hpp VoxelWork)
  return TLOAM_OK;
}
// One launch sequence for one or two clouds stored back to back in (wx, wy, wz): segment s = points
// [s ? n0 : 0, s ? n : n0) -> target[kind[s]] = VoxelDownSample(Crop(segment, box[s]), voxel[s]); sizes to counts[s].
// A single cloud: n0 == n, kind[1] ignored.
struct CropVoxelSeg { int kind; size_t n; const double* lo; const double* hi; double voxel; };
// out: the down-sampled clouds go there (SoA per segment) instead of the target arrays of seg[s].kind
int submap_job(tloam_ctx* c, const CropVoxelSeg seg[2], int nseg, VoxelJob* Jout, VoxelWork* Wout,
               double* const (*out)[3] = nullptr) {
  SubmapState& S = c->submap;
  const size_t n0 = seg[0].n, n = n0 + (nseg > 1 ? seg[1].n : 0);
  int rc = submap_reserve_work(c, n);
  if (rc != TLOAM_OK) return rc;
  VoxelJob J;
  J.x = S.wx.p; J.y = S.wy.p; J.z = S.wz.p;
  J.n = n;
  J.n0 = n0;
  VoxelWork W;
  for (int s = 0; s < 2; ++s) {
    const CropVoxelSeg& G = seg[s < nseg ? s : 0];
    for (int a = 0; a < 3; ++a) { J.lo[s][a] = G.lo[a]; J.hi[s][a] = G.hi[a]; }
    J.voxel[s] = G.voxel;
    if (out) {
      for (int a = 0; a < 3; ++a) W.out[s][a] = out[s][a];
      continue;
    }
    KindData& K = c->kd[G.kind];
    if (s < nseg) {
      const size_t m = std::max<size_t>(G.n, 1);
      HIPC(c, K.tx.reserve(m)); HIPC(c, K.ty.reserve(m)); HIPC(c, K.tz.reserve(m));
    }
    W.out[s][0] = K.tx.p; W.out[s][1] = K.ty.p; W.out[s][2] = K.tz.p;
  }
  J.mask = voxel_table_size(std::max<size_t>(n, 1)) - 1;
  W.min_partial = S.min_partial.p; W.vmin = S.vmin.p;
  W.keys = S.keys.p; W.cnt = S.cnt.p;
  W.slot_of_pt = S.slot_of_pt.p; W.urank = S.urank.p; W.members = S.members.p;
  W.leader = S.leader.p; W.leader_scan = S.leader_scan.p; W.overflow = S.overflow.p;
  W.n_out = S.counts.p;
  // the last slot of the result mirror is free outside scanMatching: the sizes come back through it
  W.host_seg = &c->h_mirror.dev[kMirrorSlots - 1].w[0];
  W.host_seq = ++c->mirror_seq;
  W.use_ticket = (c->vox_ticket || (long long)(n + 256) / 256 > (long long)vox_emit_resident_blocks(c->device_cus)) ? 1 : 0;
  W.fault = c->h_fault.dev + kFaultVoxEmit;
  S.pending_seq = W.host_seq;
  *Jout = J;
  *Wout = W;
  return TLOAM_OK;
}
int submap_crop_voxel(tloam_ctx* c, const CropVoxelSeg seg[2], int nseg) {
  VoxelJob J;
  VoxelWork W;
  const int rc = submap_job(c, seg, nseg, &J, &W);
  if (rc != TLOAM_OK) return rc;
  launch_crop_voxel(J, W, c->stream);
  return TLOAM_OK;
}
int submap_upload(tloam_ctx* c, const double* xyz, size_t n, hipMemcpyKind from = hipMemcpyHostToDevice) {  // AoS -> in_aos (device)
  SubmapState& S = c->submap;
  HIPC(c, S.in_aos.reserve(3 * std::max<size_t>(n, 1)));
  if (n > 0) HIPC(c, hipMemcpyAsync(S.in_aos.p, xyz, sizeof(double) * 3 * n, from, c->stream));
  return TLOAM_OK;
}
int submap_finish(tloam_ctx* c, size_t* n_edge, size_t* n_ground) {  // the ONE host sync of an update
  SubmapState& S = c->submap;
  unsigned long long h[2] = {0, 0};
  int ov = 0;
  bool have = false;
  if (S.pending_seq) {  // the sizes arrive in pinned memory with the last kernel (everything before it has completed)
    const unsigned long long* seg = &c->h_mirror[kMirrorSlots - 1].w[0];
    unsigned long long pay[7];
    const int rc = wait_segment(c, seg, S.pending_seq, pay);
    if (rc < 0) return rc;
    if (rc == TLOAM_OK) { h[0] = pay[0]; h[1] = pay[1]; ov = (int)pay[2]; have = true; }
    S.pending_seq = 0ull;
  }
  if (!have) {
    HIPC(c, hipMemcpyAsync(h, S.counts.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(&ov, S.overflow.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
  }
  if (tlh::check_device_faults(c) != TLOAM_OK) return TLOAM_E_HIP;   // (k_vox_emit's bounded look-back ran out: see there)
  if (ov) {
    c->last_error = "[VoxelDownSample] voxel_size is too small.";  // PointCloud2.cpp:370-372
    return TLOAM_E_INVALID;
  }
  *n_edge = (size_t)h[0];
  *n_ground = (size_t)h[1];
  return TLOAM_OK;
}
const double kNoLo[3] = {-INFINITY, -INFINITY, -INFINITY}, kNoHi[3] = {INFINITY, INFINITY, INFINITY};

// ---- tloam_submap_update in its steps (front_end.cpp:201-264), in the order submap_update_body takes them ----
struct UpdateClouds {   // the call's clouds: on the host (borrowed for the call), or all null with `resident` set
  const double* pose;
  const double *planar, *edge, *ground;
  size_t n_planar, n_sphere, n_edge, n_ground;
  DBuf<double>* resident;   // planar | edge | ground, AoS, on this device already (submap_update_resident)
};
struct StagedBlock {      // where the frame's planar | edge | ground block went
  const double* view = nullptr;   // the pinned staging half as the device sees it (read in place), or null: the ring frame's buffer
  size_t off[3] = {0, 0, 0};      // first double of planar | edge | ground in the block
  int half = -1;                  // the staging half to release after the update (view != null)
};
struct Accumulated { int kind; size_t n_new; double L, voxel; size_t n_old, n_in; };   // the edge / the ground submap of an update

// :202-218 push the frame into a buffer, keep the newest `keep`: the frame that falls out is recycled
RingFrame* ring_push(std::vector<std::unique_ptr<RingFrame>>& ring, const double pose[16], size_t n, int keep) {
  std::unique_ptr<RingFrame> fresh;
  if ((int)ring.size() >= keep) {
    fresh = std::move(ring.front());
    ring.erase(ring.begin());
    while ((int)ring.size() >= keep) ring.erase(ring.begin());
  } else {
    fresh.reset(new RingFrame());
  }
  ring.push_back(std::move(fresh));
  RingFrame* const f = ring.back().get();
  f->n = n;
  memcpy(f->pose, pose, sizeof(double) * 16);
  return f;
}

// The three clouds the device needs (planar, edge, ground) are copied end to end into pinned staging (every cloud on a 16-byte
// boundary) and the update's front launch reads them THERE, across PCIe, through LDS: the planar cloud is copied to the newest
// ring frame's device buffer on the way (it is read again by the next planar_frame_size - 1 updates), the edge and ground clouds
// are needed by this launch only.  No copy command: a hipMemcpyAsync costs the calling thread ~10 us and the copy engine about
// as much before the first kernel can start, more than the update's kernels take.  (Three pageable copies: ~25 us each.)
// (Measured against the staged upload, round 4: 0.093-0.097 against 0.102-0.106 ms per update.)  More ring frames than one front
// launch takes: ONE asynchronous copy into the ring frame's buffer instead.
int stage_or_adopt(tloam_ctx* c, const UpdateClouds& in, RingFrame* f, StagedBlock* st) {
  const double* parts[3] = {in.planar, in.edge, in.ground};
  const size_t counts[3] = {3 * in.n_planar, 3 * in.n_edge, 3 * in.n_ground};
  if (in.resident) {   // the clouds are in the caller's device block already: it becomes the frame's buffer, nothing is staged
    std::swap(f->aos, *in.resident);
    tlh::staged_offsets(counts, 3, st->off);
    return TLOAM_OK;
  }
  const size_t all = std::max<size_t>(tlh::staged_size(counts, 3), 2) + 2;   // (+ 2: read / written in 16-byte steps)
  if (f->aos.cap < all) HIPC(c, hipStreamSynchronize(c->stream));   // regrowth: nothing may be in flight
  HIPC(c, f->aos.reserve(all));
  if (c->submap.cfg.planar_frame_size > submap_front_ring_max()) return tlh::stage_and_upload(c, parts, counts, 3, f->aos.p, st->off);
  const int rc = tlh::stage_in_place(c, parts, counts, 3, st->off, &st->view, &st->half);
  if (rc != TLOAM_E_NOT_READY) return rc;
  st->view = nullptr;   // no device view of the pinned block on this system: the pieces are staged, copy them
  HIPC(c, hipMemcpyAsync(f->aos.p, c->h_stage[st->half], sizeof(double) * tlh::staged_size(counts, 3), hipMemcpyHostToDevice, c->stream));
  return tlh::stage_release(c, st->half, /*completed=*/false);
}

// :220-243 both submaps are rebuilt from submap_planar_buffer (the sphere loop iterates the PLANAR buffer): their targets
// reserved.  *fused: all buffered frames are part of the update's front launch (k_submap_front); more frames than it takes are
// transformed here, one launch per buffered frame that writes both submaps
int rebuild_planar_sphere(tloam_ctx* c, bool* fused) {
  SubmapState& S = c->submap;
  size_t total = 0;
  for (const auto& f : S.planar_ring) total += f->n;
  KindData& P = c->kd[TLOAM_KIND_PLANAR];
  KindData& Q = c->kd[TLOAM_KIND_SPHERE];
  const size_t m = std::max<size_t>(total, 1);
  if (P.tx.cap < m || Q.tx.cap < m) HIPC(c, hipStreamSynchronize(c->stream));  // regrowth: nothing may be in flight
  HIPC(c, P.tx.reserve(m)); HIPC(c, P.ty.reserve(m)); HIPC(c, P.tz.reserve(m));
  HIPC(c, Q.tx.reserve(m)); HIPC(c, Q.ty.reserve(m)); HIPC(c, Q.tz.reserve(m));
  *fused = (int)S.planar_ring.size() <= submap_front_ring_max();
  if (!*fused) {
    size_t off = 0;
    for (const auto& f : S.planar_ring) {
      launch_transform_to_soa2(f->aos.p, f->n, f->pose, P.tx.p + off, P.ty.p + off, P.tz.p + off, Q.tx.p + off,
                               Q.ty.p + off, Q.tz.p + off, c->stream);
      off += f->n;
    }
  }
  P.n_tgt = Q.n_tgt = total;
  P.tgt_set = Q.tgt_set = true;
  return TLOAM_OK;
}

// A buffer about to be regrown (hipFree) must not be in use by the kernels still in flight: synchronise only then -- in steady
// state the capacities suffice and the update runs without a host wait.
// The edge / ground submaps are INPUT (the old points, read by the assembly) and OUTPUT (the crop + voxel job writes the new
// submap into the same arrays, sized for all n_in points): an array that has to grow keeps its old points.  (DBuf::reserve does
// not; until round 5 the one-launch front read the old points through the pointer of a block that the job's reserve had just
// freed -- right only as long as nobody else was handed that block in between.)
int grow_edge_ground(tloam_ctx* c, const Accumulated acc[2]) {
  SubmapState& S = c->submap;
  const size_t m = std::max<size_t>(acc[0].n_in + acc[1].n_in, 1);
  bool grow = S.wx.cap < m || S.slot_of_pt.cap < m || S.keys.cap < voxel_table_size(m) + 1 || S.leader.cap < m + 1;
  for (int s = 0; s < 2; ++s) grow = grow || c->kd[acc[s].kind].tx.cap < std::max<size_t>(acc[s].n_in, 1);
  if (grow) HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, S.wx.reserve(m)); HIPC(c, S.wy.reserve(m)); HIPC(c, S.wz.reserve(m));
  for (int s = 0; s < 2; ++s) {
    KindData& K = c->kd[acc[s].kind];
    const size_t need = std::max<size_t>(acc[s].n_in, 1);
    DBuf<double>* arr[3] = {&K.tx, &K.ty, &K.tz};
    for (DBuf<double>* b : arr) {
      if (need <= b->cap) continue;
      DBuf<double> nb;
      HIPC(c, nb.reserve(std::max(need, b->cap + b->cap / 2)));
      if (acc[s].n_old > 0 && b->p) {
        const hipError_t e = hipMemcpy(nb.p, b->p, sizeof(double) * acc[s].n_old, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { c->last_error = hipGetErrorString(e); return TLOAM_E_HIP; }
      }
      *b = std::move(nb);   // (the old array is freed)
    }
  }
  return TLOAM_OK;
}

// :246-264 per segment [old submap | scan->Transform(pose)] and the crop box pose.translation() +- L (:250-254, :259-262).  The
// scans were staged with the planar cloud, behind it: in the pinned block itself, or uploaded to the newest ring frame's buffer
void assemble_args(tloam_ctx* c, const double pose[16], const Accumulated acc[2], const StagedBlock& st, AssembleArgs* A,
                   double lo[2][3], double hi[2][3]) {
  const double* block = st.view ? st.view : c->submap.planar_ring.back()->aos.p;
  size_t base = 0;
  for (int s = 0; s < 2; ++s) {
    const KindData& K = c->kd[acc[s].kind];
    A->ox[s] = K.tx.p; A->oy[s] = K.ty.p; A->oz[s] = K.tz.p;
    A->aos[s] = block + st.off[1 + s];
    A->n_old[s] = acc[s].n_old; A->n_new[s] = acc[s].n_new; A->base[s] = base;
    for (int x = 0; x < 3; ++x) { lo[s][x] = pose[12 + x] - acc[s].L; hi[s][x] = pose[12 + x] + acc[s].L; }
    base += acc[s].n_in;
  }
  for (int i = 0; i < 16; ++i) A->M[i] = pose[i];
}

// ONE launch for the planar ring, the assembly of both clouds and the head of the crop + voxel job (table emptied, min bound),
// then the job from its insert pass on: the update is front | insert | emit
int fused_front(tloam_ctx* c, const AssembleArgs& A, const CropVoxelSeg seg[2], const StagedBlock& st) {
  SubmapState& S = c->submap;
  size_t ring_max = 0;
  const double* aos[16]; size_t nn[16]; const double* poses[16];
  int cnt = 0;
  for (const auto& f : S.planar_ring) { aos[cnt] = f->aos.p; nn[cnt] = f->n; poses[cnt] = f->pose; ring_max = std::max(ring_max, f->n); ++cnt; }
  if (st.view) aos[cnt - 1] = st.view + st.off[0];   // the newest frame: read in the staging, copied to f->aos on the way
  const size_t rows = submap_front_rows(ring_max, std::max(seg[0].n, seg[1].n));
  if (S.min_partial.cap < rows * 6) HIPC(c, hipStreamSynchronize(c->stream));   // regrowth: nothing may be in flight
  HIPC(c, S.min_partial.reserve(rows * 6));
  VoxelJob J;
  VoxelWork W;
  const int rc = submap_job(c, seg, 2, &J, &W);
  if (rc != TLOAM_OK) return rc;
  KindData& P = c->kd[TLOAM_KIND_PLANAR];
  KindData& Q = c->kd[TLOAM_KIND_SPHERE];
  launch_submap_front(cnt, aos, nn, poses, A, J, W, P.tx.p, P.ty.p, P.tz.p, Q.tx.p, Q.ty.p, Q.tz.p, S.wx.p, S.wy.p, S.wz.p, c->stream,
                      cnt - 1, st.view ? S.planar_ring.back()->aos.p : nullptr);
  launch_crop_voxel(J, W, c->stream, /*front_done=*/true);
  return TLOAM_OK;
}

int submap_update_body(tloam_ctx* c, const UpdateClouds& in) {
  SubmapState& S = c->submap;
  for (int k = 0; k < kKinds; ++k) c->tgt_box_valid[k] = false;  // the targets are about to be rebuilt on the device
  c->grids_ahead = false; c->tgt_gen++;
  // The sphere buffer is kept for its bookkeeping only (sizes, poses, frame count): nothing ever reads its points --
  // the sphere submap is rebuilt from the PLANAR buffer (front_end.cpp:221) -- so they are not uploaded.
  ring_push(S.sphere_ring, in.pose, in.n_sphere, S.cfg.sphere_frame_size);
  StagedBlock st;
  int rc = stage_or_adopt(c, in, ring_push(S.planar_ring, in.pose, in.n_planar, S.cfg.planar_frame_size), &st);
  if (rc != TLOAM_OK) return rc;
  bool fused = false;
  rc = rebuild_planar_sphere(c, &fused);
  if (rc != TLOAM_OK) return rc;
  // :246-264 edge / ground: submap += scan->Transform(pose); Crop(pose.translation() +- L)->VoxelDownSample
  // Both clouds go through ONE launch sequence (two segments of one job, tl_common.hpp VoxelJob): half the launches
  // of two separate jobs -- the update is bound by the host's launch rate, not by the device.
  Accumulated acc[2] = {{TLOAM_KIND_EDGE, in.n_edge, S.cfg.edge_crop_box_length, S.cfg.edge_down_sample_submap, 0, 0},
                        {TLOAM_KIND_GROUND, in.n_ground, S.cfg.ground_crop_box_length, S.cfg.ground_down_sample_submap, 0, 0}};
  for (Accumulated& a : acc) {
    const KindData& K = c->kd[a.kind];
    a.n_old = K.tgt_set ? K.n_tgt : 0;
    a.n_in = a.n_old + a.n_new;
  }
  // (an accumulated cloud is a cloud: the bound of the entry points holds for what they add up to as well)
  if (acc[0].n_in > kMaxPoints || acc[1].n_in > kMaxPoints) {
    c->last_error = "submap update: an accumulated cloud would exceed the 2^28 points a cloud may hold";
    return TLOAM_E_INVALID;
  }
  rc = grow_edge_ground(c, acc);
  if (rc != TLOAM_OK) return rc;
  AssembleArgs A;
  double lo[2][3], hi[2][3];
  assemble_args(c, in.pose, acc, st, &A, lo, hi);
  const CropVoxelSeg seg[2] = {{acc[0].kind, acc[0].n_in, lo[0], hi[0], acc[0].voxel}, {acc[1].kind, acc[1].n_in, lo[1], hi[1], acc[1].voxel}};
  if (fused) {
    rc = fused_front(c, A, seg, st);
  } else {
    launch_assemble(A, S.wx.p, S.wy.p, S.wz.p, c->stream);  // [old | Transform(new)] of both clouds, one launch
    rc = submap_crop_voxel(c, seg, 2);
  }
  if (rc != TLOAM_OK) return rc;
  size_t ne = 0, ng = 0;
  rc = submap_finish(c, &ne, &ng);
  // (the update's last kernel has completed, or -- on an error -- the caller drains the stream: the staging half is free)
  if (st.view) (void)tlh::stage_release(c, st.half, /*completed=*/true);
  if (rc != TLOAM_OK) return rc;
  c->kd[TLOAM_KIND_EDGE].n_tgt = ne;
  c->kd[TLOAM_KIND_GROUND].n_tgt = ng;
  c->kd[TLOAM_KIND_EDGE].tgt_set = c->kd[TLOAM_KIND_GROUND].tgt_set = true;
  return TLOAM_OK;
}
}  // namespace

namespace tlh {
bool submap_config_ok(const tloam_submap_config& want) {
  return want.planar_frame_size >= 1 && want.sphere_frame_size >= 1 && want.edge_down_sample_submap > 0.0 &&
         want.ground_down_sample_submap > 0.0 && want.ground_down_sample > 0.0;
}

// the first-frame branch on four clouds on the host (hipMemcpyHostToDevice) or on this device (hipMemcpyDeviceToDevice)
int submap_init_body(tloam_ctx* c, const tloam_submap_config& want, const double* planar, size_t n_planar, const double* sphere,
                     size_t n_sphere, const double* edge, size_t n_edge, const double* ground, size_t n_ground, hipMemcpyKind from) {
  SubmapState& S = c->submap;
  S = SubmapState();   // (the ring frames and the pipeline's scratch are freed; not inited)
  S.cfg = want;
  // :286 / :290-291 submap += cloud on empty submaps: the clouds as given
  int rc = set_target_copy(c, TLOAM_KIND_EDGE, edge, n_edge, from);
  if (rc == TLOAM_OK) rc = set_target_copy(c, TLOAM_KIND_PLANAR, planar, n_planar, from);
  if (rc == TLOAM_OK) rc = set_target_copy(c, TLOAM_KIND_SPHERE, sphere, n_sphere, from);
  if (rc != TLOAM_OK) return rc;
  // :287 ground += ground->VoxelDownSample(ground_down_sample)
  rc = submap_upload(c, ground, n_ground, from);
  if (rc != TLOAM_OK) return rc;
  const size_t m = std::max<size_t>(n_ground, 1);
  HIPC(c, S.wx.reserve(m)); HIPC(c, S.wy.reserve(m)); HIPC(c, S.wz.reserve(m));
  launch_aos_to_soa(S.in_aos.p, n_ground, S.wx.p, S.wy.p, S.wz.p, c->stream);
  rc = submap_reserve_work(c, n_ground);
  if (rc != TLOAM_OK) return rc;
  {  // one cloud; its size lands in counts[0]
    const CropVoxelSeg seg[2] = {{TLOAM_KIND_GROUND, n_ground, kNoLo, kNoHi, S.cfg.ground_down_sample},
                                 {TLOAM_KIND_GROUND, 0, kNoLo, kNoHi, S.cfg.ground_down_sample}};
    rc = submap_crop_voxel(c, seg, 1);
  }
  if (rc != TLOAM_OK) return rc;
  size_t ne = 0, ng = 0;
  rc = submap_finish(c, &ne, &ng);
  if (rc != TLOAM_OK) return rc;
  (void)ng;
  c->kd[TLOAM_KIND_GROUND].n_tgt = ne;  // (single-cloud job: counts[0])
  c->kd[TLOAM_KIND_GROUND].tgt_set = true;
  c->tgt_box_valid[TLOAM_KIND_GROUND] = false;
  c->grids_ahead = false; c->tgt_gen++;
  S.inited = true;
  return TLOAM_OK;
}

// tloam_submap_update on clouds already on this device: `block` holds planar | edge | ground, AoS, at the offsets staged_offsets
// gives the counts (3 n_planar, 3 n_edge, 3 n_ground), with room for two doubles behind; it becomes the newest planar ring
// frame's buffer (and gets the buffer of the frame that falls out, or none, in exchange)
int submap_update_resident(tloam_ctx* c, const double pose[16], size_t n_planar, size_t n_sphere, size_t n_edge, size_t n_ground,
                           DBuf<double>& block) {
  if (!c->submap.inited) return TLOAM_E_NOT_READY;
  for (int i = 0; i < 16; ++i)
    if (!(pose[i] - pose[i] == 0.0)) return TLOAM_E_BAD_POSE;
  const int rc = submap_update_body(c, UpdateClouds{pose, nullptr, nullptr, nullptr, n_planar, n_sphere, n_edge, n_ground, &block});
  if (rc != TLOAM_OK) (void)hipStreamSynchronize(c->stream);
  return rc;
}

// PointCloud2::VoxelDownSample of the SoA cloud(s) in submap.wx / wy / wz as ONE job of one or two segments (seg[s].n points
// each, back to back) with no crop, the means into out[s] (SoA).  Enqueued only; the sizes land in submap.counts, the overflow
// flag in submap.overflow (device words)
int voxel_down_sample_launch(tloam_ctx* c, const size_t n[2], const double voxel[2], int nseg, double* const out[2][3]) {
  const CropVoxelSeg seg[2] = {{TLOAM_KIND_EDGE, n[0], kNoLo, kNoHi, voxel[0]},
                               {TLOAM_KIND_GROUND, nseg > 1 ? n[1] : 0, kNoLo, kNoHi, voxel[nseg > 1 ? 1 : 0]}};
  VoxelJob J;
  VoxelWork W;
  const int rc = submap_job(c, seg, nseg, &J, &W, out);
  if (rc != TLOAM_OK) return rc;
  W.host_seg = nullptr;            // (the caller reads the sizes with the rest of its control words)
  c->submap.pending_seq = 0ull;
  launch_crop_voxel(J, W, c->stream);
  return TLOAM_OK;
}
}  // namespace tlh

extern "C" {

// ---- submap maintenance on the device (front_end.cpp:201-275, :283-304) ---------------------------
void tloam_submap_default_config(tloam_submap_config* cfg) {
  if (!cfg) return;
  cfg->planar_frame_size = 3;
  cfg->sphere_frame_size = 3;
  cfg->edge_crop_box_length = 100.0;
  cfg->ground_crop_box_length = 100.0;
  cfg->edge_down_sample_submap = 0.3;
  cfg->ground_down_sample_submap = 0.45;
  cfg->ground_down_sample = 0.3;
}

int tloam_submap_init(tloam_ctx* c, const tloam_submap_config* cfg, const double* planar, size_t n_planar,
                      const double* sphere, size_t n_sphere, const double* edge, size_t n_edge, const double* ground,
                      size_t n_ground) {
  if (!c || (n_planar && !planar) || (n_sphere && !sphere) || (n_edge && !edge) || (n_ground && !ground) ||
      n_planar > kMaxPoints || n_sphere > kMaxPoints || n_edge > kMaxPoints || n_ground > kMaxPoints)
    return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  const tloam_submap_config want = cfg_or_default(cfg, tloam_submap_default_config);
  if (!tlh::submap_config_ok(want))
    return TLOAM_E_INVALID;  // "[VoxelDownSample] voxel_size <= 0." (PointCloud2.cpp:361-363); the submap in place stays
  return tlh::submap_init_body(c, want, planar, n_planar, sphere, n_sphere, edge, n_edge, ground, n_ground, hipMemcpyHostToDevice);
}

int tloam_submap_update(tloam_ctx* c, const double pose[16], const double* planar, size_t n_planar,
                        const double* sphere, size_t n_sphere, const double* edge, size_t n_edge,
                        const double* ground, size_t n_ground) {
  if (!c || !pose || (n_planar && !planar) || (n_sphere && !sphere) || (n_edge && !edge) || (n_ground && !ground) ||
      n_planar > kMaxPoints || n_sphere > kMaxPoints || n_edge > kMaxPoints || n_ground > kMaxPoints)
    return TLOAM_E_INVALID;
  if (!c->submap.inited) return TLOAM_E_NOT_READY;
  // Open3D's Transform takes any 4x4 (front_end.cpp:246-247 hands it an Isometry3d's matrix: no orthogonality test anywhere on
  // this path), but a non-finite entry makes the crop box of :250-262 and every transformed point non-finite: a bad pose here
  // (the reference would go on with NaN clouds)
  for (int i = 0; i < 16; ++i)
    if (!(pose[i] - pose[i] == 0.0)) return TLOAM_E_BAD_POSE;
  HIPC(c, hipSetDevice(c->device));
  const int rc = submap_update_body(c, UpdateClouds{pose, planar, edge, ground, n_planar, n_sphere, n_edge, n_ground, nullptr});
  // The host clouds are borrowed for the call only and are copied asynchronously; the success path ends in the one
  // synchronisation of submap_finish -- every error path must drain the stream before the buffers go back.
  if (rc != TLOAM_OK) (void)hipStreamSynchronize(c->stream);
  return rc;
}

int tloam_voxel_down_sample(tloam_ctx* c, double voxel, const double* xyz, size_t n, double* out, size_t capacity,
                            size_t* n_out) {
  if (n_out) *n_out = 0;
  if (!c || !n_out || (n > 0 && !xyz) || n > kMaxPoints) return TLOAM_E_INVALID;
  if (!(voxel > 0.0)) {
    c->last_error = "[VoxelDownSample] voxel_size <= 0.";  // PointCloud2.cpp:361-363
    return TLOAM_E_INVALID;
  }
  HIPC(c, hipSetDevice(c->device));
  SubmapState& S = c->submap;
  OdomState& O = c->odom;
  const size_t m = std::max<size_t>(n, 1);
  HIPC(c, S.wx.reserve(m)); HIPC(c, S.wy.reserve(m)); HIPC(c, S.wz.reserve(m)); HIPC(c, O.vox_out.reserve(3 * m));
  int rc = submap_upload(c, xyz, n);
  if (rc != TLOAM_OK) return rc;
  launch_aos_to_soa(S.in_aos.p, n, S.wx.p, S.wy.p, S.wz.p, c->stream);
  // one segment, a single-cloud job as tloam_submap_init's ground (its sizes come back through the result mirror)
  const CropVoxelSeg seg[2] = {{TLOAM_KIND_GROUND, n, kNoLo, kNoHi, voxel}, {TLOAM_KIND_GROUND, 0, kNoLo, kNoHi, voxel}};
  double* const outs[2][3] = {{O.vox_out.p, O.vox_out.p + m, O.vox_out.p + 2 * m}, {O.vox_out.p, O.vox_out.p + m, O.vox_out.p + 2 * m}};
  VoxelJob J;
  VoxelWork W;
  rc = submap_job(c, seg, 1, &J, &W, outs);
  if (rc != TLOAM_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  launch_crop_voxel(J, W, c->stream);
  size_t nv = 0, unused = 0;
  rc = submap_finish(c, &nv, &unused);
  if (rc != TLOAM_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
  *n_out = nv;
  if (nv == 0) return TLOAM_OK;
  if (capacity < nv || !out) return TLOAM_E_INVALID;
  HIPC(c, c->misc.reserve(3 * nv));
  launch_soa_to_aos(O.vox_out.p, O.vox_out.p + m, O.vox_out.p + 2 * m, nv, c->misc.p, c->stream);
  HIPC(c, hipMemcpyAsync(out, c->misc.p, sizeof(double) * 3 * nv, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_get_target(tloam_ctx* c, int kind, size_t capacity, size_t* n, double* xyz) {
  if (!c || kind < 0 || kind >= kKinds || !n) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  const KindData& K = c->kd[kind];
  *n = K.tgt_set ? K.n_tgt : 0;
  if (*n == 0) return TLOAM_OK;
  if (capacity < *n || !xyz) return TLOAM_E_INVALID;
  HIPC(c, c->misc.reserve(3 * *n));
  launch_soa_to_aos(K.tx.p, K.ty.p, K.tz.p, *n, c->misc.p, c->stream);
  HIPC(c, hipMemcpyAsync(xyz, c->misc.p, sizeof(double) * 3 * *n, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

}  // extern "C"
