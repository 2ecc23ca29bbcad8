// tl_api_odom.hip -- C ABI of the odometry frame (include/tloam_hip.h: tloam_odom_default_config, tloam_odometry_reset,
// tloam_odometry_frame): FrontEnd::updateLidarOdometry (front_end.cpp:278-337) with processCloud (:181-199), fed by
// Segmentation::spinOnce, on the device.
//
// The stages are those of the public entry points, run from their device-resident halves (tl_ctx.hpp): the raw scan is the
// only cloud that is uploaded, and what the host glue of the stage chain gathered with numpy and uploaded again is gathered by
// k_gather_lists (tl_odom.hip) from the resident scan.  After each gather the launches are those of the chain, on the same bytes.
// Host waits (later frames): the segmentation's control block, the PCA cloud's bounds, the PCA / voxel sizes, the submap sizes --
// each where the next stage needs a size for a host-sized grid -- plus those of the scan match.
#include "tl_ctx.hpp"

using namespace tl;

namespace {

bool odom_config_ok(const tloam_odom_config& c) {
  return tlh::seg_config_ok(c.seg) && c.feature.K >= 3 && c.feature.K <= 20 && c.feature.radius >= 0.0 &&
         tlh::submap_config_ok(c.submap) && c.edge_down_sample > 0.0;
}

GatherJob aos_rows(const double* src, int src_n, double* dst, int n, const int* idx1, int n1, const int* idx2,
                   const int* count = nullptr) {
  GatherJob J;
  J.sx = src; J.sy = src + 1; J.sz = src + 2; J.ss = 3;
  J.dx = dst; J.dy = dst + 1; J.dz = dst + 2; J.ds = 3;
  J.idx1 = idx1; J.idx2 = idx2; J.count = count;
  J.n = n; J.n1 = n1; J.src_n = src_n;
  return J;
}
LoopSpan span(const double* src, size_t n, const int* idx = nullptr) {   // a cloud the frame hands on, for the keyframe clouds
  LoopSpan L;
  memset(&L, 0, sizeof(L));
  L.src = src; L.idx = idx; L.n = (long long)n;
  return L;
}
GatherJob soa_rows(const double* sx, const double* sy, const double* sz, int n, double* dst) {   // SoA -> AoS, row for row
  GatherJob J;
  J.sx = sx; J.sy = sy; J.sz = sz; J.ss = 1;
  J.dx = dst; J.dy = dst + 1; J.dz = dst + 2; J.ds = 3;
  J.idx1 = nullptr; J.idx2 = nullptr; J.count = nullptr;
  J.n = n; J.n1 = 0; J.src_n = n;
  return J;
}

constexpr size_t kMinCloud = 10;   // registration.cpp:928-929

int odometry_frame_impl(tloam_ctx* c, const double* xyz, const double* t_sec, size_t n, double pose_out[16],
                        tloam_odom_stats* stats);

// the frame after the reset is known; everything up to the scan match.  Returns the status; the sizes go to *st
int odometry_frame_body(tloam_ctx* c, const double* xyz, const double* t_sec, size_t n, double pose[16], tloam_odom_stats* st) {
  OdomState& O = c->odom;
  const tloam_odom_config& cfg = O.cfg;
  SegBuffers& S = c->seg;
  FeatBuffers& F = c->feat;
  SubmapState& M = c->submap;
  const bool first = O.frame == 0;

  // ---- the global map (mapping on, later frames): room for what this frame can append, before anything else changes
  int rc = first ? TLOAM_OK : map_frame_reserve(c, n);
  if (rc != TLOAM_OK) return rc;
  rc = first ? TLOAM_OK : vmap_frame_reserve(c, n);   // (the merged voxel map, likewise: tl_api_vmap.hip)
  if (rc != TLOAM_OK) return rc;
  rc = place_frame_reserve(c, n);   // (place recognition: room for one more keyframe, any frame; tl_api_place.hip)
  if (rc != TLOAM_OK) return rc;

  // ---- Segmentation::spinOnce on the raw scan: the one upload of the frame
  SegParams P;
  rc = segment_begin(c, cfg.seg, n, &P);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, hipMemcpyAsync(S.aos.p, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  st->h2d_bytes += (int64_t)(sizeof(double) * 3 * n);
  rc = deskew_frame_upload(c, t_sec, n, st);   // (deskew on: the times, timed mode; tl_api_deskew.hip)
  if (rc != TLOAM_OK) return rc;
  rc = segment_launch(c, P);   // on the raw scan: its ring recovery and gates follow the firing geometry
  if (rc != TLOAM_OK) return rc;
  // ---- deskew (on, with motion): the corrected copy every later stage of the frame reads (frame_scan)
  unsigned long long bad_time = 0;
  rc = deskew_frame_launch(c, n, &bad_time, st);
  if (rc != TLOAM_OK) return rc;
  SegCtl ctl;
  HIPC(c, hipMemcpyAsync(&ctl, S.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));   // wait 1: the sizes of the segmentation's lists (and the deskew's time check)
  st->d2h_bytes += (int64_t)sizeof(ctl);
  st->host_syncs++;
  if (bad_time) {
    c->last_error = "tloam_odometry_frame_timed: a time is not finite or more than two sweeps from the pose's instant";
    return TLOAM_E_INVALID;
  }
  if (ctl.invalid && ctl.n_obj > 0) return TLOAM_E_INVALID;   // (without an object point the node stops before polarBounds)
  const double* scan = frame_scan(c);
  if (ctl.n_obj <= 0 || ctl.n_clusters <= 0) return TLOAM_E_TOO_FEW_POINTS;   // the node publishes nothing
  const size_t ng = (size_t)ctl.n_ground, ne = (size_t)ctl.n_edge, nge = (size_t)ctl.n_general;
  st->n_ground = (int64_t)ng; st->n_edge = (int64_t)ne; st->n_general = (int64_t)nge;
  // every cloud the frame hands on is a subset of one of these three (or their voxel means)
  if (ng < kMinCloud || ne < kMinCloud || nge < kMinCloud) return TLOAM_E_TOO_FEW_POINTS;

  // ---- gather 1 (nothing is in flight: the buffers may grow): general -> the PCA cloud, edge | ground -> the voxel job
  rc = feature_reserve(c, cfg.feature, nge, F);
  if (rc != TLOAM_OK) return rc;
  const size_t nv = ne + ng;
  HIPC(c, M.wx.reserve(nv)); HIPC(c, M.wy.reserve(nv)); HIPC(c, M.wz.reserve(nv));
  HIPC(c, O.vox_out.reserve(3 * nv)); HIPC(c, O.ctl.reserve(8));
  {
    GatherArgs G;
    memset(&G, 0, sizeof(G));
    G.j[0] = aos_rows(scan, (int)n, F.aos.p, (int)nge, S.general.p, (int)nge, nullptr, &S.ctl.p->n_general);
    G.j[1] = aos_rows(scan, (int)n, M.wx.p, (int)ne, S.edge.p, (int)ne, nullptr, &S.ctl.p->n_edge);
    G.j[2] = aos_rows(scan, (int)n, M.wx.p + ne, (int)ng, S.ground.p, (int)ng, nullptr, &S.ctl.p->n_ground);
    for (int j = 1; j < 3; ++j) {   // the voxel job's input: SoA, edge then ground back to back
      const size_t base = j == 1 ? 0 : ne;
      G.j[j].dy = M.wy.p + base; G.j[j].dz = M.wz.p + base; G.j[j].ds = 1;
    }
    launch_gather_lists(G, 3, c->stream);
  }
  // ---- processCloud's VoxelDownSample of edge (edge_down_sample) and ground (ground_down_sample): ONE two-segment job
  double* vox_edge = O.vox_out.p;            // x, y, z of ne rows each
  double* vox_ground = O.vox_out.p + 3 * ne; // x, y, z of ng rows each
  if (!first) {
    const size_t segn[2] = {ne, ng};
    const double vs[2] = {cfg.edge_down_sample, cfg.submap.ground_down_sample};
    double* const outs[2][3] = {{vox_edge, vox_edge + ne, vox_edge + 2 * ne}, {vox_ground, vox_ground + ng, vox_ground + 2 * ng}};
    rc = voxel_down_sample_launch(c, segn, vs, 2, outs);
    if (rc != TLOAM_OK) return rc;
  }
  // ---- extractPlanarSphere over the general points (wait 2 inside: the cloud's bounds size the search grid)
  FeatArgs A;
  rc = feature_pca_run(c, cfg.feature, nge, F, &A);
  if (rc == TLOAM_OK) rc = feature_select_launch(c, cfg.feature, nge, F, A);
  if (rc != TLOAM_OK) return rc;
  st->host_syncs++;
  {
    OdomCountArgs K;
    K.total = F.scan.p + nge;
    K.ranked = F.out.p;
    K.planar_num = cfg.feature.planar_num; K.sphere_num = cfg.feature.sphere_num;
    K.planar_scan_thres = cfg.feature.planar_scan_thres; K.cvr_scan = cfg.feature.cvr_scan;
    K.vox_n = first ? nullptr : M.counts.p;   // (the first frame runs no voxel job here)
    K.vox_overflow = first ? nullptr : M.overflow.p;
    K.ctl = O.ctl.p;
    launch_odom_counts(K, c->stream);
  }
  int cnt[8];
  HIPC(c, hipMemcpyAsync(cnt, O.ctl.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));   // wait 3: the selections' and the voxel clouds' sizes
  st->d2h_bytes += (int64_t)sizeof(cnt);
  st->host_syncs++;
  rc = check_device_faults(c);   // (the grid build's single-pass scan, k_vox_emit's look-back: bounded waits)
  if (rc != TLOAM_OK) return rc;
  const size_t np = (size_t)cnt[0], ns = (size_t)cnt[1], nps = (size_t)cnt[2], nss = (size_t)cnt[3];
  st->n_planar_submap = (int64_t)np; st->n_sphere_submap = (int64_t)ns;
  st->n_planar_scan = (int64_t)nps; st->n_sphere_scan = (int64_t)nss;
  const int* pidx = reinterpret_cast<const int*>(F.out.p + np + ns);   // FeatRankOut: the planar list's point indices

  {   // ---- loop verification on: room in the keyframe cloud arena for this frame's eight clouds (tl_api_place.hip)
    const size_t ne_ds = first ? 0 : (size_t)cnt[4], ng_ds = first ? 0 : (size_t)cnt[5];
    const size_t n8[8] = {first ? 0 : nps, ng_ds, ne_ds, first ? 0 : nss, np, first ? ng : ng_ds, first ? ne : ne_ds, ns};
    rc = place_clouds_reserve(c, n8);
    if (rc != TLOAM_OK) return rc;
  }

  if (first) {
    // ---- :283-304: the submap IS this scan -- raw edge (not down-sampled, :286), the selections; ground voxel'd inside
    if (np < kMinCloud || ns < kMinCloud) return TLOAM_E_TOO_FEW_POINTS;
    const size_t counts[4] = {3 * np, 3 * ns, 3 * ne, 3 * ng};
    size_t off[4];
    const size_t total = staged_offsets(counts, 4, off);
    HIPC(c, O.block.reserve(total + 2));
    GatherArgs G;
    memset(&G, 0, sizeof(G));
    G.j[0] = aos_rows(scan, (int)n, O.block.p + off[0], (int)np, pidx, (int)nge, S.general.p);
    G.j[1] = aos_rows(scan, (int)n, O.block.p + off[1], (int)ns, nullptr, (int)nge, S.general.p);   // ranks (:188)
    G.j[2] = aos_rows(scan, (int)n, O.block.p + off[2], (int)ne, S.edge.p, (int)ne, nullptr);
    G.j[3] = aos_rows(scan, (int)n, O.block.p + off[3], (int)ng, S.ground.p, (int)ng, nullptr);
    launch_gather_lists(G, 4, c->stream);
    const double* B = O.block.p;   // (the keyframe's target clouds: as submap_init_body receives them; no source clouds)
    const LoopSpan kfc[8] = {span(nullptr, 0), span(nullptr, 0), span(nullptr, 0), span(nullptr, 0),
                             span(B + off[0], np), span(B + off[3], ng), span(B + off[2], ne), span(B + off[1], ns)};
    place_clouds_note(c, kfc);
    rc = submap_init_body(c, cfg.submap, O.block.p + off[0], np, O.block.p + off[1], ns, O.block.p + off[2], ne,
                          O.block.p + off[3], ng, hipMemcpyDeviceToDevice);
    if (rc != TLOAM_OK) return rc;
    st->host_syncs += 4;   // tloam_submap_init's: the three targets' bounds, the ground voxel's sizes
    memcpy(pose, O.last, sizeof(double) * 16);   // the init pose
    return TLOAM_OK;   // (:304 returns before updateSubmap: the first frame adds nothing to the global map)
  }

  if (cnt[6]) {
    c->last_error = "[VoxelDownSample] voxel_size is too small.";  // PointCloud2.cpp:370-372
    return TLOAM_E_INVALID;
  }
  const size_t ne_ds = (size_t)cnt[4], ng_ds = (size_t)cnt[5];
  st->n_edge_ds = (int64_t)ne_ds; st->n_ground_ds = (int64_t)ng_ds;
  // the eight clouds of the match (registration.cpp:928-929): refused before anything of the odometry state is touched
  if (nps < kMinCloud || ng_ds < kMinCloud || ne_ds < kMinCloud || nss < kMinCloud) return TLOAM_E_TOO_FEW_POINTS;
  for (int k = 0; k < kKinds; ++k)
    if (!c->kd[k].tgt_set || c->kd[k].n_tgt < kMinCloud) return TLOAM_E_TOO_FEW_POINTS;

  // ---- gather 2: the source frame (planar_scan, ground, edge, sphere_scan) into the registered block, and planar_submap |
  // edge | ground into the block the submap update takes as its newest ring frame
  const size_t n4[4] = {nps, ng_ds, ne_ds, nss};
  size_t cnt4[4], soff[4];
  rc = source_frame_reserve(c, n4, cnt4);
  if (rc != TLOAM_OK) return rc;
  staged_offsets(cnt4, kKinds, soff);
  const size_t rcounts[3] = {3 * np, 3 * ne_ds, 3 * ng_ds};
  size_t roff[3];
  const size_t rtotal = std::max<size_t>(staged_offsets(rcounts, 3, roff), 2) + 2;   // (as the update's staged block)
  HIPC(c, O.block.reserve(rtotal));
  {
    GatherArgs G;
    memset(&G, 0, sizeof(G));
    double* sp = c->src_pack.p;
    G.j[0] = aos_rows(scan, (int)n, sp + soff[TLOAM_KIND_PLANAR], (int)nps, pidx, (int)nge, S.general.p);
    G.j[1] = soa_rows(vox_ground, vox_ground + ng, vox_ground + 2 * ng, (int)ng_ds, sp + soff[TLOAM_KIND_GROUND]);
    G.j[2] = soa_rows(vox_edge, vox_edge + ne, vox_edge + 2 * ne, (int)ne_ds, sp + soff[TLOAM_KIND_EDGE]);
    G.j[3] = aos_rows(scan, (int)n, sp + soff[TLOAM_KIND_SPHERE], (int)nss, nullptr, (int)nge, S.general.p);   // ranks (:186)
    G.j[4] = aos_rows(scan, (int)n, O.block.p + roff[0], (int)np, pidx, (int)nge, S.general.p);
    G.j[5] = soa_rows(vox_edge, vox_edge + ne, vox_edge + 2 * ne, (int)ne_ds, O.block.p + roff[1]);
    G.j[6] = soa_rows(vox_ground, vox_ground + ng, vox_ground + 2 * ng, (int)ng_ds, O.block.p + roff[2]);
    launch_gather_lists(G, 7, c->stream);
  }
  source_frame_commit(c, true, soff);
  {   // the keyframe's clouds: the source frame, and the submap update's (its block; the sphere selection gathered by rank)
    const double* sp = c->src_pack.p;
    const double* B = O.block.p;   // (swapped into the planar ring by the update: the storage itself stays)
    const LoopSpan kfc[8] = {span(sp + soff[0], nps), span(sp + soff[1], ng_ds), span(sp + soff[2], ne_ds), span(sp + soff[3], nss),
                             span(B + roff[0], np), span(B + roff[2], ng_ds), span(B + roff[1], ne_ds),
                             span(scan, ns, S.general.p)};
    place_clouds_note(c, kfc);
  }

  // ---- scanMatching from the constant-velocity prediction (:321, :329-332)
  memset(&st->match, 0, sizeof(st->match));
  const int mrc = tloam_scan_match(c, O.predict, nullptr, pose, nullptr, 0, &st->match);
  if (mrc != TLOAM_OK && mrc != TLOAM_E_WEIGHT_RANGE) return mrc;
  // ---- updateSubmap's mapping branch (:269-274), enqueued ahead of the submap update so that wait 4 follows it: the raw scan
  // transformed by the pose, voxel-gridded, appended to the global map (mapping on; tl_api_map.hip)
  rc = map_stage_launch(c, pose, n);
  if (rc != TLOAM_OK) return rc;
  rc = vmap_stage_launch(c, pose, n);   // the merged voxel map's staging of the same scan (voxel map on)
  if (rc != TLOAM_OK) return rc;
  // ---- updateSubmap (:336) with the planar submap selection, the sphere one's size, edge / ground as down-sampled
  rc = submap_update_resident(c, pose, np, ns, ne_ds, ng_ds, O.block);
  if (rc != TLOAM_OK) return rc;
  st->host_syncs++;   // wait 4: the submap's sizes
  rc = map_stage_collect(c, st);   // (the map stage's count: already in pinned memory)
  if (rc != TLOAM_OK) return rc;
  rc = vmap_stage_collect(c, st);   // (likewise)
  if (rc != TLOAM_OK) return rc;
  return mrc;
}

}  // namespace

extern "C" {

void tloam_odom_default_config(tloam_odom_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  tloam_seg_default_config(&cfg->seg);
  tloam_feature_default_config(&cfg->feature);
  tloam_submap_default_config(&cfg->submap);
  cfg->edge_down_sample = 0.1;   // lidar_odometry.yaml:8
}

int tloam_odometry_reset(tloam_ctx* c, const tloam_odom_config* cfg, const double init[16]) {
  if (!c) return TLOAM_E_INVALID;
  const tloam_odom_config want = cfg_or_default(cfg, tloam_odom_default_config);
  if (!odom_config_ok(want)) return TLOAM_E_INVALID;
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (init) {
    for (int i = 0; i < 16; ++i)
      if (!(init[i] - init[i] == 0.0)) return TLOAM_E_INVALID;
    memcpy(T, init, sizeof(T));
  }
  OdomState& O = c->odom;
  O.cfg = want;
  memcpy(O.last, T, sizeof(T));      // last_pose = init_pose (:281)
  memcpy(O.predict, T, sizeof(T));   // predicate_pose = init_pose (:282)
  for (int i = 0; i < 16; ++i) O.step[i] = (i % 5 == 0) ? 1.0 : 0.0;   // no motion before the second frame is accepted
  O.frame = 0;
  O.ready = true;
  O.reg_valid = false;   // no registered scan before the first frame
  c->map.clear();                // the global map starts again; its configuration stays
  c->vmap.clear();               // the merged voxel map too
  c->place.clear(c->stream);     // and the keyframe database (its configuration stays), with its clouds
  c->loop.clear();               // and the verified constraints (likewise)
  c->graph.drop();               // and the corrected keyframe poses (likewise)
  c->cmap.drop();                // and the closed map built from those keyframes (likewise)
  c->deskew.clear();             // (its configuration stays too)
  return TLOAM_OK;
}

int tloam_odometry_frame(tloam_ctx* c, const double* xyz, size_t n, double pose_out[16], tloam_odom_stats* stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  if (c && c->deskew.cfg.enabled && c->deskew.cfg.time_source == 1) return TLOAM_E_INVALID;   // timed mode takes times
  return odometry_frame_impl(c, xyz, nullptr, n, pose_out, stats);
}

int tloam_odometry_frame_timed(tloam_ctx* c, const double* xyz, const double* t_sec, size_t n, double pose_out[16],
                               tloam_odom_stats* stats) {
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!c || !t_sec || !c->deskew.cfg.enabled || c->deskew.cfg.time_source != 1) return TLOAM_E_INVALID;
  return odometry_frame_impl(c, xyz, t_sec, n, pose_out, stats);
}

}  // extern "C"

namespace {

int odometry_frame_impl(tloam_ctx* c, const double* xyz, const double* t_sec, size_t n, double pose_out[16],
                        tloam_odom_stats* stats) {
  if (!c || !pose_out || (n > 0 && !xyz) || n > kMaxPoints || n > (size_t)INT32_MAX / 3) return TLOAM_E_INVALID;
  if (c->nranks > 1) return TLOAM_E_INVALID;   // multi-rank frames: not offered (the match would need every rank's clouds)
  if (!c->odom.ready) return TLOAM_E_NOT_READY;
  if (c->active) return TLOAM_E_NOT_READY;     // between tloam_sm_begin and tloam_sm_end
  HIPC(c, hipSetDevice(c->device));
  OdomState& O = c->odom;
  tloam_odom_stats st;
  memset(&st, 0, sizeof(st));
  st.frame = O.frame;
  double T[16];
  const int rc = odometry_frame_body(c, xyz, t_sec, n, T, &st);
  (void)hipStreamSynchronize(c->stream);   // (a failed stage may have left work in flight; the success paths have drained)
  const bool accepted = rc == TLOAM_OK || rc == TLOAM_E_WEIGHT_RANGE;
  map_frame_end(c, accepted);
  vmap_frame_end(c, accepted);
  // place recognition: an accepted keyframe described from the scan the frame used, committed and searched -- enqueued after the
  // frame's last wait, not waited for (tl_api_place.hip)
  place_frame_end(c, accepted, O.frame, T, frame_scan(c), n);
  const bool deskewed = c->deskew.active;
  deskew_frame_end(c, accepted, O.frame);
  if (accepted) {
    // spinOnce's /raw_cloud (:84-86): this scan by lidar_odom_pose -- still Identity on the first frame (front_end.hpp:106),
    // whatever the init pose
    O.reg_valid = true;
    O.reg_seq = c->seg.aos_seq;
    O.reg_n = n;
    O.reg_deskewed = deskewed;
    if (O.frame > 0) memcpy(O.reg_pose, T, sizeof(T));
    else for (int i = 0; i < 16; ++i) O.reg_pose[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (O.frame > 0) {   // step_pose = last_pose^-1 * lidar_odom_pose; predicate_pose = lidar_odom_pose * step_pose (:329-332)
      double inv[16];
      rigid_inverse(O.last, inv);
      mat_mul(inv, T, O.step);   // (kept: the next frame's deskew motion)
      mat_mul(T, O.step, O.predict);
      memcpy(O.last, T, sizeof(T));
    }
    O.frame++;
    memcpy(pose_out, T, sizeof(T));
  }
  if (stats) *stats = st;
  return rc;
}

}  // namespace
