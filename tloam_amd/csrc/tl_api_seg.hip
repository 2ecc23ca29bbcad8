// tl_api_seg.hip -- C ABI of the segmentation node (include/tloam_hip.h: tloam_seg_default_config, tloam_segment):
// Segmentation::spinOnce (segmentation.cpp:40-93) on the device (kernels in tl_seg.hip).
//
// One stream.  Every grid is sized by the input's n, so the launches go out back to back; sizes come to the host ONCE,
// after the last launch (the control block), and decide how much of each output list is copied back.
#include "tl_ctx.hpp"

using namespace tl;

namespace {

// initSections (:174-223): the section bounds, host side (a constant of the configuration)
int section_bounds(const tloam_seg_config& c, double out[16]) {
  const int model = c.sensor_model, num_sec = c.num_sec;
  const int width = static_cast<int>(std::ceil(1.0 * model) / num_sec);
  int bidx[16];
  for (int i = 0; i < num_sec; ++i) bidx[i] = width * (i + 1) - 1;
  double prev = 0.0, ang = c.init_angle;
  int nb = 0, sb = 0;
  for (int i = 0; i < model; ++i) {
    if (model == 64 && i == 31) ang += 1.7;
    double cur = c.sensor_height / std::tan(std::fabs(ang) / 180.0 * M_PI);
    cur = cur < c.sensor_max_range ? cur : c.sensor_max_range;
    if (i >= 1) {
      const double d = std::fabs(cur - prev);
      if (d >= 5.0 || d <= 0.0) continue;   // :202-205: neither the angle nor prevRadius advance
    }
    if (sb < num_sec && i == bidx[sb] && sb <= 3) {
      const double theta = std::fabs(ang / 180 * M_PI);
      out[nb++] = (theta != 0 && i < model) ? (double)static_cast<float>(c.sensor_height / tan(theta)) : c.sensor_max_range;
      sb++;
    }
    prev = cur;
    ang += c.vertical_res;
  }
  return nb;
}

bool config_ok(const tloam_seg_config& c) {
  if (c.sensor_model != 64 || c.quadrant != 4) return false;   // the HDL-64E lambda and four quadrants only
  if (c.num_sec < 1 || c.num_sec > 16 || c.max_iter < 1 || c.ground_seed_num < 0 || c.ground_seed_num > kSegMaxSeeds) return false;
  if (c.ring_min_num < 16 || c.min_seg < 0) return false;   // below 16 a ring's sectors would run backwards (:1291)
  if (!(c.delta_p > 0) || !(c.delta_a > 0) || !(c.start_r > 0) || !(c.delta_r >= 0) || !(c.near_dis >= 0)) return false;
  // voxel keys in 32 bits: (polarNum + 1) (width + 1) (height + 2) with the largest polarNum / height the stage admits
  const double width = std::round(360.0 / c.delta_a) + 1;
  const double cells = (kSegMaxBounds + 1.0) * (width + 1.0) * (180.0 / c.delta_p + 3.0);
  return cells < 2147483647.0;
}

}  // namespace

extern "C" {

void tloam_seg_default_config(tloam_seg_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->sensor_model = 64; c->scan_period = 0.1; c->sensor_height = 1.73; c->vertical_res = 0.4; c->init_angle = -24.9;
  c->sensor_min_range = 1.0; c->sensor_max_range = 120.0; c->near_dis = 3.0;
  c->quadrant = 4; c->num_sec = 3; c->dis = 0.3; c->max_iter = 3; c->ground_seed_num = 20; c->ring_min_num = 131;
  c->start_r = 0.35; c->delta_r = 0.0004; c->delta_p = 1.2; c->delta_a = 1.2; c->min_seg = 80;
}

}  // extern "C"

namespace tlh {
bool seg_config_ok(const tloam_seg_config& cfg) { return config_ok(cfg); }

// the upload-independent head of tloam_segment: the call is counted, the parameters formed, the buffers sized for n points
int segment_begin(tloam_ctx* c, const tloam_seg_config& cfg, size_t n, SegParams* out) {
  SegBuffers& S = c->seg;
  const bool first = S.frames == 0;   // minPolar / maxPolar: 5.0 on the node's first frame, 0.0 after resetParams (:1123)
  S.frames++;                         // (a frame that fails advances it too: DESIGN.md 11)
  if (n == 0) return TLOAM_E_TOO_FEW_POINTS;   // object_scan is empty (:1089-1092)
  S.aos_seq++;                        // the input buffer is about to be reallocated / overwritten (tloam_registered_scan)

  SegParams P;
  memset(&P, 0, sizeof(P));
  P.n = (int)n;
  P.num_sec = cfg.num_sec;
  P.n_regions = cfg.quadrant * cfg.num_sec;
  P.n_bounds = section_bounds(cfg, P.sec_bounds);
  P.near_th = cfg.near_dis * cfg.near_dis;
  P.sensor_height = cfg.sensor_height; P.min_range = cfg.sensor_min_range; P.max_range = cfg.sensor_max_range;
  P.plane_dis = cfg.dis; P.max_iter = cfg.max_iter; P.seed_num = cfg.ground_seed_num; P.ring_min = cfg.ring_min_num;
  P.min_seg = cfg.min_seg; P.start_r = cfg.start_r; P.delta_r = cfg.delta_r; P.delta_p = cfg.delta_p;
  P.delta_a = cfg.delta_a; P.polar_seed = first ? 5.0 : 0.0;
  size_t hcap = 16;
  while (hcap < 2 * n) hcap <<= 1;
  P.hash_mask = (int)(hcap - 1);

  const size_t R = (size_t)P.n_regions;
  HIPC(c, S.aos.reserve(3 * n)); HIPC(c, S.ctl.reserve(1)); HIPC(c, S.ring.reserve(n)); HIPC(c, S.cur.reserve(n));
  HIPC(c, S.cur_reg.reserve(n)); HIPC(c, S.ng.reserve(n)); HIPC(c, S.reg_mem.reserve(R * n)); HIPC(c, S.reg_flag.reserve(R * n));
  HIPC(c, S.reg_g.reserve(R * n)); HIPC(c, S.reg_v.reserve(R * n)); HIPC(c, S.ground.reserve(n)); HIPC(c, S.obj.reserve(n));
  HIPC(c, S.pol_val.reserve(3 * n)); HIPC(c, S.bounds.reserve(kSegMaxBounds)); HIPC(c, S.vox.reserve(4 * n));
  HIPC(c, S.hkey.reserve(hcap)); HIPC(c, S.hval.reserve(hcap)); HIPC(c, S.parent.reserve(n)); HIPC(c, S.csize.reserve(n));
  HIPC(c, S.croot.reserve(n)); HIPC(c, S.cl_root.reserve(n)); HIPC(c, S.cl_off.reserve(n)); HIPC(c, S.cl_size.reserve(n));
  HIPC(c, S.seg_local.reserve(n)); HIPC(c, S.seg_orig.reserve(n)); HIPC(c, S.seg_label.reserve(n));
  HIPC(c, S.boxes.reserve(6 * n)); HIPC(c, S.ring_list.reserve(n)); HIPC(c, S.cv.reserve(n)); HIPC(c, S.sorted.reserve(n));
  HIPC(c, S.genbuf.reserve(n)); HIPC(c, S.picked.reserve(n)); HIPC(c, S.edge_sec.reserve(kSegSectors * kSegEdgePerSector));
  HIPC(c, S.sec_cnt.reserve(2 * kSegSectors)); HIPC(c, S.sec_base.reserve(kSegSectors)); HIPC(c, S.edge.reserve(n));
  HIPC(c, S.general.reserve(n));
  *out = P;
  return TLOAM_OK;
}

// the stage on the scan resident in seg.aos: ends in the control block, no host synchronisation
int segment_launch(tloam_ctx* c, const SegParams& P) {
  SegBuffers& S = c->seg;
  const size_t n = (size_t)P.n, hcap = (size_t)P.hash_mask + 1;
  SegBufs B;
  B.aos = S.aos.p; B.ctl = S.ctl.p; B.ring = S.ring.p; B.cur = S.cur.p; B.cur_reg = S.cur_reg.p; B.ng = S.ng.p;
  B.reg_mem = S.reg_mem.p; B.reg_flag = S.reg_flag.p; B.reg_g = S.reg_g.p; B.reg_v = S.reg_v.p; B.ground = S.ground.p;
  B.obj = S.obj.p; B.pol_val = S.pol_val.p; B.bounds = S.bounds.p; B.vox = S.vox.p; B.hkey = S.hkey.p; B.hval = S.hval.p;
  B.parent = S.parent.p; B.csize = S.csize.p; B.croot = S.croot.p; B.cl_root = S.cl_root.p; B.cl_off = S.cl_off.p;
  B.cl_size = S.cl_size.p; B.seg_local = S.seg_local.p; B.seg_orig = S.seg_orig.p; B.seg_label = S.seg_label.p;
  B.boxes = S.boxes.p; B.ring_list = S.ring_list.p; B.cv = S.cv.p; B.sorted = S.sorted.p; B.genbuf = S.genbuf.p;
  B.picked = S.picked.p; B.edge_sec = S.edge_sec.p; B.sec_cnt = S.sec_cnt.p; B.sec_base = S.sec_base.p; B.edge = S.edge.p;
  B.general = S.general.p;
  HIPC(c, hipMemsetAsync(S.hkey.p, 0xff, sizeof(int) * hcap, c->stream));   // empty slot: key -1
  HIPC(c, hipMemsetAsync(S.hval.p, 0x7f, sizeof(int) * hcap, c->stream));   // above every index (atomicMin)
  HIPC(c, hipMemsetAsync(S.csize.p, 0, sizeof(int) * n, c->stream));
  launch_segment(P, B, c->stream);
  HIPC(c, hipGetLastError());
  return TLOAM_OK;
}
}  // namespace tlh

extern "C" {

int tloam_segment(tloam_ctx* c, const tloam_seg_config* cfg, const double* xyz, size_t n, int32_t* ring,
                  int32_t* ground_index, size_t* n_ground, int32_t* object_index, size_t* n_object,
                  int32_t* segmented_index, int32_t* segmented_label, size_t* n_segmented, int32_t* edge_index,
                  size_t* n_edge, int32_t* general_index, size_t* n_general, double* boxes, size_t box_capacity,
                  size_t* n_boxes) {
  size_t* counts[6] = {n_ground, n_object, n_segmented, n_edge, n_general, n_boxes};
  for (size_t* p : counts)
    if (p) *p = 0;
  if (!c || !cfg || (n > 0 && !xyz) || n > kMaxPoints || !config_ok(*cfg)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  SegBuffers& S = c->seg;
  SegParams P;
  int rc = segment_begin(c, *cfg, n, &P);
  if (rc != TLOAM_OK) return rc;
  HIPC(c, hipMemcpyAsync(S.aos.p, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
  rc = segment_launch(c, P);
  if (rc != TLOAM_OK) return rc;

  SegCtl ctl;
  HIPC(c, hipMemcpyAsync(&ctl, S.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));   // the one place sizes come back
  // the polarBounds loop would not end (:831); without an object point the node never reaches it (:1088-1092)
  if (ctl.invalid && ctl.n_obj > 0) return TLOAM_E_INVALID;

  const size_t ng = (size_t)ctl.n_ground, no = (size_t)ctl.n_obj, ns = (size_t)ctl.n_seg, ne = (size_t)ctl.n_edge,
               nge = (size_t)ctl.n_general, nb = (size_t)ctl.n_clusters;
  hipError_t e = hipSuccess;
  auto get = [&](void* dst, const void* src, size_t bytes) {
    if (dst && bytes && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
  };
  get(ring, S.ring.p, sizeof(int) * n);
  get(ground_index, S.ground.p, sizeof(int) * ng);
  get(object_index, S.obj.p, sizeof(int) * no);
  const bool ok = no > 0 && nb > 0;   // the node publishes nothing without an object point or a kept cluster (:1089, :1222)
  if (ok) {
    get(segmented_index, S.seg_orig.p, sizeof(int) * ns);
    get(segmented_label, S.seg_label.p, sizeof(int) * ns);
    get(edge_index, S.edge.p, sizeof(int) * ne);
    get(general_index, S.general.p, sizeof(int) * nge);
    get(boxes, S.boxes.p, sizeof(double) * 6 * std::min(nb, box_capacity));
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { c->last_error = hipGetErrorString(e); return TLOAM_E_HIP; }
  if (n_ground) *n_ground = ng;
  if (n_object) *n_object = no;
  if (!ok) return TLOAM_E_TOO_FEW_POINTS;
  if (n_segmented) *n_segmented = ns;
  if (n_edge) *n_edge = ne;
  if (n_general) *n_general = nge;
  if (n_boxes) *n_boxes = nb;
  return TLOAM_OK;
}

}  // extern "C"
