// tl_api_carve.hip -- C ABI of the closed map's carve (include/tloam_hip.h: tloam_closed_map_carve*, _read_misses,
// _read_carved; kernels in tl_carve.hip).
//
// A carve takes the built closed map (CmapState: its rows, its table, the poses it was built with) and the host's keyframe
// table (PlaceState::kf) for the build's keyframes, uploads one span table for the ray mask and the poses, and enqueues three
// launches on the context's stream; it waits once, for the counters.  The counts M live beside the rows in id order and go with
// the closed map (CmapState::drop).  Nothing of the closed map or of anything else in the context is written.
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

bool carve_config_ok(const tloam_closed_map_carve_config& m) {
  return m.max_range > 0.0 && std::isfinite(m.max_range) && m.end_margin >= 0.0 && std::isfinite(m.end_margin) && m.radius > 0.0 &&
         m.ray_mask >= 0 && m.ray_mask <= 0xFF;
}

// the enqueue, the wait and the counters of a carve; the previous counts have been dropped
int carve_body(tloam_ctx* c, tloam_closed_map_carve_info& I) {
  CmapState& M = c->cmap;
  const PlaceState& P = c->place;
  const size_t K = M.poses.size() / 16;   // the build's keyframes: later ones cast no rays
  const int mask = M.carve_cfg.ray_mask ? M.carve_cfg.ray_mask : M.cfg.cloud_mask;
  std::vector<CmapSpan> spans;
  long long n = 0;
  for (size_t k = 0; k < K && k < P.kf.size(); ++k)
    for (int j = 0; j < 8; ++j) {
      if (!((mask >> j) & 1) || P.kf[k].n[j] == 0) continue;
      spans.push_back(CmapSpan{(long long)P.kf[k].off[j], n, (int)k, 0});
      n += (long long)P.kf[k].n[j];
    }
  const int nspan = (int)spans.size();
  spans.push_back(CmapSpan{0, n, 0, 0});   // (the end: span[nspan].start = n)
  const size_t nv = (size_t)M.info.n_voxels;
  HIPC(c, hipSetDevice(c->device));
  if (M.miss.cap < std::max<size_t>(nv, 1) || M.carve_ctl.cap < 8)
    HIPC(c, hipStreamSynchronize(c->stream));   // (the counts replaced may still be read)
  HIPC(c, M.miss.reserve(std::max<size_t>(nv, 1))); HIPC(c, M.carve_ctl.reserve(8));
  DBuf<CmapSpan> dspan;   // the carve's own, freed with it (hipFree waits for the launches that use them)
  DBuf<double> dpose;
  HIPC(c, dspan.reserve(spans.size())); HIPC(c, dpose.reserve(std::max<size_t>(16 * K, 16)));
  HIPC(c, hipMemcpyAsync(dspan.p, spans.data(), sizeof(CmapSpan) * spans.size(), hipMemcpyHostToDevice, c->stream));
  if (K) HIPC(c, hipMemcpyAsync(dpose.p, M.poses.data(), sizeof(double) * 16 * K, hipMemcpyHostToDevice, c->stream));
  CarveWork W;
  memset(&W, 0, sizeof(W));
  W.arena = P.arena.p;
  W.span = dspan.p;
  W.nspan = nspan;
  W.nkf = (int)K;
  W.n = n;
  W.pose = dpose.p;
  W.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) W.origin[a] = M.cfg.origin[a];
  W.max_range = M.carve_cfg.max_range;
  W.end_margin = M.carve_cfg.end_margin;
  W.radius2 = M.carve_cfg.radius * M.carve_cfg.radius;
  const VmapTable T = M.rows.table();
  W.pmask = T.pmask; W.ptab = T.ptab; W.pkey = T.pkey;
  W.pn = T.pn; W.pqx = T.pqx; W.pqy = T.pqy; W.pqz = T.pqz;
  W.nv = (long long)nv;
  W.miss = M.miss.p;
  W.ctl = M.carve_ctl.p;
  I.launches = launch_carve(W, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long ctl[8];
  HIPC(c, hipMemcpyAsync(ctl, M.carve_ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  I.n_keyframes = (int64_t)K;
  I.n_rays = (int64_t)n;
  I.skipped_rays = (int64_t)ctl[0];
  I.steps = (int64_t)ctl[1];
  I.tested = (int64_t)ctl[2];
  I.misses = (int64_t)ctl[3];
  I.voxels_missed = (int64_t)ctl[4];
  return TLOAM_OK;
}

}  // namespace

extern "C" {

void tloam_closed_map_carve_default_config(tloam_closed_map_carve_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->max_range = 60.0;
  cfg->end_margin = 1.0;
  cfg->radius = 0.25;
  cfg->ray_mask = 0;
}

int tloam_closed_map_carve_configure(tloam_ctx* c, const tloam_closed_map_carve_config* cfg) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  tloam_closed_map_carve_config want;
  if (cfg) want = *cfg;
  else tloam_closed_map_carve_default_config(&want);
  if (!carve_config_ok(want)) return TLOAM_E_INVALID;
  c->cmap.drop_carve();
  c->cmap.carve_cfg = want;
  return TLOAM_OK;
}

int tloam_closed_map_get_carve_info(tloam_ctx* c, tloam_closed_map_carve_info* info) {
  if (!c || !info || c->nranks > 1) return TLOAM_E_INVALID;
  *info = c->cmap.carve_info;
  return TLOAM_OK;
}

int tloam_closed_map_carve(tloam_ctx* c, tloam_closed_map_carve_info* info) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built) return TLOAM_E_NOT_READY;
  M.drop_carve();   // from here on a failure leaves no counts
  tloam_closed_map_carve_info I;
  memset(&I, 0, sizeof(I));
  const int rc = carve_body(c, I);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);   // (nothing of the carve is in flight when its span table goes)
    return rc;
  }
  M.carve_info = I;
  M.carved = true;
  if (info) *info = I;
  return TLOAM_OK;
}

int tloam_closed_map_read_misses(tloam_ctx* c, size_t first, size_t count, int64_t* misses) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  const CmapState& M = c->cmap;
  if (!M.built || !M.carved) return TLOAM_E_NOT_READY;
  const size_t nv = (size_t)M.info.n_voxels;
  if (first > nv || count > nv - first) return TLOAM_E_INVALID;
  if (count == 0) return TLOAM_OK;
  if (!misses) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipMemcpyAsync(misses, M.miss.p + first, sizeof(int64_t) * count, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

int tloam_closed_map_read_carved(tloam_ctx* c, const double* lo, const double* hi, int64_t min_count, int64_t min_miss,
                                 double miss_ratio, size_t capacity, size_t* n, double* centroids_aos, int64_t* counts,
                                 int64_t* misses) {
  if (n) *n = 0;
  if (!c || !n || (lo == nullptr) != (hi == nullptr) || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built || !M.carved) return TLOAM_E_NOT_READY;
  const size_t nv = (size_t)M.info.n_voxels;
  if (nv == 0) return TLOAM_OK;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (the scratch may be replaced)
  const size_t blocks = (nv + 255) / 256;
  HIPC(c, M.rd_c.reserve(3 * nv)); HIPC(c, M.rd_n.reserve(nv)); HIPC(c, M.rd_m.reserve(nv));
  HIPC(c, M.look.reserve(blocks + 1)); HIPC(c, M.ctl.reserve(8));
  HIPC(c, hipMemsetAsync(M.look.p, 0, sizeof(unsigned long long) * (blocks + 1), c->stream));
  HIPC(c, hipMemsetAsync(M.ctl.p, 0, sizeof(unsigned long long) * 8, c->stream));
  CarveReadArgs A;
  A.rows = voxel_rows_of(M, nv, "closed map").base;
  A.rows.first = 0; A.rows.count = nv;
  for (int a = 0; a < 3; ++a) { A.rows.lo[a] = lo ? lo[a] : 0.0; A.rows.hi[a] = hi ? hi[a] : 0.0; }
  A.rows.min_count = min_count;
  A.rows.out_c = M.rd_c.p; A.rows.out_n = M.rd_n.p;
  A.rows.look = M.look.p; A.rows.ctl = M.ctl.p;
  A.miss = (const long long*)M.miss.p;
  A.min_miss = min_miss;
  A.miss_ratio = miss_ratio;
  A.out_m = M.rd_m.p;
  A.boxed = lo ? 1 : 0;
  launch_carve_read(A, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long w[3];
  HIPC(c, hipMemcpyAsync(w, M.ctl.p, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (w[1]) {
    c->last_error = "closed map: a look-back of k_carve_box timed out";
    return TLOAM_E_HIP;
  }
  const size_t m = (size_t)w[2];
  *n = m;
  if (m == 0) return TLOAM_OK;
  if (capacity < m) return TLOAM_E_INVALID;
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  if (centroids_aos) HIPC(c, hipMemcpyAsync(centroids_aos, M.rd_c.p, sizeof(double) * 3 * m, D2H, c->stream));
  if (counts) HIPC(c, hipMemcpyAsync(counts, M.rd_n.p, sizeof(int64_t) * m, D2H, c->stream));
  if (misses) HIPC(c, hipMemcpyAsync(misses, M.rd_m.p, sizeof(int64_t) * m, D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}

}  // extern "C"
