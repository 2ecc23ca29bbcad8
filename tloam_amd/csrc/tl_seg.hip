// tl_seg.hip -- the segmentation node on the device: Segmentation::spinOnce (segmentation.cpp:40-93) from the raw scan to
// the ground / object / segmented / edge / general index lists.  Compiled with -ffp-contract=off:
// every threshold is a discontinuous gate, no multiply-add is fused unless it is spelled out (none is).
//
// Launches (all on one stream, no size comes back to the host in between -- every grid is sized by the input's n):
//   k_seg_front    1 x 1024  near filter, quadrant codes, rings (saturating prefix count), z mean, height split, regions
//   k_seg_ground   R x 1024  one workgroup per region: members, lowest seeds, the plane-fit iterations, ground / vertical
//   k_seg_concat   1 x 1024  ground_scan and object_scan in (q, s) order, then non_ground_scan
//   k_seg_polar    grid      polarCor of every object point
//   k_seg_bounds   1 x 1024  min / max pitch and polar, polarBounds (one lane, the reference's sequential loop)
//   k_seg_voxel    grid      voxel coordinates + key, hash insert (smallest object index per voxel), union-find init
//   k_seg_union    grid      union over the neighbour voxels of searchKNN, edges taken as undirected
//   k_seg_flatten  grid      root per point, component sizes
//   k_seg_clusters 1 x 1024  kept clusters (size > minSeg), ranked by size desc / smallest member
//   k_seg_members  G x 1024  per cluster: members ascending, labels, bounding box
//   k_seg_ringcnt  64 x 1024 segmented points per ring
//   k_seg_ringlist 64 x 1024 the ring buckets in segmented order
//   k_seg_sector   384 x 256 curvature, sort, the pick walk, general entries of one (ring, sector)
//   k_seg_emit     1 x 1024  edge / general lists in (ring, sector) order
#include <math.h>

#include "tl_seg.hpp"

namespace tl {
namespace {

constexpr int kT = 1024;

// ---- block helpers (blockDim.x threads, at most 1024) -----------------------------------------------
template <class T>
__device__ T block_excl_scan(T v, T* sh, T* total) {
  const int t = threadIdx.x, n = blockDim.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < n; off <<= 1) {
    T a = t >= off ? sh[t - off] : T(0);
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  T incl = sh[t];
  *total = sh[n - 1];
  __syncthreads();
  return incl - v;
}

// fixed-order tree reductions (the same bits on every run)
__device__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int h = blockDim.x >> 1; h > 0; h >>= 1) {
    if (t < h) sh[t] = sh[t] + sh[t + h];
    __syncthreads();
  }
  double r = sh[0];
  __syncthreads();
  return r;
}
__device__ double block_min(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int h = blockDim.x >> 1; h > 0; h >>= 1) {
    if (t < h) sh[t] = fmin(sh[t], sh[t + h]);
    __syncthreads();
  }
  double r = sh[0];
  __syncthreads();
  return r;
}
__device__ double block_max(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int h = blockDim.x >> 1; h > 0; h >>= 1) {
    if (t < h) sh[t] = fmax(sh[t], sh[t + h]);
    __syncthreads();
  }
  double r = sh[0];
  __syncthreads();
  return r;
}

// stable compaction of [0, N): every thread owns one contiguous chunk; emit(i, position) in index order
template <class Pred, class Emit>
__device__ int block_compact(int N, Pred pred, Emit emit, int* sh) {
  const int nt = blockDim.x, t = threadIdx.x;
  const int C = (N + nt - 1) / nt;
  const int lo = min(N, t * C), hi = min(N, lo + C);
  int c = 0;
  for (int i = lo; i < hi; ++i) c += pred(i) ? 1 : 0;
  int total;
  int pos = block_excl_scan(c, sh, &total);
  for (int i = lo; i < hi; ++i)
    if (pred(i)) emit(i, pos++);
  __syncthreads();
  return total;
}

__device__ inline double sq3(double x, double y, double z) { return (x * x + y * y) + z * z; }

// OpenCV 4 cv::fastAtan2 (atan_f32): 7th-order polynomial in float, degrees (recalled upstream behaviour)
__device__ inline float fast_atan2f(float y, float x) {
  const float r2d = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * r2d, p3 = -0.3258083974640975f * r2d;
  const float p5 = 0.1555786518463281f * r2d, p7 = -0.04432655554792128f * r2d;
  const float eps = (float)2.220446049250313080847e-16;
  float ax = fabsf(x), ay = fabsf(y), a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + eps);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + eps);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

__device__ inline int quadrant_code(double x, double y) {
  if (x > 0 && y >= 0) return 1;
  if (x <= 0 && y > 0) return 2;
  if (x < 0 && y <= 0) return 3;
  return 4;
}

// ---- k_seg_front ------------------------------------------------------------------------------------
struct RingAgg {
  int cnt, tr, fq, lq;   // kept points, q4->q1 transitions inside, first / last quadrant code (0: none)
};
__device__ inline RingAgg ring_combine(const RingAgg& a, const RingAgg& b) {
  RingAgg r;
  r.cnt = a.cnt + b.cnt;
  r.tr = a.tr + b.tr + ((a.lq == 4 && b.fq == 1) ? 1 : 0);
  r.fq = a.cnt ? a.fq : b.fq;
  r.lq = b.cnt ? b.lq : a.lq;
  return r;
}

__device__ inline bool kept_point(const double* p, double th) {
  if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) return false;
  return sqrt(sq3(p[0], p[1], p[2])) >= th;   // :485: the norm against dis_th * dis_th
}

__global__ __launch_bounds__(kT) void k_seg_front(SegParams P, SegBufs B) {
  __shared__ RingAgg sa[kT];
  __shared__ double sd[kT];
  __shared__ int si[kT];
  const int t = threadIdx.x, n = P.n;
  const int C = (n + kT - 1) / kT;
  const int lo = min(n, t * C), hi = min(n, lo + C);
  // pass A: per chunk
  RingAgg a{0, 0, 0, 0};
  double zs = 0.0;
  for (int i = lo; i < hi; ++i) {
    const double* p = B.aos + 3 * (size_t)i;
    if (!kept_point(p, P.near_th)) continue;
    int q = quadrant_code(p[0], p[1]);
    if (a.cnt && a.lq == 4 && q == 1) a.tr++;
    if (!a.cnt) a.fq = q;
    a.lq = q;
    a.cnt++;
    zs += p[2];
  }
  sa[t] = a;
  __syncthreads();
  for (int off = 1; off < kT; off <<= 1) {
    RingAgg b = sa[t];
    if (t >= off) b = ring_combine(sa[t - off], b);
    __syncthreads();
    sa[t] = b;
    __syncthreads();
  }
  const RingAgg ex = t ? sa[t - 1] : RingAgg{0, 0, 0, 0};
  const int n_kept = sa[kT - 1].cnt;
  __syncthreads();
  const double zsum = block_sum(zs, sd);
  // estimateRingsAndTimes2 returns 1.0 on an empty cloud (:335-338); + 0.5 (:743)
  const double split = (n_kept ? zsum / (double)n_kept : 1.0) + 0.5;
  // pass B: non-ground per chunk
  int cng = 0;
  for (int i = lo; i < hi; ++i) {
    const double* p = B.aos + 3 * (size_t)i;
    if (kept_point(p, P.near_th) && p[2] > split) cng++;
  }
  int n_ng;
  const int ng0 = block_excl_scan(cng, si, &n_ng);
  // pass C: write
  int k = ex.cnt, g = ng0, prev = ex.lq, beam = ex.tr;
  for (int i = lo; i < hi; ++i) {
    const double* p = B.aos + 3 * (size_t)i;
    if (!kept_point(p, P.near_th)) {
      B.ring[i] = -1;
      continue;
    }
    int q = quadrant_code(p[0], p[1]);
    if (q == 1 && prev == 4) beam++;
    prev = q;
    B.ring[i] = min(beam, kSegRings - 1);
    if (p[2] > split) {
      B.ng[g++] = i;
    } else {
      const int c = k - g;   // current_scan position: kept so far minus non-ground so far
      B.cur[c] = i;
      const double x = p[0], y = p[1];
      const double r = sqrt(x * x + y * y);
      const float th = fast_atan2f((float)(-y), (float)x);
      int s = P.num_sec - 1;   // getSection: a bound past sectionBounds' end never matches
      for (int j = min(P.num_sec, P.n_bounds) - 1; j >= 0; --j)
        if (r < P.sec_bounds[j]) s = j;
      int qd = -1;
      if (th >= 0.0f && th < 90.0f) qd = 0;
      else if (th >= 90.0f && th < 180.0f) qd = 1;
      else if (th >= 180.0f && th < 270.0f) qd = 2;
      else if (th >= 270.0f && th < 360.0f) qd = 3;
      B.cur_reg[c] = qd < 0 ? -1 : qd * P.num_sec + s;
    }
    k++;
  }
  if (t == 0) {
    B.ctl->n_kept = n_kept;
    B.ctl->n_ng = n_ng;
    B.ctl->n_cur = n_kept - n_ng;
    B.ctl->mean_split = split;
  }
}

// ---- k_seg_ground: one workgroup per region (segmentGroundThread :626-731) -------------------------
__device__ void plane_fit(const double* aos, const int* mem, const unsigned char* flag, int m, double* sd, double pl[4]) {
  const int t = threadIdx.x;
  double sx = 0, sy = 0, sz = 0, cnt = 0;
  for (int k = t; k < m; k += blockDim.x)
    if (flag[k] & 1) {
      const double* p = aos + 3 * (size_t)mem[k];
      sx += p[0]; sy += p[1]; sz += p[2]; cnt += 1.0;
    }
  const double N = block_sum(cnt, sd);
  const double cx = block_sum(sx, sd) / N, cy = block_sum(sy, sd) / N, cz = block_sum(sz, sd) / N;
  double a[6] = {0, 0, 0, 0, 0, 0};
  for (int k = t; k < m; k += blockDim.x)
    if (flag[k] & 1) {
      const double* p = aos + 3 * (size_t)mem[k];
      const double rx = p[0] - cx, ry = p[1] - cy, rz = p[2] - cz;
      a[0] += rx * rx; a[1] += rx * ry; a[2] += rx * rz; a[3] += ry * ry; a[4] += ry * rz; a[5] += rz * rz;
    }
  const double xx = block_sum(a[0], sd) / N, xy = block_sum(a[1], sd) / N, xz = block_sum(a[2], sd) / N;
  const double yy = block_sum(a[3], sd) / N, yz = block_sum(a[4], sd) / N, zz = block_sum(a[5], sd) / N;
  const double dets[3] = {yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy};
  const double ax[3][3] = {{dets[0], xz * yz - xy * zz, xy * yz - xz * yy},
                           {xz * yz - xy * zz, dets[1], xy * xz - yz * xx},
                           {xy * yz - xz * yy, xy * xz - yz * xx, dets[2]}};
  double wx = 0, wy = 0, wz = 0;
  for (int d = 0; d < 3; ++d) {
    double w = dets[d] * dets[d];
    if (wx * ax[d][0] + wy * ax[d][1] + wz * ax[d][2] < 0.0) w = -w;
    wx += ax[d][0] * w; wy += ax[d][1] * w; wz += ax[d][2] * w;
  }
  const double nr = sqrt(wx * wx + wy * wy + wz * wz);
  if (nr > 0) { wx /= nr; wy /= nr; wz /= nr; }   // Eigen >= 3.3: normalize() leaves a zero vector as it is
  pl[0] = wx; pl[1] = wy; pl[2] = wz;
  pl[3] = -(wx * cx + wy * cy + wz * cz);
}

__device__ inline bool sub_gate(const double* p, int k, const SegParams& P) {
  const double r = sqrt(sq3(p[0], p[1], p[2]));
  return k % 10 == 0 && p[2] >= -1.5 * P.sensor_height && r >= P.min_range && r <= P.max_range;
}

__global__ __launch_bounds__(kT) void k_seg_ground(SegParams P, SegBufs B) {
  __shared__ int si[kT];
  __shared__ double sd[kT];
  __shared__ double seedz[kSegMaxSeeds];
  __shared__ double plane[4];
  const int r = blockIdx.x, t = threadIdx.x;
  const int n_cur = B.ctl->n_cur;
  int* mem = B.reg_mem + (size_t)r * P.n;
  unsigned char* flag = B.reg_flag + (size_t)r * P.n;
  const int* cur = B.cur;
  const int* creg = B.cur_reg;
  const int m = block_compact(
      n_cur, [&](int i) { return creg[i] == r; }, [&](int i, int pos) { mem[pos] = cur[i]; }, si);
  for (int k = t; k < m; k += kT) flag[k] = 0;
  // the lowest seed_num of the subsample by (z, k): rank by counting, early out once the rank is out of reach
  const int S = (m + 9) / 10;
  for (int a = t; a < S; a += kT) {
    const int ka = 10 * a;
    const double* pa = B.aos + 3 * (size_t)mem[ka];
    if (!sub_gate(pa, ka, P)) continue;
    int rank = 0;
    for (int b = 0; b < S && rank < P.seed_num; ++b) {
      const int kb = 10 * b;
      const double* pb = B.aos + 3 * (size_t)mem[kb];
      if (!sub_gate(pb, kb, P)) continue;
      if (pb[2] < pa[2] || (pb[2] == pa[2] && kb < ka)) rank++;
    }
    if (rank < P.seed_num) seedz[rank] = pa[2];
  }
  int c = 0;
  for (int a = t; a < S; a += kT) c += sub_gate(B.aos + 3 * (size_t)mem[10 * a], 10 * a, P) ? 1 : 0;
  const double n_sub = block_sum((double)c, sd);
  if (t == 0) {
    const int cnt = min((int)n_sub, P.seed_num);
    double s = 0.0;
    for (int j = 0; j < cnt; ++j) s += seedz[j];   // the sorted order's sum (:656-658)
    plane[0] = cnt != 0 ? s / cnt : 0;
  }
  __syncthreads();
  const double gate = plane[0] + P.plane_dis;
  __syncthreads();
  int ns = 0;
  for (int a = t; a < S; a += kT) {
    const int ka = 10 * a;
    const double* pa = B.aos + 3 * (size_t)mem[ka];
    if (sub_gate(pa, ka, P) && pa[2] < gate) { flag[ka] = 1; ns++; }
  }
  const double n_seed = block_sum((double)ns, sd);
  if (n_seed <= 3.0) {   // :666: the region is dropped
    if (t == 0) { B.ctl->reg_m[r] = m; B.ctl->reg_g[r] = 0; B.ctl->reg_v[r] = 0; }
    return;
  }
  double n_fit = n_seed;
  for (int it = 0; it < P.max_iter; ++it) {
    if (n_fit <= 3.0) break;   // :671: this and every later iteration is skipped
    double pl[4];
    plane_fit(B.aos, mem, flag, m, sd, pl);
    const bool last = it == P.max_iter - 1;
    int nf = 0;
    for (int k = t; k < m; k += kT) {
      const double* p = B.aos + 3 * (size_t)mem[k];
      const double dis = fabs(pl[0] * p[0] + pl[1] * p[1] + pl[2] * p[2] + pl[3]);
      unsigned char f;
      if (last) f = dis < P.plane_dis ? 1 : 2;    // 1 ground, 2 vertical
      else f = (dis < P.plane_dis && k % 5 == 0) ? 1 : 0;
      flag[k] = f;
      nf += f == 1;
    }
    n_fit = block_sum((double)nf, sd);
  }
  // (a skipped tail leaves the last fit set as ground and no vertical point: flags 1 / 0)
  int* g = B.reg_g + (size_t)r * P.n;
  int* v = B.reg_v + (size_t)r * P.n;
  const int ng = block_compact(
      m, [&](int k) { return flag[k] == 1; }, [&](int k, int pos) { g[pos] = mem[k]; }, si);
  const int nv = block_compact(
      m, [&](int k) { return flag[k] == 2; }, [&](int k, int pos) { v[pos] = mem[k]; }, si);
  if (t == 0) { B.ctl->reg_m[r] = m; B.ctl->reg_g[r] = ng; B.ctl->reg_v[r] = nv; }
}

// ---- k_seg_concat: groundRemove's merge (:722-727, :763) -------------------------------------------
__global__ __launch_bounds__(kT) void k_seg_concat(SegParams P, SegBufs B) {
  __shared__ int og[kSegMaxRegions + 1], ov[kSegMaxRegions + 1];
  const int t = threadIdx.x;
  if (t == 0) {
    og[0] = ov[0] = 0;
    for (int r = 0; r < P.n_regions; ++r) {
      og[r + 1] = og[r] + B.ctl->reg_g[r];
      ov[r + 1] = ov[r] + B.ctl->reg_v[r];
    }
  }
  __syncthreads();
  for (int r = 0; r < P.n_regions; ++r) {
    const int* g = B.reg_g + (size_t)r * P.n;
    const int* v = B.reg_v + (size_t)r * P.n;
    for (int k = t; k < og[r + 1] - og[r]; k += kT) B.ground[og[r] + k] = g[k];
    for (int k = t; k < ov[r + 1] - ov[r]; k += kT) B.obj[ov[r] + k] = v[k];
  }
  const int nv = ov[P.n_regions], n_ng = B.ctl->n_ng;
  for (int k = t; k < n_ng; k += kT) B.obj[nv + k] = B.ng[k];
  if (t == 0) {
    B.ctl->n_ground = og[P.n_regions];
    B.ctl->n_obj = nv + n_ng;
  }
}

// ---- k_seg_polar: convertToPolar (:791-823) ---------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_polar(SegParams P, SegBufs B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.ctl->n_obj) return;
  const double* p = B.aos + 3 * (size_t)B.obj[i];
  const double x = p[0], y = p[1], z = p[2];
  const double rho = sqrt(sq3(x, y, z));
  const double pitch = asin(z / rho) * 180.0 / M_PI;
  const double ang = atan2(y, x);
  const double az = ang > 0.0 ? ang * 180 / M_PI : (ang + 2 * M_PI) * 180 / M_PI;
  double* o = B.pol_val + 3 * (size_t)i;
  if (rho >= P.max_range || rho <= P.min_range) {   // keeps the zero entry of polarCor.resize
    o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
    B.vox[4 * (size_t)i + 3] = 0;   // marks "not in the min / max"
    return;
  }
  o[0] = rho; o[1] = pitch; o[2] = az;
  B.vox[4 * (size_t)i + 3] = 1;
}

// ---- k_seg_bounds: min / max and polarBounds (:816-835) ---------------------------------------------
__global__ __launch_bounds__(kT) void k_seg_bounds(SegParams P, SegBufs B) {
  __shared__ double sd[kT];
  const int t = threadIdx.x, n = B.ctl->n_obj;
  double mnp = 0.0, mxp = 0.0, mnr = P.polar_seed, mxr = P.polar_seed;   // minPitch / maxPitch start at 0 every frame
  for (int i = t; i < n; i += kT) {
    if (!B.vox[4 * (size_t)i + 3]) continue;
    const double* o = B.pol_val + 3 * (size_t)i;
    mnp = fmin(mnp, o[1]); mxp = fmax(mxp, o[1]); mnr = fmin(mnr, o[0]); mxr = fmax(mxr, o[0]);
  }
  mnp = block_min(mnp, sd); mxp = block_max(mxp, sd); mnr = block_min(mnr, sd); mxr = block_max(mxr, sd);
  if (t == 0) {
    int num = 0, invalid = 0, step = 1;
    double range = mnr;
    while (range <= mxr) {
      const double inc = P.start_r - step * P.delta_r;
      if (inc <= 0.0 || num >= kSegMaxBounds) { invalid = 1; break; }   // the reference's loop would not end
      range += inc;
      B.bounds[num++] = range;
      step++;
    }
    SegCtl* c = B.ctl;
    c->polar_num = num;
    c->invalid = invalid;
    c->width = (int)(round(360.0 / P.delta_a) + 1);
    c->height = (int)((mxp - mnp) / P.delta_p);
    c->min_pitch = mnp; c->max_pitch = mxp; c->min_polar = mnr; c->max_polar = mxr;
  }
}

// ---- k_seg_voxel: createHashTable (:843-870) --------------------------------------------------------
__device__ inline int hash_slot(int key, int mask) {
  unsigned h = (unsigned)key * 2654435761u;
  return (int)(h & (unsigned)mask);
}

__global__ __launch_bounds__(256) void k_seg_voxel(SegParams P, SegBufs B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const SegCtl* c = B.ctl;
  if (i >= c->n_obj || c->invalid) return;
  const double* o = B.pol_val + 3 * (size_t)i;
  const int pn = c->polar_num;
  // getPolarIndex: the first bound above the radius (the bounds increase strictly), else the last
  int lo = 0, hi = pn;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (o[0] < B.bounds[mid]) hi = mid; else lo = mid + 1;
  }
  const int pol = lo < pn ? lo : pn - 1;
  const int pit = (int)round((o[1] - c->min_pitch) / P.delta_p);
  const int az = (int)round(o[2] / P.delta_a);
  const int key = (az * (pn + 1) + pol) + pit * (pn + 1) * (c->width + 1);
  int* v = B.vox + 4 * (size_t)i;
  v[0] = pol; v[1] = pit; v[2] = az; v[3] = key;
  int s = hash_slot(key, P.hash_mask);
  for (;;) {
    const int prev = atomicCAS(&B.hkey[s], -1, key);
    if (prev == -1 || prev == key) break;
    s = (s + 1) & P.hash_mask;
  }
  atomicMin(&B.hval[s], i);
  B.parent[i] = i;
}

__device__ inline int hash_find(const int* hkey, int key, int mask) {
  int s = hash_slot(key, mask);
  for (;;) {
    const int k = hkey[s];
    if (k == key) return s;
    if (k == -1) return -1;
    s = (s + 1) & mask;
  }
}

__device__ inline int uf_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (parent words are read and halved through the device-coherent path: a stale word cached near the CU would make a
//  failed link retry forever)
__device__ inline int uf_find(int* parent, int x) {
  int p = uf_load(&parent[x]);
  while (p != x) {
    const int gp = uf_load(&parent[p]);
    if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving
    x = p;
    p = gp;
  }
  return x;
}

__device__ inline void uf_union(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }   // the larger root goes under the smaller: roots are component minima
    if (atomicCAS(&parent[a], a, b) == a) return;
  }
}

// ---- k_seg_union: DCVC (:912-985) as connected components over searchKNN's edges, taken as undirected -----
__global__ __launch_bounds__(256) void k_seg_union(SegParams P, SegBufs B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const SegCtl* c = B.ctl;
  if (i >= c->n_obj || c->invalid) return;
  const int* v = B.vox + 4 * (size_t)i;
  const int pol = v[0], pit = v[1], az = v[2], key = v[3];
  const int pn = c->polar_num, height = c->height, width = c->width;
  const int rep = B.hval[hash_find(B.hkey, key, P.hash_mask)];
  // a point in row height + 1 (:888) or in an azimuth column above 300 (:898: all three of its columns clamp to 300)
  // does not see its own voxel
  const bool own_seen = pit <= height && az <= 300;
  if (own_seen && i != rep) {           // points of one voxel: joined through its smallest member, which walks
    uf_union(B.parent, i, rep);
    return;
  }
  for (int z = pit - 1; z <= pit + 1; ++z) {
    if (z < 0 || z > height) continue;
    for (int y = pol - 1; y <= pol + 1; ++y) {
      if (y < 0 || y > pn) continue;
      for (int x = az - 1; x <= az + 1; ++x) {
        int ax = x;
        if (ax < 0) ax = width - 1;
        if (ax > 300) ax = 300;   // the reference's literal bound (:898)
        const int nk = (ax * (pn + 1) + y) + z * (pn + 1) * (width + 1);
        const int s = hash_find(B.hkey, nk, P.hash_mask);
        if (s >= 0) uf_union(B.parent, i, B.hval[s]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_seg_flatten(SegParams P, SegBufs B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const SegCtl* c = B.ctl;
  if (i >= c->n_obj || c->invalid) return;
  const int r = uf_find(B.parent, i);
  B.croot[i] = r;
  atomicAdd(&B.csize[r], 1);
}

// ---- k_seg_clusters: labelAnalysis (:995-1021) ------------------------------------------------------
__global__ __launch_bounds__(kT) void k_seg_clusters(SegParams P, SegBufs B) {
  __shared__ int si[kT];
  const int t = threadIdx.x;
  SegCtl* c = B.ctl;
  const int n = c->invalid ? 0 : c->n_obj;
  // roots of kept clusters, ascending (scratch: seg_local)
  const int K = block_compact(
      n, [&](int i) { return B.croot[i] == i && B.csize[i] > P.min_seg; }, [&](int i, int pos) { B.seg_local[pos] = i; }, si);
  // rank: size descending, ties by the smallest member (= the root)
  for (int a = t; a < K; a += kT) {
    const int ra = B.seg_local[a], sa = B.csize[ra];
    int rank = 0;
    for (int b = 0; b < K; ++b) {
      const int rb = B.seg_local[b], sb = B.csize[rb];
      rank += (sb > sa || (sb == sa && rb < ra)) ? 1 : 0;
    }
    B.cl_root[rank] = ra;
    B.cl_size[rank] = sa;
  }
  __syncthreads();
  int part = 0;
  const int C = (K + kT - 1) / kT, lo = min(K, t * C), hi = min(K, lo + C);
  for (int a = lo; a < hi; ++a) part += B.cl_size[a];
  int total;
  int off = block_excl_scan(part, si, &total);
  for (int a = lo; a < hi; ++a) { B.cl_off[a] = off; off += B.cl_size[a]; }
  if (t == 0) { c->n_clusters = K; c->n_seg = total; }
}

// ---- k_seg_members: colorSegmentation (:1032-1083) --------------------------------------------------
__global__ __launch_bounds__(kT) void k_seg_members(SegParams P, SegBufs B) {
  __shared__ int si[kT];
  __shared__ double sd[kT];
  const SegCtl* c = B.ctl;
  const int K = c->n_clusters, n = c->n_obj;
  for (int cl = blockIdx.x; cl < K; cl += gridDim.x) {
    const int root = B.cl_root[cl], off = B.cl_off[cl];
    block_compact(
        n, [&](int i) { return B.croot[i] == root; },
        [&](int i, int pos) {
          B.seg_local[off + pos] = i;
          B.seg_orig[off + pos] = B.obj[i];
          B.seg_label[off + pos] = cl + 1;
        },
        si);
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    const int sz = B.cl_size[cl];
    for (int k = threadIdx.x; k < sz; k += blockDim.x) {
      const double* p = B.aos + 3 * (size_t)B.seg_orig[off + k];
      for (int d = 0; d < 3; ++d) { lo[d] = fmin(lo[d], p[d]); hi[d] = fmax(hi[d], p[d]); }
    }
    double* bx = B.boxes + 6 * (size_t)cl;
    for (int d = 0; d < 3; ++d) {
      const double l = block_min(lo[d], sd), h = block_max(hi[d], sd);
      const double len = h - l;
      if (threadIdx.x == 0) { bx[d] = l + len / 2.0; bx[3 + d] = len < 0 ? -1 * len : len; }
    }
    __syncthreads();
  }
}

// ---- k_seg_ringcnt / k_seg_ringlist: extractEdgePoint's ring buckets (:1227-1237) ---------------------
__global__ __launch_bounds__(kT) void k_seg_ringcnt(SegParams P, SegBufs B) {
  __shared__ double sd[kT];
  const int b = blockIdx.x, n = B.ctl->n_seg;
  int c = 0;
  for (int s = threadIdx.x; s < n; s += kT) c += B.ring[B.seg_orig[s]] == b;
  const double tot = block_sum((double)c, sd);
  if (threadIdx.x == 0) B.ctl->ring_cnt[b] = (int)tot;
}

__global__ __launch_bounds__(kT) void k_seg_ringlist(SegParams P, SegBufs B) {
  __shared__ int si[kT];
  __shared__ int s_off;
  const int b = blockIdx.x, n = B.ctl->n_seg;
  if (threadIdx.x == 0) {
    int o = 0;
    for (int j = 0; j < b; ++j) o += B.ctl->ring_cnt[j];
    s_off = o;
    B.ctl->ring_off[b] = o;
  }
  __syncthreads();
  const int off = s_off;
  int* out = B.ring_list + off;
  block_compact(
      n, [&](int s) { return B.ring[B.seg_orig[s]] == b; }, [&](int s, int pos) { out[pos] = s; }, si);
}

// ---- k_seg_sector: curvature + extractFromSection (:1144-1210, :1248-1293) ---------------------------
__device__ inline const double* ring_pt(const SegBufs& B, int off, int id) {
  return B.aos + 3 * (size_t)B.seg_orig[B.ring_list[off + id]];
}

__global__ __launch_bounds__(256) void k_seg_sector(SegParams P, SegBufs B) {
  __shared__ int si[256];
  const int b = blockIdx.x / 6, j = blockIdx.x % 6, t = threadIdx.x;
  const SegCtl* c = B.ctl;
  const int m = c->ring_cnt[b], off = c->ring_off[b];
  int* cnt = B.sec_cnt + 2 * blockIdx.x;
  if (m < P.ring_min || c->n_seg == 0) {
    if (t == 0) { cnt[0] = 0; cnt[1] = 0; B.sec_base[blockIdx.x] = 0; }
    return;
  }
  const int tp = m - 10, L = tp / 6;
  const int s0 = L * j;
  const int s1 = j != 5 ? L * (j + 1) - 1 : tp - 1;   // [s0, s1): the entry at s1 is in no sector
  const int S = max(0, s1 - s0);
  double* cv = B.cv + off;
  int* sorted = B.sorted + off + s0;
  unsigned char* picked = B.picked + off;
  for (int e = s0 + t; e < s1; e += blockDim.x) {
    const int id = e + 5;
    double d[3];
    for (int k = 0; k < 3; ++k) {
      double s = ring_pt(B, off, id - 5)[k] + ring_pt(B, off, id - 4)[k];
      s = s + ring_pt(B, off, id - 3)[k];
      s = s + ring_pt(B, off, id - 2)[k];
      s = s + ring_pt(B, off, id - 1)[k];
      s = s - 10 * ring_pt(B, off, id)[k];
      s = s + ring_pt(B, off, id + 1)[k];
      s = s + ring_pt(B, off, id + 2)[k];
      s = s + ring_pt(B, off, id + 3)[k];
      s = s + ring_pt(B, off, id + 4)[k];
      s = s + ring_pt(B, off, id + 5)[k];
      d[k] = s;
    }
    cv[e] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    picked[e] = 0;
  }
  __syncthreads();
  // ascending (curvature, entry): rank by counting
  for (int e = s0 + t; e < s1; e += blockDim.x) {
    const double ce = cv[e];
    int rank = 0;
    for (int f = s0; f < s1; ++f) {
      const double cf = cv[f];
      rank += (cf < ce || (cf == ce && f < e)) ? 1 : 0;
    }
    sorted[rank] = e;
  }
  __syncthreads();
  __shared__ int s_edges;
  if (t == 0) {
    int* ed = B.edge_sec + kSegEdgePerSector * blockIdx.x;
    int picks = 0;
    for (int pos = S - 1; pos >= 0; --pos) {
      const int e = sorted[pos];
      if (picked[e]) continue;
      if (cv[e] <= 0.1) break;
      picks++;
      picked[e] = 1;
      if (picks > kSegEdgePerSector) break;
      const int id = e + 5;
      ed[picks - 1] = id;
      for (int k = 1; k <= 5; ++k) {
        const double *a = ring_pt(B, off, id + k), *q = ring_pt(B, off, id + k - 1);
        const double dx = a[0] - q[0], dy = a[1] - q[1], dz = a[2] - q[2];
        if (dx * dx + dy * dy + dz * dz > 0.05) break;
        const int f = id + k - 5;   // marks outside this sector hold nothing it reads
        if (f >= s0 && f < s1) picked[f] = 1;
      }
      for (int k = -1; k >= -5; --k) {
        const double *a = ring_pt(B, off, id + k), *q = ring_pt(B, off, id + k + 1);
        const double dx = a[0] - q[0], dy = a[1] - q[1], dz = a[2] - q[2];
        if (dx * dx + dy * dy + dz * dz > 0.05) break;
        const int f = id + k - 5;
        if (f >= s0 && f < s1) picked[f] = 1;
      }
    }
    s_edges = min(picks, kSegEdgePerSector);
  }
  __syncthreads();
  int* gen = B.genbuf + off + s0;
  const int ng = block_compact(
      S, [&](int p) { return !picked[sorted[p]]; }, [&](int p, int pos) { gen[pos] = sorted[p] + 5; }, si);
  if (t == 0) { cnt[0] = s_edges; cnt[1] = ng; B.sec_base[blockIdx.x] = off; }
}

// ---- k_seg_emit: edge / general lists in (ring, sector) order ---------------------------------------
__global__ __launch_bounds__(kT) void k_seg_emit(SegParams P, SegBufs B) {
  __shared__ int oe[kSegSectors + 1], og[kSegSectors + 1], sbase[kSegSectors], sgen[kSegSectors];
  __shared__ int si[kT];
  const int t = threadIdx.x;
  const bool live = B.ctl->n_seg > 0;
  int ce = 0, cg = 0;
  if (t < kSegSectors && live) { ce = B.sec_cnt[2 * t]; cg = B.sec_cnt[2 * t + 1]; }
  int te, tg;
  const int e0 = block_excl_scan(ce, si, &te);
  const int g0 = block_excl_scan(cg, si, &tg);
  if (t < kSegSectors) {
    oe[t] = e0; og[t] = g0;
    if (live) {
      const int b = t / 6, j = t % 6, m = B.ctl->ring_cnt[b], L = (m - 10) / 6;
      sbase[t] = B.sec_base[t];
      sgen[t] = L * j;
    }
  }
  if (t == 0) { oe[kSegSectors] = te; og[kSegSectors] = tg; }
  __syncthreads();
  for (int k = t; k < te; k += kT) {
    int lo = 0, hi = kSegSectors - 1;   // the sector holding output position k
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (oe[mid] <= k) lo = mid; else hi = mid - 1;
    }
    const int id = B.edge_sec[kSegEdgePerSector * lo + (k - oe[lo])];
    B.edge[k] = B.seg_orig[B.ring_list[sbase[lo] + id]];
  }
  for (int k = t; k < tg; k += kT) {
    int lo = 0, hi = kSegSectors - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (og[mid] <= k) lo = mid; else hi = mid - 1;
    }
    const int id = B.genbuf[sbase[lo] + sgen[lo] + (k - og[lo])];
    B.general[k] = B.seg_orig[B.ring_list[sbase[lo] + id]];
  }
  if (t == 0) { B.ctl->n_edge = te; B.ctl->n_general = tg; }
}

}  // namespace

int launch_segment(const SegParams& P, const SegBufs& B, hipStream_t s) {
  const int g = (P.n + 255) / 256 > 0 ? (P.n + 255) / 256 : 1;
  int launches = 0;
  k_seg_front<<<1, kT, 0, s>>>(P, B); ++launches;
  k_seg_ground<<<P.n_regions, kT, 0, s>>>(P, B); ++launches;
  k_seg_concat<<<1, kT, 0, s>>>(P, B); ++launches;
  k_seg_polar<<<g, 256, 0, s>>>(P, B); ++launches;
  k_seg_bounds<<<1, kT, 0, s>>>(P, B); ++launches;
  k_seg_voxel<<<g, 256, 0, s>>>(P, B); ++launches;
  k_seg_union<<<g, 256, 0, s>>>(P, B); ++launches;
  k_seg_flatten<<<g, 256, 0, s>>>(P, B); ++launches;
  k_seg_clusters<<<1, kT, 0, s>>>(P, B); ++launches;
  k_seg_members<<<256, kT, 0, s>>>(P, B); ++launches;
  k_seg_ringcnt<<<kSegRings, kT, 0, s>>>(P, B); ++launches;
  k_seg_ringlist<<<kSegRings, kT, 0, s>>>(P, B); ++launches;
  k_seg_sector<<<kSegSectors, 256, 0, s>>>(P, B); ++launches;
  k_seg_emit<<<1, kT, 0, s>>>(P, B); ++launches;
  return launches;
}

}  // namespace tl
