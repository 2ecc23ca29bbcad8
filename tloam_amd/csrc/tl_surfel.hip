// tl_surfel.hip -- the device side of the closed map's surfels (tl_api_surfel.hip): per occupied voxel of
// the closed map the second moments of the points that fell in it, and from them a normal and the three variances.
//
// Launches of a pass, the same four for any number of keyframes, spans and points (no host synchronisation between them):
//   k_surfel_clear   grid x 256   zeroes the thirteen sums, the keyframes' flags and the control words
//   k_surfel_flag    grid x 256   per point: its span from its global index, transform, quantise; a finite point beyond the grid
//                                 raises its keyframe's flag (as k_cmap_flag: a plain store of 1)
//   k_surfel_accum   grid x 256   per point of an unflagged keyframe: the same, the voxel's id from the closed map's slot table
//                                 (read only; none: an orphan), then the thirteen integers; runs of equal ids among a wave's
//                                 consecutive lanes are summed by shuffle scans and the run's tail does the thirteen int64 atomic
//                                 adds (a wave without such a run, and the plain form, add per point: the same bits)
//   k_surfel_solve   grid x 256   per voxel: mean, covariance, eig3_sym, orientation, scale; the solved voxels counted by ballot,
//                                 one atomic per wave
// The box read is k_surfel_box: k_carve_box's selection, order and compaction with the surfel gate.
//
// Compiled with -ffp-contract=off.  The arithmetic (tests/closed_map_surfel_np.py restates it), per point of keyframe k and axis a:
//   E = map_transform_point(P_k, p),  O_a = P_k[12 + a],  (i, q) = vmap_quantise(E),  r_a = q_a >> 8  (2^-16 of a voxel)
//   w_a = (int64) floor(min(max(((O_a - E_a) / v) * 256.0, -2^30), 2^30) + 0.5)
//   Ns += 1,  R_a += r_a,  S_ab += r_a * r_b  (xx xy xz yy yz zz),  W_a += w_a
// and per voxel with Ns >= min_points:
//   m_a = (double) R_a / (double) Ns,  c_ab = (double) S_ab / (double) Ns - m_a * m_b,  (lambda, V) = eig3_sym(c),  n = V[:, 0]
//   d = (n_x * (double) W_x + n_y * (double) W_y) + n_z * (double) W_z;  d < 0: n = -n
//   sc = v * 2^-16,  ev_a = lambda_a * (sc * sc)
#include <algorithm>

#include "tl_knn.hpp"
#include "tl_voxel.hpp"

namespace tl {
namespace {

constexpr double kSurfelWClamp = 1073741824.0;   // 2^30

// the id of the closed map's voxel `key`, -1 when it has none
__device__ __forceinline__ int surfel_find(const SurfelWork& W, unsigned long long key) {
  for (unsigned long long t = mix64(key) & W.pmask;; t = (t + 1) & W.pmask) {
    const int id = W.ptab[t];
    if (id < 0) return -1;
    if (W.pkey[id] == key) return id;
  }
}

// point g (< W.n): its keyframe, its pose, the point under it, and where that falls in the grid (key and q when inside)
__device__ __forceinline__ VmapCell surfel_point(const SurfelWork& W, long long g, int s_lo, int s_hi, int* kf, const double** P,
                                                 double E[3], unsigned long long* key, unsigned q[3]) {
  const CmapSpan S = W.span[span_of(W.span, s_lo, s_hi, g)];
  const double* x = W.arena + S.off + 3 * (g - S.start);
  *kf = S.kf;
  *P = W.pose + 16 * (size_t)S.kf;
  map_transform_point(*P, x[0], x[1], x[2], &E[0], &E[1], &E[2]);
  return vmap_quantise(E, W.origin, W.voxel, key, q);
}

__global__ __launch_bounds__(256) void k_surfel_clear(SurfelWork W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t t = i; t < (size_t)W.nv * kSurfelSums; t += stride) W.sums[t] = 0ull;
  for (size_t t = i; t < (size_t)W.nkf; t += stride) W.kf_over[t] = 0;
  if (i < 8) W.ctl[i] = 0ull;
}

__global__ __launch_bounds__(256) void k_surfel_flag(SurfelWork W) {
  __shared__ int s_span[2];
  block_spans(W, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= W.n) return;
  int kf;
  const double* P;
  double E[3];
  unsigned long long key;
  unsigned q[3];
  if (surfel_point(W, g, s_span[0], s_span[1], &kf, &P, E, &key, q) == kVmapBeyond) W.kf_over[kf] = 1;
}

// inclusive prefix sum of `v` over the wave's lanes
template <typename T>
__device__ __forceinline__ T wave_scan(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// the sum of `v` over lanes [head_lane, this lane] from its inclusive prefix sum
template <typename T>
__device__ __forceinline__ T run_sum(T incl, int head_lane) {
  const T below = __shfl(incl, head_lane > 0 ? head_lane - 1 : 0, 64);
  return incl - (head_lane > 0 ? below : (T)0);
}

template <bool kRuns>
__global__ __launch_bounds__(256) void k_surfel_accum(SurfelWork W) {
  __shared__ int s_span[2];
  block_spans(W, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool ok = false, orphan = false;
  int id = -1;
  unsigned r[3] = {0u, 0u, 0u};
  long long w[3] = {0, 0, 0};
  if (g < W.n) {
    int kf;
    const double* P;
    double E[3];
    unsigned long long key;
    unsigned q[3];
    if (surfel_point(W, g, s_span[0], s_span[1], &kf, &P, E, &key, q) == kVmapInside && W.kf_over[kf] == 0) {
      id = surfel_find(W, key);
      ok = id >= 0;
      orphan = !ok;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        r[a] = q[a] >> 8;
        const double t = ((P[12 + a] - E[a]) / W.voxel) * 256.0;
        w[a] = (long long)floor(fmin(fmax(t, -kSurfelWClamp), kSurfelWClamp) + 0.5);
      }
    }
  }
  // the point's thirteen: the count and the first moments fit 32 bits over a wave (64 * 2^16), the others do not
  unsigned lo[4] = {ok ? 1u : 0u, r[0], r[1], r[2]};
  unsigned long long hi[9] = {(unsigned long long)r[0] * r[0], (unsigned long long)r[0] * r[1], (unsigned long long)r[0] * r[2],
                              (unsigned long long)r[1] * r[1], (unsigned long long)r[1] * r[2], (unsigned long long)r[2] * r[2],
                              (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2]};
  const unsigned long long okb = __ballot(ok);
  bool add = ok;
  if (kRuns) {
    const int idprev = __shfl_up(id, 1, 64), idnext = __shfl_down(id, 1, 64);
    const bool ok_prev = lane > 0 && ((okb >> (lane - 1)) & 1ull);
    const bool ok_next = lane < 63 && ((okb >> (lane + 1)) & 1ull);
    const bool head = ok && !(ok_prev && idprev == id);
    const bool tail = ok && !(ok_next && idnext == id);
    const unsigned long long heads = __ballot(head);
    if (heads != okb) {   // (wave-uniform) some run is longer than one point
      const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
      const int hl = (heads & upto) ? 63 - __clzll(heads & upto) : 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) lo[k] = run_sum(wave_scan(lo[k], lane), hl);
#pragma unroll
      for (int k = 0; k < 9; ++k) hi[k] = run_sum(wave_scan(hi[k], lane), hl);
      add = tail;
    }
  }
  if (add) {
    unsigned long long* s = W.sums + (size_t)id * kSurfelSums;
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(&s[k], (unsigned long long)lo[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) atomicAdd(&s[4 + k], hi[k]);
  }
  const unsigned long long orb = __ballot(orphan);
  if (lane == 0) {
    if (okb) atomicAdd(&W.ctl[0], (unsigned long long)__popcll(okb));
    if (orb) atomicAdd(&W.ctl[1], (unsigned long long)__popcll(orb));
  }
}

__global__ __launch_bounds__(256) void k_surfel_solve(SurfelWork W) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  bool solved = false;
  if (id < W.nv) {
    const long long* s = (const long long*)W.sums + (size_t)id * kSurfelSums;
    const long long Ns = s[0];
    double n[3] = {0.0, 0.0, 0.0}, ev[3] = {0.0, 0.0, 0.0};
    if (Ns >= (long long)W.min_points) {
      solved = true;
      const double dN = (double)Ns;
      const double m[3] = {(double)s[1] / dN, (double)s[2] / dN, (double)s[3] / dN};
      Sym3 M;
      M.a[0][0] = (double)s[4] / dN - m[0] * m[0];
      M.a[0][1] = M.a[1][0] = (double)s[5] / dN - m[0] * m[1];
      M.a[0][2] = M.a[2][0] = (double)s[6] / dN - m[0] * m[2];
      M.a[1][1] = (double)s[7] / dN - m[1] * m[1];
      M.a[1][2] = M.a[2][1] = (double)s[8] / dN - m[1] * m[2];
      M.a[2][2] = (double)s[9] / dN - m[2] * m[2];
      double lam[3];
      eig3_sym(M, lam);
      n[0] = M.v[0][0]; n[1] = M.v[1][0]; n[2] = M.v[2][0];
      const double d = (n[0] * (double)s[10] + n[1] * (double)s[11]) + n[2] * (double)s[12];
      if (d < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
      const double sc = W.voxel * (1.0 / 65536.0);
      const double s2 = sc * sc;
      ev[0] = lam[0] * s2; ev[1] = lam[1] * s2; ev[2] = lam[2] * s2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      W.normal[3 * id + a] = n[a];
      W.eval[3 * id + a] = ev[a];
    }
  }
  const unsigned long long bal = __ballot(solved);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&W.ctl[2], (unsigned long long)__popcll(bal));
}

// the voxels of k_vmap_box's selection (the box only when A.boxed) whose surfel passes the gate, compacted in id order
__global__ __launch_bounds__(256) void k_surfel_box(SurfelReadArgs A, int nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const VmapReadArgs& R = A.rows;
  const int tid = threadIdx.x;
  const int bid = block_ticket(&R.ctl[0], &s_bid);
  const size_t id = (size_t)bid * 256 + tid;
  double c[3] = {0.0, 0.0, 0.0}, nr[3] = {0.0, 0.0, 0.0}, ev[3] = {0.0, 0.0, 0.0};
  long long ns = 0;
  bool sel = false;
  if (id < R.count) {
    const unsigned long long key = R.pkey[id];
    const long long Q[3] = {R.pqx[id], R.pqy[id], R.pqz[id]};
    const long long n = R.pn[id];
    ns = (long long)A.sums[id * kSurfelSums];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = centroid(R.origin[a], R.voxel, key_axis(key, a), Q[a], n);
      nr[a] = A.normal[3 * id + a];
      ev[a] = A.eval[3 * id + a];
    }
    sel = n >= R.min_count;
    if (A.boxed) {
#pragma unroll
      for (int a = 0; a < 3; ++a) sel = sel && c[a] >= R.lo[a] && c[a] <= R.hi[a];
    }
    sel = sel && ns >= (long long)A.min_points && ev[2] > 0.0 && ev[0] <= A.max_sigma2 && (ev[1] - ev[0]) >= A.min_planarity * ev[2];
  }
  int pos, total;
  block_flag_scan(sel, s_wave, &pos, &total);
  if (tid == 0) s_prefix = lookback_prefix(R.look, bid, (unsigned long long)total, LookFaultDevice{&R.ctl[1]});
  __syncthreads();
  if (sel) {
    const size_t p = (size_t)(s_prefix + pos);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (R.out_c) R.out_c[3 * p + a] = c[a];
      if (A.out_nrm) A.out_nrm[3 * p + a] = nr[a];
      if (A.out_ev) A.out_ev[3 * p + a] = ev[a];
    }
    if (R.out_n) R.out_n[p] = ns;
  }
  if (bid == nblocks - 1 && tid == 0) R.ctl[2] = s_prefix + total;
}

inline unsigned blocks_of(long long n) { return (unsigned)std::max<long long>((n + 255) / 256, 1); }   // (nothing still launches)

}  // namespace

int launch_surfels(const SurfelWork& W, hipStream_t s) {
  hipLaunchKernelGGL(k_surfel_clear, dim3(std::min(blocks_of(W.nv * kSurfelSums), 2048u)), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_surfel_flag, dim3(blocks_of(W.n)), dim3(256), 0, s, W);
  if (W.runs) hipLaunchKernelGGL(k_surfel_accum<true>, dim3(blocks_of(W.n)), dim3(256), 0, s, W);
  else hipLaunchKernelGGL(k_surfel_accum<false>, dim3(blocks_of(W.n)), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_surfel_solve, dim3(blocks_of(W.nv)), dim3(256), 0, s, W);
  return 4;
}

void launch_surfel_read(const SurfelReadArgs& A, hipStream_t s) {
  if (A.rows.count == 0) return;
  const int nb = (int)blocks_of((long long)A.rows.count);
  hipLaunchKernelGGL(k_surfel_box, dim3(nb), dim3(256), 0, s, A, nb);
}

}  // namespace tl
