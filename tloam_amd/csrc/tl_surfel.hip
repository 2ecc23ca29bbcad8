// tl_surfel.hip -- the device side of the closed map's surfels (tl_api_surfel.hip): per occupied voxel of
// the closed map the second moments of the points that fell in it, and from them a normal and the three variances.
//
// Launches of a pass, the same four for any number of keyframes, spans and points (no host synchronisation between them):
//   k_surfel_clear   grid x 256   zeroes the thirteen sums, the keyframes' flags and the control words
//   k_surfel_flag    grid x 256   per point: its span from its global index, transform, quantise; a finite point beyond the grid
//                                 raises its keyframe's flag (a plain store of 1: every writer writes the same value)
//   k_surfel_accum   grid x 256   per point of an unflagged keyframe: the same, the voxel's id from the closed map's slot table
//                                 (id_table_find; none: an orphan), then the thirteen integers; runs of equal ids among a wave's
//                                 consecutive lanes are summed by shuffle scans and the run's tail does the thirteen int64 atomic
//                                 adds (a wave without such a run, and the plain form, add per point: the same bits)
//   k_surfel_solve   grid x 256   per voxel: mean, covariance, eig3_sym, orientation, scale; the solved voxels counted by ballot,
//                                 one atomic per wave
// An extension of the closed map (tl_api_extend.hip) launches k_surfel_accum over the new keyframes' spans
// without the clear, then
//   k_surfel_solve_staged  T/256 x 256   per slot of the extension's staging table: the voxel the slot added to solved again
//                                 (surfel_solve_voxel, k_surfel_solve's body); the voxels that became solved counted
// The box read is k_surfel_box: the box read's one body (tl_voxel.hpp: voxel_box_body) with the surfel gate (surfel_gate).
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

// point g (< W.in.n): its keyframe, its pose, the point under it, and where that falls in the grid (key and q when inside)
__device__ __forceinline__ VmapCell surfel_point(const SurfelWork& W, long long g, const int s_span[2], int* kf, const double** P,
                                                 double E[3], unsigned long long* key, unsigned q[3]) {
  span_point(W.in, g, s_span[0], s_span[1], kf, P, E);
  return vmap_quantise(E, W.grid.origin, W.grid.voxel, key, q);
}

__global__ __launch_bounds__(256) void k_surfel_clear(SurfelWork W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t t = i; t < (size_t)W.grid.nv * kSurfelSums; t += stride) W.sums[t] = 0ull;
  for (size_t t = i; t < (size_t)W.in.nkf; t += stride) W.kf_over[t] = 0;
  if (i < 8) W.ctl[i] = 0ull;
}

__global__ __launch_bounds__(256) void k_surfel_flag(SurfelWork W) {
  __shared__ int s_span[2];
  block_spans(W.in, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= W.in.n) return;
  int kf;
  const double* P;
  double E[3];
  unsigned long long key;
  unsigned q[3];
  if (surfel_point(W, g, s_span, &kf, &P, E, &key, q) == kVmapBeyond) W.kf_over[kf] = 1;
}

template <bool kRuns>
__global__ __launch_bounds__(256) void k_surfel_accum(SurfelWork W) {
  __shared__ int s_span[2];
  block_spans(W.in, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool ok = false, orphan = false;
  int id = -1;
  unsigned r[3] = {0u, 0u, 0u};
  long long w[3] = {0, 0, 0};
  if (g < W.in.n) {
    int kf;
    const double* P;
    double E[3];
    unsigned long long key;
    unsigned q[3];
    if (surfel_point(W, g, s_span, &kf, &P, E, &key, q) == kVmapInside && W.kf_over[kf] == 0) {
      id = id_table_find(W.grid.map.ptab, W.grid.map.pmask, W.grid.map.pkey, key);
      ok = id >= 0;
      orphan = !ok;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        r[a] = q[a] >> 8;
        const double t = ((P[12 + a] - E[a]) / W.grid.voxel) * 256.0;
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

// voxel id (< W.grid.nv) solved from its thirteen sums: its normal and variances written (zeros below min_points); true when solved
__device__ __forceinline__ bool surfel_solve_voxel(const SurfelWork& W, long long id) {
  bool solved = false;
  {
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
      const double sc = W.grid.voxel * (1.0 / 65536.0);
      const double s2 = sc * sc;
      ev[0] = lam[0] * s2; ev[1] = lam[1] * s2; ev[2] = lam[2] * s2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      W.normal[3 * id + a] = n[a];
      W.eval[3 * id + a] = ev[a];
    }
  }
  return solved;
}

__global__ __launch_bounds__(256) void k_surfel_solve(SurfelWork W) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool solved = id < W.grid.nv && surfel_solve_voxel(W, id);
  const unsigned long long bal = __ballot(solved);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&W.ctl[2], (unsigned long long)__popcll(bal));
}

// per slot of a staging table (the closed map's extension): the voxel the slot added to is solved again; one that had fewer than
// min_points before the slot's N was added and is solved now is counted
__global__ __launch_bounds__(256) void k_surfel_solve_staged(SurfelWork W, StagedVoxels V) {
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool newly = false;
  if (s <= V.fmask && V.fkey[s] != kFree) {
    const long long id = V.fid[s];
    if (id >= 0 && id < W.grid.nv) {
      const long long before = ((const long long*)W.sums)[(size_t)id * kSurfelSums] - (long long)V.fsum[s];
      newly = surfel_solve_voxel(W, id) && before < (long long)W.min_points;
    }
  }
  const unsigned long long bal = __ballot(newly);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&W.ctl[2], (unsigned long long)__popcll(bal));
}

// the box read (the box only when A.boxed) of the voxels whose surfel passes the gate; the normals and the variances beside the
// centroids, and Ns where the plain read has N
struct BoxSurfel {
  const SurfelReadArgs& A;
  __device__ __forceinline__ bool keep(size_t id, long long, const double*) const {
    const double ev[3] = {A.eval[3 * id], A.eval[3 * id + 1], A.eval[3 * id + 2]};
    return surfel_gate((long long)A.sums[id * kSurfelSums], ev, A.min_points, A.max_sigma2, A.min_planarity);
  }
  __device__ __forceinline__ long long emit(size_t id, size_t p, long long) const {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (A.out_nrm) A.out_nrm[3 * p + a] = A.normal[3 * id + a];
      if (A.out_ev) A.out_ev[3 * p + a] = A.eval[3 * id + a];
    }
    return (long long)A.sums[id * kSurfelSums];
  }
};
__global__ __launch_bounds__(256) void k_surfel_box(SurfelReadArgs A, int nblocks) {
  voxel_box_body(A.rows, A.boxed != 0, nblocks, BoxSurfel{A});
}

}  // namespace

int launch_surfels(const SurfelWork& W, hipStream_t s) {
  const size_t nv = (size_t)std::max<long long>(W.grid.nv, 1);   // (nothing still launches)
  const unsigned pt_blocks = blocks_of((size_t)std::max<long long>(W.in.n, 1));
  hipLaunchKernelGGL(k_surfel_clear, dim3(std::min(blocks_of(nv * kSurfelSums), 2048u)), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_surfel_flag, dim3(pt_blocks), dim3(256), 0, s, W);
  launch_surfel_accum(W, s);
  hipLaunchKernelGGL(k_surfel_solve, dim3(blocks_of(nv)), dim3(256), 0, s, W);
  return 4;
}

int launch_surfel_accum(const SurfelWork& W, hipStream_t s) {
  const unsigned pt_blocks = blocks_of((size_t)std::max<long long>(W.in.n, 1));
  if (W.runs) hipLaunchKernelGGL(k_surfel_accum<true>, dim3(pt_blocks), dim3(256), 0, s, W);
  else hipLaunchKernelGGL(k_surfel_accum<false>, dim3(pt_blocks), dim3(256), 0, s, W);
  return 1;
}

int launch_surfel_solve_staged(const SurfelWork& W, const StagedVoxels& V, hipStream_t s) {
  hipLaunchKernelGGL(k_surfel_solve_staged, dim3(blocks_of((size_t)V.fmask + 1)), dim3(256), 0, s, W, V);
  return 1;
}

void launch_surfel_solve(const SurfelWork& W, hipStream_t s) {
  hipLaunchKernelGGL(k_surfel_solve, dim3(blocks_of((size_t)std::max<long long>(W.grid.nv, 1))), dim3(256), 0, s, W);
}

void launch_surfel_read(const SurfelReadArgs& A, hipStream_t s) {
  if (A.rows.count == 0) return;
  const int nb = (int)blocks_of(A.rows.count);
  hipLaunchKernelGGL(k_surfel_box, dim3(nb), dim3(256), 0, s, A, nb);
}

}  // namespace tl
