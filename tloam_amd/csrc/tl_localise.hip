// tl_localise.hip -- the device side of the localisation of a scan in the closed map (tl_api_localise.hip):
// point-to-plane Gauss-Newton on the surfels.
//
// Launches (no host synchronisation between them; nothing of the closed map, the carve or the surfels is written):
//   k_loc_prepare   grid x 256   per voxel one 64-byte record {c, n, eligible}: a probe hit then costs one cache line
//   k_loc_sweep     grid x 256   per point: transform, quantise, 27 read-only probes of the closed map's slot table, the nearest
//                                eligible centroid, residual, truncation; the 28 terms and the two counts summed over the wave
//                                by shuffles and over the block's four waves through LDS; one partial row per block
//   k_loc_step      1 x 64       the partial rows added in block order, the degeneracy tests, the 6 x 6 Cholesky, the pose
//                                update, the log record and the `done` word
// A sweep or a step that finds `done` set returns on entry (a wave-uniform branch), so a call is the same launches for every
// input.  No block waits on another block.  No floating-point atomics: the order of every sum is fixed by the point index
// (lane, wave, block), so two calls give the same bits.
//
// Compiled with -ffp-contract=off.  The arithmetic (tests/closed_map_localise_np.py restates it), per point p and matrix M:
//   E = map_transform_point(M, p),  (i, q) = vmap_quantise(E);  for dz, dy, dx in -1 .. 1 (dx innermost) the voxel of cell
//   i + (dx, dy, dz) when it has one and its record is eligible: d = E - c, D = (d_x*d_x + d_y*d_y) + d_z*d_z, kept under D < best
//   r = (n_x*d_x + n_y*d_y) + n_z*d_z,  used: fabs(r) <= tau
//   J = [n, E x n] (tl_se3.hpp::cross),  terms: J_a * J_b (a <= b, by rows), J_a * r, 0.5 * (r * r)
// and per iteration k (k_loc_step, one lane):
//   tau_k = max(min_residual, pw_k), pw_0 = max_residual0, pw_{k+1} = pw_k * shrink
//   H = L L^T by rows, every inner sum left to right: s = H_kk - sum_j L_kj^2, degenerate unless s > min_pivot_ratio * H_kk,
//   L_kk = sqrt(s), L_ik = (H_ik - sum_j L_ij L_kj) / L_kk;  L y = -g,  L^T d = y
//   T <- compose(se3_exp(d), T),  M = pose_to_matrix(T)
//   converged: sqrt((d0*d0 + d1*d1) + d2*d2) < step_tol_t && sqrt((d3*d3 + d4*d4) + d5*d5) < step_tol_r
#include "tl_voxel.hpp"

namespace tl {
namespace {

// the id of the closed map's voxel `key`, -1 when it has none (tl_surfel.hip's surfel_find)
__device__ __forceinline__ int loc_find(const LocSweepArgs& W, unsigned long long key) {
  for (unsigned long long t = mix64(key) & W.pmask;; t = (t + 1) & W.pmask) {
    const int id = W.ptab[t];
    if (id < 0) return -1;
    if (W.pkey[id] == key) return id;
  }
}

__global__ __launch_bounds__(256) void k_loc_prepare(LocPrepArgs A) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= A.nv) return;
  const unsigned long long key = A.pkey[id];
  const long long Q[3] = {A.pqx[id], A.pqy[id], A.pqz[id]};
  const long long n = A.pn[id];
  const long long ns = (long long)A.sums[id * kSurfelSums];
  LocRecord R;
  double ev[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    R.c[a] = centroid(A.origin[a], A.voxel, key_axis(key, a), Q[a], n);
    R.n[a] = A.normal[3 * id + a];
    ev[a] = A.eval[3 * id + a];
  }
  R.eligible = ns >= (long long)A.min_points && ev[2] > 0.0 && ev[0] <= A.max_sigma2 && (ev[1] - ev[0]) >= A.min_planarity * ev[2];
  R.pad[0] = R.pad[1] = R.pad[2] = 0;
  A.rec[id] = R;
}

__global__ __launch_bounds__(256) void k_loc_sweep(LocSweepArgs W) {
  __shared__ double s_row[4][kLocRow];
  if (W.st->done) return;   // (the same word for every thread of the grid)
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double t[kLocTerms + 2];
#pragma unroll
  for (int k = 0; k < kLocTerms + 2; ++k) t[k] = 0.0;
  if (g < W.n) {
    const double* M = W.st->M;
    const double tau = W.st->tau;
    double E[3];
    map_transform_point(M, W.pts[3 * g], W.pts[3 * g + 1], W.pts[3 * g + 2], &E[0], &E[1], &E[2]);
    unsigned long long key;
    unsigned q[3];
    int best = -1;
    double bd[3] = {0.0, 0.0, 0.0}, bn[3] = {0.0, 0.0, 0.0};
    if (W.nv > 0 && vmap_quantise(E, W.origin, W.voxel, &key, q) == kVmapInside) {
      const long long i0 = key_axis(key, 0), i1 = key_axis(key, 1), i2 = key_axis(key, 2);
      const long long lim = 1ll << kVmapBits;
      double bD = HUGE_VAL;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const long long c0 = i0 + dx, c1 = i1 + dy, c2 = i2 + dz;
            if (c0 <= -lim || c0 >= lim || c1 <= -lim || c1 >= lim || c2 <= -lim || c2 >= lim) continue;   // beyond the grid: no voxel
            const unsigned long long ck = (unsigned long long)(c0 + lim) | ((unsigned long long)(c1 + lim) << 21) |
                                          ((unsigned long long)(c2 + lim) << 42);
            const int id = loc_find(W, ck);
            if (id < 0) continue;
            const LocRecord* R = W.rec + id;
            if (!R->eligible) continue;
            const double d0 = E[0] - R->c[0], d1 = E[1] - R->c[1], d2 = E[2] - R->c[2];
            const double D = (d0 * d0 + d1 * d1) + d2 * d2;
            if (D < bD) {
              best = id; bD = D;
              bd[0] = d0; bd[1] = d1; bd[2] = d2;
              bn[0] = R->n[0]; bn[1] = R->n[1]; bn[2] = R->n[2];
            }
          }
    }
    double r = 0.0;
    if (best >= 0) {
      r = (bn[0] * bd[0] + bn[1] * bd[1]) + bn[2] * bd[2];
      t[kLocTerms] = 1.0;
      if (fabs(r) <= tau) {
        const Vec3 x = cross(Vec3{E[0], E[1], E[2]}, Vec3{bn[0], bn[1], bn[2]});
        const double J[6] = {bn[0], bn[1], bn[2], x.x, x.y, x.z};
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) t[k++] = J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) t[21 + a] = J[a] * r;
        t[27] = 0.5 * (r * r);
        t[kLocTerms + 1] = 1.0;
      }
    }
    if (W.ids) W.ids[g] = best;
    if (W.res) W.res[g] = r;
  }
  // over the wave: a butterfly, the same order in every launch; then the four waves in order
#pragma unroll
  for (int k = 0; k < kLocTerms + 2; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t[k] += __shfl_xor(t[k], off, 64);
    if (lane == 0) s_row[wave][k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x < kLocRow) {
    const int k = threadIdx.x;
    double s = 0.0;
    if (k < kLocTerms + 2) s = ((s_row[0][k] + s_row[1][k]) + s_row[2][k]) + s_row[3][k];
    W.partial[(size_t)blockIdx.x * kLocRow + k] = s;
  }
}

// H d = -g by Cholesky; false: a pivot is not > ratio * H_kk
__device__ bool loc_solve6(const double* sums, double ratio, double d[6]) {
  double H[6][6], L[6][6];
  int t = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) { H[a][b] = H[b][a] = sums[t++]; }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double s = H[k][k];
#pragma unroll
    for (int j = 0; j < k; ++j) s = s - L[k][j] * L[k][j];
    if (!(s > ratio * H[k][k])) return false;
    L[k][k] = sqrt(s);
#pragma unroll
    for (int i = k + 1; i < 6; ++i) {
      double u = H[i][k];
#pragma unroll
      for (int j = 0; j < k; ++j) u = u - L[i][j] * L[k][j];
      L[i][k] = u / L[k][k];
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double u = -sums[21 + i];
#pragma unroll
    for (int j = 0; j < i; ++j) u = u - L[i][j] * y[j];
    y[i] = u / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double u = y[i];
#pragma unroll
    for (int j = i + 1; j < 6; ++j) u = u - L[j][i] * d[j];
    d[i] = u / L[i][i];
  }
  return true;
}

__global__ __launch_bounds__(64) void k_loc_step(LocStepArgs A) {
  __shared__ double s_sum[kLocRow];
  LocState* S = A.st;
  if (S->done) return;
  const int lane = threadIdx.x;
  if (lane < kLocRow) {   // a lane per column, the rows in block order
    const double* col = A.partial + lane;
    double s = 0.0;
    int b = 0;
    for (; b + 32 <= A.nblocks; b += 32) {   // 32 rows fetched ahead, added in order: the loads overlap, the order stays
      double v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = col[(size_t)(b + u) * kLocRow];
#pragma unroll
      for (int u = 0; u < 32; ++u) s += v[u];
    }
    for (; b < A.nblocks; ++b) s += col[(size_t)b * kLocRow];
    s_sum[lane] = s;
    S->sums[lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  if (A.k < 0) {   // a linearise: the sums are the result
    S->done = 1;
    return;
  }
  const long long matched = (long long)s_sum[kLocTerms], used = (long long)s_sum[kLocTerms + 1];
  LocLog R;
  for (int i = 0; i < 16; ++i) R.pose[i] = S->M[i];
  R.tau = S->tau;
  R.cost = s_sum[27];
  R.matched = matched;
  R.used = used;
  double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = used >= (long long)A.min_matches;
  for (int i = 0; i < kLocTerms; ++i) ok = ok && __builtin_isfinite(s_sum[i]);
  ok = ok && loc_solve6(s_sum, A.min_pivot_ratio, d);
  S->iterations = A.k + 1;
  if (!ok) {
    for (int i = 0; i < 6; ++i) R.d[i] = 0.0;
    A.log[A.k] = R;
    S->status = TLOAM_LOCALISE_DEGENERATE;
    S->done = 1;
    return;
  }
  for (int i = 0; i < 6; ++i) R.d[i] = d[i];
  A.log[A.k] = R;
  const Pose T = compose(se3_exp(d), S->T);
  S->T = T;
  double M[16];
  pose_to_matrix(T, M);
  for (int i = 0; i < 16; ++i) S->M[i] = M[i];
  const double pw = S->pw * A.shrink;
  S->pw = pw;
  S->tau = fmax(A.min_residual, pw);
  const bool conv = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < A.step_tol_t &&
                    sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]) < A.step_tol_r;
  if (conv) {
    S->status = TLOAM_LOCALISE_CONVERGED;
    S->done = 1;
  } else if (A.k + 1 >= A.max_iterations) {
    S->status = TLOAM_LOCALISE_MAX_ITERATIONS;
    S->done = 1;
  }
}

}  // namespace

void launch_loc_prepare(const LocPrepArgs& A, hipStream_t s) {
  if (A.nv <= 0) return;
  hipLaunchKernelGGL(k_loc_prepare, dim3(loc_blocks(A.nv)), dim3(256), 0, s, A);
}

void launch_loc_sweep(const LocSweepArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_loc_sweep, dim3(loc_blocks(A.n)), dim3(256), 0, s, A);
}

void launch_loc_step(const LocStepArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_loc_step, dim3(1), dim3(64), 0, s, A);
}

}  // namespace tl
