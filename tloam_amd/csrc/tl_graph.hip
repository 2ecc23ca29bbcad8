// tl_graph.hip -- the device side of the keyframe pose-graph optimisation (tl_api_graph.hip).
//
// Launch:
//   k_graph_step   1 x 512    per Gauss-Newton iteration: linearise every edge at P (residual, A = rigid_inverse(P_j) * P_i, its two
//                             terms of the right-hand side), the chain's Q_k = rigid_inverse(P_0) * P_k, then the preconditioned
//                             conjugate gradients to their end, the step P_n * exp(d_n) into Pn, the cost at Pn, one record
// The work of a conjugate-gradient iteration is a few thousand 6-vectors: what it costs is the hand-over between its phases.  So
// the whole solve is ONE workgroup whose phases are separated by workgroup barriers: no launch boundary, no host wait and no
// cross-block spin inside it.  Vectors live in global memory (L2); a thread owns `chunk` consecutive nodes and a stride of edges.
// Per iteration: the edges' terms q = W (p_j - Ad(A) p_i) and -Ad(A)^T q | barrier | every node gathers its terms in edge order
// (the table the host built), p . Ap | x, r, and the chain preconditioner as a suffix and a prefix sum over the nodes (a thread's
// chunk serially, the chunks by a wave scan, the waves in order) | r . z, p.  Every sum has a fixed order and there are no atomics:
// two runs give the same bits.
//   k_graph_reweight 1 x 512  robust mode only, once per outer iteration: a thread strides the loop edges; an
//                             edge's r = sum_a w0_a e_a^2 at P (edge_residual's expression, base weights), its scale by the rule at
//                             mu, the solver's weights s * w0; max r, the three counts and sum s r in block_max / block_sum order
// Compiled with -ffp-contract=off, like the other stages whose numpy restatement (tests/graph_np.py) states the arithmetic.
#include "tl_common.hpp"

namespace tl {
namespace {

constexpr int kT = kGraphThreads;
constexpr int kWaves = kT / 64;

__device__ __forceinline__ Pose pose_inverse(const Pose& T) {
  Pose I;
  I.qw = T.qw; I.qx = -T.qx; I.qy = -T.qy; I.qz = -T.qz;
  const Vec3 t = rotate(I, Vec3{T.tx, T.ty, T.tz});
  I.tx = -t.x; I.ty = -t.y; I.tz = -t.z;
  return I;
}
__device__ __forceinline__ Vec3 mul(const double R[9], Vec3 v) {
  return {(R[0] * v.x + R[1] * v.y) + R[2] * v.z, (R[3] * v.x + R[4] * v.y) + R[5] * v.z, (R[6] * v.x + R[7] * v.y) + R[8] * v.z};
}
__device__ __forceinline__ Vec3 mul_t(const double R[9], Vec3 v) {
  return {(R[0] * v.x + R[3] * v.y) + R[6] * v.z, (R[1] * v.x + R[4] * v.y) + R[7] * v.z, (R[2] * v.x + R[5] * v.y) + R[8] * v.z};
}
// y = Ad(T) x, Ad(T) = [[R, hat(t) R], [0, R]]
__device__ __forceinline__ void ad(const Rt& T, const double x[6], double y[6]) {
  const Vec3 ru = mul(T.r, Vec3{x[0], x[1], x[2]}), ro = mul(T.r, Vec3{x[3], x[4], x[5]});
  const Vec3 c = cross(Vec3{T.t[0], T.t[1], T.t[2]}, ro);
  y[0] = ru.x + c.x; y[1] = ru.y + c.y; y[2] = ru.z + c.z;
  y[3] = ro.x; y[4] = ro.y; y[5] = ro.z;
}
// y = Ad(T)^T x = (R^T a, R^T (b - t x a))
__device__ __forceinline__ void ad_t(const Rt& T, const double x[6], double y[6]) {
  const Vec3 a{x[0], x[1], x[2]}, b{x[3], x[4], x[5]};
  const Vec3 ra = mul_t(T.r, a), rb = mul_t(T.r, b - cross(Vec3{T.t[0], T.t[1], T.t[2]}, a));
  y[0] = ra.x; y[1] = ra.y; y[2] = ra.z;
  y[3] = rb.x; y[4] = rb.y; y[5] = rb.z;
}

// the workgroup's sum: lanes by a shuffle tree, waves in order; s_w is this call site's own row (a barrier inside)
__device__ __forceinline__ double block_sum(double v, double* s_w) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t = t + s_w[w];
  return t;
}
__device__ __forceinline__ double block_max(double v, double* s_w) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t = fmax(t, s_w[w]);
  return t;
}

// exclusive scan of the threads' 6-vectors: what the threads before this one (Rev: after it) sum to.  Lanes by a shuffle scan, the
// waves before (after) in order.  s_w is this call site's own block (a barrier inside)
template <bool Rev>
__device__ __forceinline__ void block_scan6(const double tot[6], double ex[6], double (*s_w)[6]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double inc[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) inc[a] = tot[a];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const bool ok = Rev ? (lane + off < 64) : (lane >= off);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double o = Rev ? __shfl_down(inc[a], off) : __shfl_up(inc[a], off);
      if (ok) inc[a] = inc[a] + o;
    }
  }
  if (lane == (Rev ? 0 : 63)) {
#pragma unroll
    for (int a = 0; a < 6; ++a) s_w[wave][a] = inc[a];
  }
  const bool edge = Rev ? (lane == 63) : (lane == 0);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double o = Rev ? __shfl_down(inc[a], 1) : __shfl_up(inc[a], 1);
    ex[a] = edge ? 0.0 : o;
  }
  __syncthreads();
  double base[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (Rev) {
    for (int w = kWaves - 1; w > wave; --w)
#pragma unroll
      for (int a = 0; a < 6; ++a) base[a] = base[a] + s_w[w][a];
  } else {
    for (int w = 0; w < wave; ++w)
#pragma unroll
      for (int a = 0; a < 6; ++a) base[a] = base[a] + s_w[w][a];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) ex[a] = base[a] + ex[a];
}

__device__ __forceinline__ void load6(const double* p, double v[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) v[a] = p[a];
}
__device__ __forceinline__ void store6(double* p, const double v[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) p[a] = v[a];
}

// a node's row of J^T (.): its edges' terms in edge order
__device__ __forceinline__ void gather(const GraphArgs& A, int k, double y[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) y[a] = 0.0;
  for (int q = A.node_start[k]; q < A.node_start[k + 1]; ++q) {
    const double* c = A.contrib + 6 * (size_t)A.node_ent[q];
#pragma unroll
    for (int a = 0; a < 6; ++a) y[a] = y[a] + c[a];
  }
}

// e = log(rigid_inverse(Z) * rigid_inverse(P_i) * P_j) and sum_a (w_a e_a) e_a of one edge; Tij = rigid_inverse(P_i) * P_j
__device__ __forceinline__ double edge_residual(const GraphArgs& A, const Pose* P, int e, Pose* Tij, double g[6]) {
  const int2 ij = A.ij[e];
  *Tij = compose(pose_inverse(P[ij.x]), P[ij.y]);
  double err[6];
  se3_log(compose(A.Zinv[e], *Tij), err);
  double c = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    g[a] = A.w[6 * (size_t)e + a] * err[a];
    c = c + g[a] * err[a];
  }
  return c;
}

// z = M^-1 r over the thread's nodes [n0, n1), M = J_c^T W_c J_c of the chain: v_{k-1} = v_k + Ad(Q_k)^-T r_k (a suffix sum),
// u_{k-1} = Ad(Q_k)^T v_{k-1} / w_{k-1}, s_k = s_{k-1} + Ad(Q_k) u_{k-1} (a prefix sum), z_k = Ad(Q_k^-1) s_k.  Returns r . z
__device__ __forceinline__ double precondition(const GraphArgs& A, int n0, int n1, double (*s_scan)[kWaves][6], double* s_red) {
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ex[6], v[6], u[6];
  for (int k = n1 - 1; k >= n0; --k) {
    const Rt Qi = A.Qi[k];
    load6(A.r + 6 * (size_t)k, v);
    ad_t(Qi, v, u);
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] = acc[a] + u[a];
    store6(A.tmp + 6 * (size_t)k, acc);
  }
  block_scan6<true>(acc, ex, s_scan[0]);
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[a] = 0.0;
  for (int k = n0; k < n1; ++k) {
    const Rt Q = A.Q[k];
    load6(A.tmp + 6 * (size_t)k, v);
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a] = ex[a] + v[a];
    ad_t(Q, v, u);
#pragma unroll
    for (int a = 0; a < 6; ++a) u[a] = u[a] / A.w[6 * (size_t)(k - 1) + a];
    ad(Q, u, v);
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] = acc[a] + v[a];
    store6(A.tmp + 6 * (size_t)k, acc);
  }
  block_scan6<false>(acc, ex, s_scan[1]);
  double part = 0.0;
  for (int k = n0; k < n1; ++k) {
    const Rt Qi = A.Qi[k];
    load6(A.tmp + 6 * (size_t)k, v);
#pragma unroll
    for (int a = 0; a < 6; ++a) v[a] = ex[a] + v[a];
    ad(Qi, v, u);
    store6(A.z + 6 * (size_t)k, u);
    load6(A.r + 6 * (size_t)k, v);
#pragma unroll
    for (int a = 0; a < 6; ++a) part = part + v[a] * u[a];
  }
  return block_sum(part, s_red);
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_step(GraphArgs A) {
  __shared__ double s_red[5][kWaves];          // one row per reduction site: a site's next use is barriers away
  __shared__ double s_scan[2][kWaves][6];
  const int tid = threadIdx.x;
  const int n0 = 1 + tid * A.chunk, n1 = min(n0 + A.chunk, A.n);   // this thread's nodes (none when n0 >= n)

  // ---- linearise at P
  double part = 0.0;
  for (int e = tid; e < A.m; e += kT) {
    Pose Tij;
    double g[6], gi[6];
    part = part + edge_residual(A, A.P, e, &Tij, g);
    const Rt Aij = to_rt(pose_inverse(Tij));
    A.A[e] = Aij;
    ad_t(Aij, g, gi);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      A.contrib[12 * (size_t)e + a] = -g[a];       // -J_j^T W e
      A.contrib[12 * (size_t)e + 6 + a] = gi[a];   // -J_i^T W e
    }
  }
  const Pose P0inv = pose_inverse(A.P[0]);
  for (int k = n0; k < n1; ++k) {
    const Pose Q = compose(P0inv, A.P[k]);
    A.Q[k] = to_rt(Q);
    A.Qi[k] = to_rt(pose_inverse(Q));
  }
  if (tid < 6) A.p[tid] = 0.0;   // node 0 is fixed: its row of p stays 0
  const double cost_before = block_sum(part, s_red[0]);
  double v[6], u[6];
  for (int k = n0; k < n1; ++k) {
    gather(A, k, v);
    store6(A.r + 6 * (size_t)k, v);
#pragma unroll
    for (int a = 0; a < 6; ++a) A.x[6 * (size_t)k + a] = 0.0;
  }

  // ---- (J^T W J) d = -J^T W e by preconditioned conjugate gradients
  double rz = 0.0, rz0 = 0.0;
  int it = 0, limit = 0;
  for (;;) {
    const double rz_new = precondition(A, n0, n1, s_scan, s_red[1]);
    const double beta = it ? rz_new / rz : 0.0;
    for (int k = n0; k < n1; ++k) {
      load6(A.z + 6 * (size_t)k, v);
      if (it) {
        load6(A.p + 6 * (size_t)k, u);
#pragma unroll
        for (int a = 0; a < 6; ++a) v[a] = v[a] + beta * u[a];
      }
      store6(A.p + 6 * (size_t)k, v);
    }
    if (!it) rz0 = rz_new;
    rz = rz_new;
    if (!(rz > A.cg_tol2 * rz0)) break;
    if (it >= A.max_cg) { limit = 1; break; }
    __syncthreads();
    for (int e = tid; e < A.m; e += kT) {
      const int2 ij = A.ij[e];
      const Rt Aij = A.A[e];
      double q[6];
      load6(A.p + 6 * (size_t)ij.x, v);
      ad(Aij, v, u);
      load6(A.p + 6 * (size_t)ij.y, v);
#pragma unroll
      for (int a = 0; a < 6; ++a) q[a] = A.w[6 * (size_t)e + a] * (v[a] - u[a]);
      ad_t(Aij, q, u);
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        A.contrib[12 * (size_t)e + a] = q[a];
        A.contrib[12 * (size_t)e + 6 + a] = -u[a];
      }
    }
    __syncthreads();
    part = 0.0;
    for (int k = n0; k < n1; ++k) {
      gather(A, k, v);
      store6(A.ap + 6 * (size_t)k, v);
      load6(A.p + 6 * (size_t)k, u);
#pragma unroll
      for (int a = 0; a < 6; ++a) part = part + u[a] * v[a];
    }
    const double pAp = block_sum(part, s_red[2]);
    if (!(pAp > 0.0)) break;
    const double alpha = rz / pAp;
    for (int k = n0; k < n1; ++k) {
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const size_t at = 6 * (size_t)k + a;
        A.x[at] = A.x[at] + alpha * A.p[at];
        A.r[at] = A.r[at] - alpha * A.ap[at];
      }
    }
    ++it;
  }

  // ---- the step and the cost behind it
  double md = 0.0;
  for (int k = n0; k < n1; ++k) {
    load6(A.x + 6 * (size_t)k, v);
#pragma unroll
    for (int a = 0; a < 6; ++a) md = fmax(md, fabs(v[a]));
    A.Pn[k] = compose(A.P[k], se3_exp(v));
  }
  if (tid == 0) A.Pn[0] = A.P[0];
  const double max_step = block_max(md, s_red[3]);
  part = 0.0;
  for (int e = tid; e < A.m; e += kT) {
    Pose Tij;
    part = part + edge_residual(A, A.Pn, e, &Tij, v);
  }
  const double cost_after = block_sum(part, s_red[4]);
  if (tid == 0) {
    GraphRecord R;
    R.cost_before = cost_before;
    R.cost_after = cost_after;
    R.max_step = max_step;
    R.cg_residual = rz0 > 0.0 ? sqrt(rz / rz0) : 0.0;
    R.cg_iterations = it;
    R.cg_limit = limit;
    *A.rec = R;
  }
}

// One workgroup, like the solver: the reductions keep a fixed order.  B is A with the base weights in place of the solver's, so
// that edge_residual states r as it states the cost's terms
__global__ __launch_bounds__(kGraphThreads) void k_graph_reweight(GraphArgs B, GraphReweightArgs W) {
  __shared__ double s_red[5][kWaves];
  const int first = B.n - 1;   // the loop edges are first .. m-1
  const double lo = W.mu / (W.mu + 1.0) * W.c2, hi = (W.mu + 1.0) / W.mu * W.c2;   // (read under kGraphReweightRule only)
  double mx = 0.0, sr = 0.0, n_rej = 0.0, n_kept = 0.0, n_mid = 0.0;   // (counts as doubles: exact, and block_sum adds them)
  for (int e = first + (int)threadIdx.x; e < B.m; e += kT) {
    Pose Tij;
    double g[6];
    const double r = edge_residual(B, B.P, e, &Tij, g);
    const int l = e - first;
    double s = 1.0;
    if (W.mode == kGraphReweightKeep) s = W.s[l];
    if (W.mode == kGraphReweightRule) {
      if (r <= lo) s = 1.0;
      else if (!(r < hi)) s = 0.0;   // (a non-finite r is rejected)
      else s = fmin(fmax(sqrt(W.c2 * W.mu * (W.mu + 1.0) / r) - W.mu, 0.0), 1.0);   // (rounding at the two ends)
    }
    W.s[l] = s;
    W.r[l] = r;
#pragma unroll
    for (int a = 0; a < 6; ++a) W.w[6 * (size_t)e + a] = s * W.w0[6 * (size_t)e + a];
    mx = fmax(mx, r);
    sr = sr + s * r;
    n_rej = n_rej + (s == 0.0 ? 1.0 : 0.0);
    n_kept = n_kept + (s == 1.0 ? 1.0 : 0.0);
    n_mid = n_mid + (s != 0.0 && s != 1.0 ? 1.0 : 0.0);
  }
  const double max_r = block_max(mx, s_red[0]);
  const double sum_sr = block_sum(sr, s_red[1]);
  const double rejected = block_sum(n_rej, s_red[2]);
  const double kept = block_sum(n_kept, s_red[3]);
  const double undecided = block_sum(n_mid, s_red[4]);
  if (threadIdx.x == 0) {
    GraphRobustRecord R;
    R.max_r = max_r;
    R.sum_sr = sum_sr;
    R.rejected = (int)rejected;
    R.kept = (int)kept;
    R.undecided = (int)undecided;
    R.reserved0 = 0;
    *W.rec = R;
  }
}

}  // namespace

void launch_graph_reweight(const GraphArgs& A, const GraphReweightArgs& W, hipStream_t s) {
  GraphArgs B = A;
  B.w = W.w0;
  hipLaunchKernelGGL(k_graph_reweight, dim3(1), dim3(kGraphThreads), 0, s, B, W);
}

void launch_graph_step(const GraphArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_graph_step, dim3(1), dim3(kGraphThreads), 0, s, A);
}

}  // namespace tl
