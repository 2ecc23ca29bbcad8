// tl_loop.hip -- the device side of loop verification (tl_api_loop.hip): a keyframe's eight clouds kept in
// the arena, the local target and the source of a verification put together, and the score of the fine pose.
//
// Launches:
//   k_place_clouds   grid x 256   per keyframe (after the frame's last wait, with the place launches; not waited for): the spans
//                                 of the eight clouds the frame handed to the match and the submap, gathered into the arena
//   k_loop_assemble  grid x 256   per verification: the query's source clouds as they are, the window's target clouds moved into
//                                 the match keyframe's frame by their T_rel, written where the coarse stage's context reads them
//   k_loop_score     256 x 256    per verification: every source point moved by the fine pose, its nearest target of the same
//                                 kind over the fine stage's grids (tl_knn.hpp knn_grid_reach), inliers and their squared
//                                 distances summed per kind; block partials in a fixed order, combined by the host in block order
// Both span kernels are segmented grid-stride copies: span j owns rows [start[j], start[j + 1]) of the launch.
// Compiled with -ffp-contract=off: the transform and the squared distances round as tests/loop_np.py restates them.
#include <algorithm>

#include "tl_common.hpp"
#include "tl_knn.hpp"

namespace tl {
namespace {

__device__ __forceinline__ void move_point(const double R[9], const double t[3], double x, double y, double z, double o[3]) {
  o[0] = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
  o[1] = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
  o[2] = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
}

__device__ __forceinline__ void span_rows(const LoopSpanArgs& A) {
  const long long total = A.start[A.nspan];
  const long long stride = (long long)gridDim.x * blockDim.x;
  int j = 0;
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < total; r += stride) {
    while (r >= A.start[j + 1]) ++j;   // (rows ascend along a thread's walk: the span index only moves forward)
    const LoopSpan& S = A.s[j];
    const long long i = r - A.start[j];
    const long long p = S.idx ? (long long)S.idx[i] : i;
    const double x = S.src[3 * p], y = S.src[3 * p + 1], z = S.src[3 * p + 2];
    double* d = S.dst + 3 * i;
    if (S.rigid) {
      double o[3];
      move_point(S.R, S.t, x, y, z, o);
      d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    } else {
      d[0] = x; d[1] = y; d[2] = z;
    }
  }
}

__global__ __launch_bounds__(256) void k_place_clouds(LoopSpanArgs A) { span_rows(A); }
__global__ __launch_bounds__(256) void k_loop_assemble(LoopSpanArgs A) { span_rows(A); }

__global__ __launch_bounds__(256) void k_loop_score(LoopScoreArgs A) {
  __shared__ double s_part[4][kKinds][2];
  double cnt[kKinds], sum[kKinds];
#pragma unroll
  for (int k = 0; k < kKinds; ++k) { cnt[k] = 0.0; sum[k] = 0.0; }
  const long long stride = (long long)gridDim.x * 256;
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kKinds; ++k) {
    if (A.g[k].n <= 0) continue;
    for (long long i = first; i < A.n[k]; i += stride) {
      const double* p = A.src[k] + 3 * i;
      double q[3];
      move_point(A.R, A.t, p[0], p[1], p[2], q);
      TopK<1> tk;
      knn_grid_reach<1>(A.g[k], q[0], q[1], q[2], A.reach[k], tk);
      if (tk.j[0] >= 0 && tk.d[0] < A.r2) {
        cnt[k] = cnt[k] + 1.0;
        sum[k] = sum[k] + tk.d[0];
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kKinds; ++k) {
    for (int off = 32; off > 0; off >>= 1) {
      cnt[k] = cnt[k] + __shfl_xor(cnt[k], off, 64);
      sum[k] = sum[k] + __shfl_xor(sum[k], off, 64);
    }
    if (lane == 0) { s_part[wave][k][0] = cnt[k]; s_part[wave][k][1] = sum[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * kKinds) {
    const int k = threadIdx.x >> 1, c = threadIdx.x & 1;
    const double v = ((s_part[0][k][c] + s_part[1][k][c]) + s_part[2][k][c]) + s_part[3][k][c];
    A.partial[((size_t)blockIdx.x * kKinds + k) * 2 + c] = v;
  }
}

unsigned span_blocks(const LoopSpanArgs& A) {
  return (unsigned)std::min<long long>((A.start[A.nspan] + 255) / 256, 1024);
}

}  // namespace

void launch_place_clouds(const LoopSpanArgs& A, hipStream_t s) {
  if (A.nspan <= 0 || A.start[A.nspan] <= 0) return;
  hipLaunchKernelGGL(k_place_clouds, dim3(span_blocks(A)), dim3(256), 0, s, A);
}
void launch_loop_assemble(const LoopSpanArgs& A, hipStream_t s) {
  if (A.nspan <= 0 || A.start[A.nspan] <= 0) return;
  hipLaunchKernelGGL(k_loop_assemble, dim3(span_blocks(A)), dim3(256), 0, s, A);
}
void launch_loop_score(const LoopScoreArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_loop_score, dim3(kLoopScoreBlocks), dim3(256), 0, s, A);
}

}  // namespace tl
