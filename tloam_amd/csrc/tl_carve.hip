// tl_carve.hip -- the device side of the closed map's carve (tl_api_carve.hip): per occupied voxel of the
// closed map the number M of keyframe rays that passed through it, beside the number N of returns that fell in it.
//
// Launches of a carve, the same three for any number of keyframes, spans and rays (no host synchronisation between them):
//   k_carve_clear   grid x 256   zeroes M and the control words
//   k_carve_rays    grid x 256   per ray: its span from its global index, transform (span_point), then tl_voxel.hpp's ray_walk:
//                                the walk through the grid's cells, every visited cell looked up in the closed map's slot table
//                                (id_table_find), the miss test against an occupied cell's centroid; a miss is an int64 atomic
//                                add on the voxel's M; the ray's counters summed over the wave by shuffles, one atomic per counter
//                                and wave
//   k_carve_count   grid x 256   per voxel: M > 0 counted by ballot, one atomic per wave
// An extension of the closed map (tl_api_extend.hip) launches k_carve_rays over the new keyframes' rays and
// k_carve_count without the clear: the misses are added to the M that is there.
// The carved read is k_carve_box: the box read's one body (tl_voxel.hpp: voxel_box_body), with the voxels seen through left out
// by the carve gate's own test (tl_common.hpp: CarveGate::seen_through, which the diff, the ray-cast and the free space ask too).
//
// Compiled with -ffp-contract=off.  The operation order of a ray (ray_walk; tests/closed_map_carve_np.py restates it), per axis a:
//   O_a = P[12 + a],  E = map_transform_point(P, p),  D_a = E_a - O_a,  DD = (Dx*Dx + Dy*Dy) + Dz*Dz,  L = sqrt(DD)
//   s0_a = (O_a - o_a) / v,  s1_a = (E_a - o_a) / v,  c_a = floor(s0_a),  ce_a = floor(s1_a),  d_a = s1_a - s0_a
//   tMax_a = ((c_a + 1) - s0_a) / d_a  (d_a > 0),  (c_a - s0_a) / d_a  (d_a < 0),  +inf  (d_a == 0 or c_a == ce_a)
//   tDelta_a = step_a / d_a,  step_a = sign(d_a)
//   n = sum_a |ce_a - c_a| steps; before each one the current cell is visited; the step takes the axis of the smallest tMax
//   (a tie: the lowest axis), c_a += step_a, tMax_a = +inf when c_a == ce_a, else tMax_a + tDelta_a
//   an occupied visited cell with centroid C:  u_a = C_a - O_a,  tt = ((ux*Dx + uy*Dy) + uz*Dz) / DD,  w_a = u_a - tt * D_a,
//   a miss when 0 <= tt, tt < 1 - end_margin / L and (wx*wx + wy*wy) + wz*wz <= radius * radius
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__global__ __launch_bounds__(256) void k_carve_clear(CarveWork W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t t = i; t < (size_t)W.grid.nv; t += stride) W.miss[t] = 0ull;
  if (i < 8) W.ctl[i] = 0ull;
}

__global__ __launch_bounds__(256) void k_carve_rays(CarveWork W) {
  __shared__ int s_span[2];
  block_spans(W.in, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long skipped = 0ull, steps = 0ull, tested = 0ull, misses = 0ull;
  if (g < W.in.n) {
    int kf;
    const double* P;
    double E[3];
    span_point(W.in, g, s_span[0], s_span[1], &kf, &P, E);
    ray_walk(W.grid, W.max_range, W.end_margin, W.radius2, P[12], P[13], P[14], E[0], E[1], E[2], &skipped, &steps, &tested,
             &misses, [&](int id) { atomicAdd(&W.miss[id], 1ull); });
  }
  wave_add(&W.ctl[0], skipped);
  wave_add(&W.ctl[1], steps);
  wave_add(&W.ctl[2], tested);
  wave_add(&W.ctl[3], misses);
}

__global__ __launch_bounds__(256) void k_carve_count(CarveWork W) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long bal = __ballot(id < W.grid.nv && W.miss[id] > 0ull);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&W.ctl[4], (unsigned long long)__popcll(bal));
}

// the box read (the box only when A.boxed) with the voxels seen through left out (the gate's own test, whatever gate.gate says:
// the read is the gate's; min_count is the box read's); their misses beside the counts
struct BoxCarved {
  const CarveReadArgs& A;
  __device__ __forceinline__ bool keep(size_t id, long long n, const double*) const {
    return !A.gate.seen_through(A.gate.miss[id], n);
  }
  __device__ __forceinline__ long long emit(size_t id, size_t p, long long n) const {
    if (A.out_m) A.out_m[p] = A.gate.miss[id];
    return n;
  }
};
__global__ __launch_bounds__(256) void k_carve_box(CarveReadArgs A, int nblocks) {
  voxel_box_body(A.rows, A.boxed != 0, nblocks, BoxCarved{A});
}

}  // namespace

int launch_carve(const CarveWork& W, hipStream_t s) {
  const unsigned nv_blocks = blocks_of((size_t)std::max<long long>(W.grid.nv, 1));   // (nothing still launches)
  hipLaunchKernelGGL(k_carve_clear, dim3(std::min(nv_blocks, 2048u)), dim3(256), 0, s, W);
  return 1 + launch_carve_rays(W, s) + launch_carve_count(W, s);
}

int launch_carve_rays(const CarveWork& W, hipStream_t s) {
  hipLaunchKernelGGL(k_carve_rays, dim3(blocks_of((size_t)std::max<long long>(W.in.n, 1))), dim3(256), 0, s, W);
  return 1;
}

int launch_carve_count(const CarveWork& W, hipStream_t s) {
  hipLaunchKernelGGL(k_carve_count, dim3(blocks_of((size_t)std::max<long long>(W.grid.nv, 1))), dim3(256), 0, s, W);
  return 1;
}

void launch_carve_read(const CarveReadArgs& A, hipStream_t s) {
  if (A.rows.count == 0) return;
  const int nb = (int)blocks_of(A.rows.count);
  hipLaunchKernelGGL(k_carve_box, dim3(nb), dim3(256), 0, s, A, nb);
}

}  // namespace tl
