// tl_vmap.hip -- the device side of the odometry frame's merged voxel map (tl_api_vmap.hip): one grid
// for the whole run, per voxel the count and the int64 sums of the quantised offsets of every return that fell in it.
//
// Launches (a later frame with the voxel map on, beside the append map's after the scan match; no host synchronisation):
//   k_vmap_clear    grid x 256   empties the frame's table, the look-back words and the control words
//   k_vmap_stage    grid x 256   per point: (transform,) key and q; runs of equal keys in a wave summed by shuffles, the run's
//                                head enters the frame's table and takes the atomic minimum of the point index, its tail adds
//                                N and Q with int64 atomics (one per run, not per point: 1 m cells of a raw scan are crowded)
//   k_vmap_emit     grid x 256   per frame voxel (at its leader): the persistent table looked up (read only), new voxels numbered
//                                in leader order by a single-pass look-back scan; counts and overflow to pinned memory
// an accepted frame (after the frame's last wait, not waited for):
//   k_vmap_commit   grid x 256   per frame voxel: N and Q added into its id's row; a new one keyed and entered in the table
// Compiled with -ffp-contract=off: map_transform_point, vmap_quantise and centroid round as DESIGN.md 13 and 14 state them.
#include <string.h>

#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__global__ __launch_bounds__(256) void k_vmap_clear(VmapStageWork W, int emit_blocks) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  const size_t T = (size_t)W.fmask + 1;
  for (size_t t = i; t < T; t += stride) {
    W.fkey[t] = kFree;
    W.flead[t] = 0x7fffffff;
    W.fsum[t] = 0ull; W.fsum[T + t] = 0ull; W.fsum[2 * T + t] = 0ull; W.fsum[3 * T + t] = 0ull;
  }
  for (size_t t = i; t <= (size_t)emit_blocks; t += stride) W.look[t] = 0ull;
  if (i < 8) W.ctl[i] = 0ull;
}

__global__ __launch_bounds__(256) void k_vmap_stage(VmapStageWork W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool ok = false, over = false;
  unsigned long long key = 0ull;
  unsigned q[3] = {0u, 0u, 0u};
  if (i < W.n) {
    double p[3];
    if (W.sx) { p[0] = W.sx[i]; p[1] = W.sy[i]; p[2] = W.sz[i]; }
    else map_transform_point(W.M, W.aos[3 * i], W.aos[3 * i + 1], W.aos[3 * i + 2], &p[0], &p[1], &p[2]);
    const VmapCell cell = vmap_quantise(p, W.origin, W.voxel, &key, q);
    ok = cell == kVmapInside;
    over = cell == kVmapBeyond;
  }
  if (over) __hip_atomic_store(&W.ctl[0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const WaveRun r = wave_run_sums(ok, key, q);
  int slot = -1;
  if (r.head) {
    slot = (int)table_enter(W.fkey, W.fmask, key);
    atomicMin(&W.flead[slot], (int)i);   // the run's head is its smallest index
  }
  slot = __shfl(slot, r.head_lane, 64);
  if (i < W.n) W.slot_of_pt[i] = ok ? slot : -1;
  if (r.tail) {
    const size_t T = (size_t)W.fmask + 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(&W.fsum[k * T + slot], (unsigned long long)r.sum[k]);
  }
  const unsigned long long okb = __ballot(ok);
  if (lane == 0 && okb) atomicAdd(&W.ctl[1], (unsigned long long)__popcll(okb));
}

// per point: the leader of a frame voxel finds it in the persistent table or numbers it after every earlier voxel, in
// leader order; the block holding the last point posts the counts to the host
__global__ __launch_bounds__(256) void k_vmap_emit(VmapStageWork W, int nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const int tid = threadIdx.x;
  const int bid = block_ticket(&W.ctl[2], &s_bid);
  const size_t i = (size_t)bid * 256 + tid;
  const int h = i < W.n ? W.slot_of_pt[i] : -1;
  const bool leader = h >= 0 && W.flead[h] == (int)i;
  unsigned long long upto;
  const int id = staged_voxel_id(leader, leader ? W.fkey[h] : 0ull, W.pmask, W.ptab, W.pkey, W.base, W.look, bid, &W.ctl[3], s_wave,
                                 &s_prefix, &upto);
  if (leader) W.fid[h] = id;
  if (bid == nblocks - 1 && tid < 8) {   // the block that holds the last point: the frame's new voxels
    if (tid == 0) W.ctl[4] = upto;
    unsigned long long w = tid == 0 ? upto
                         : tid == 1 ? __hip_atomic_load(&W.ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                         : tid == 2 ? __hip_atomic_load(&W.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                         : tid == 3 ? __hip_atomic_load(&W.ctl[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    post_host_segment(W.host_seg, W.host_seq, w, tid);
  }
}

// per occupied slot of the frame's table: its sums into its id's row (one slot per id: plain stores and adds); a new voxel is
// keyed and entered in the persistent table (load <= 1/2: a free slot is found)
__global__ __launch_bounds__(256) void k_vmap_commit(VmapStageWork W, VmapTable P) {
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (s > W.fmask) return;
  const unsigned long long key = W.fkey[s];
  if (key == kFree) return;
  const size_t T = (size_t)W.fmask + 1;
  const int id = W.fid[s];
  const long long n = (long long)W.fsum[s], qx = (long long)W.fsum[T + s], qy = (long long)W.fsum[2 * T + s],
                  qz = (long long)W.fsum[3 * T + s];
  staged_voxel_commit(P, id, id >= W.base, key, n, qx, qy, qz);
}

__global__ __launch_bounds__(256) void k_vmap_rehash(VmapTable P, size_t n) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  id_table_insert(P.ptab, P.pmask, P.pkey[id], (int)id);
}

__global__ __launch_bounds__(256) void k_vmap_read(VmapReadArgs A) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= A.count) return;
  double c[3];
  long long n;
  voxel_centroid(A.map, A.origin, A.voxel, A.first + k, c, &n);
  if (A.out_c) { A.out_c[3 * k] = c[0]; A.out_c[3 * k + 1] = c[1]; A.out_c[3 * k + 2] = c[2]; }
  if (A.out_n) A.out_n[k] = n;
}

// the voxels in the box with N >= min_count, compacted in id order (tl_voxel.hpp: voxel_box_body)
__global__ __launch_bounds__(256) void k_vmap_box(VmapReadArgs A, int nblocks) { voxel_box_body(A, true, nblocks, BoxPlain{}); }

}  // namespace

void launch_vmap_stage(const VmapStageWork& W, hipStream_t s) {
  const int emit_blocks = (int)blocks_of(W.n + 1);   // (n + 1: an empty job still has a block that reports)
  const size_t T = (size_t)W.fmask + 1;
  hipLaunchKernelGGL(k_vmap_clear, dim3((unsigned)std::min<size_t>(blocks_of(T), 2048)), dim3(256), 0, s, W, emit_blocks);
  if (W.n > 0) hipLaunchKernelGGL(k_vmap_stage, dim3(blocks_of(W.n)), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_vmap_emit, dim3(emit_blocks), dim3(256), 0, s, W, emit_blocks);
}

void launch_vmap_commit(const VmapStageWork& W, const VmapTable& T, hipStream_t s) {
  hipLaunchKernelGGL(k_vmap_commit, dim3(blocks_of((size_t)W.fmask + 1)), dim3(256), 0, s, W, T);
}

void launch_vmap_rehash(const VmapTable& T, size_t n, hipStream_t s, bool even_empty) {
  if (n == 0 && !even_empty) return;
  hipLaunchKernelGGL(k_vmap_rehash, dim3(blocks_of(std::max<size_t>(n, 1))), dim3(256), 0, s, T, n);
}

void launch_vmap_read(const VmapReadArgs& A, hipStream_t s) {
  if (A.count == 0) return;
  hipLaunchKernelGGL(k_vmap_read, dim3(blocks_of(A.count)), dim3(256), 0, s, A);
}

void launch_vmap_read_box(const VmapReadArgs& A, hipStream_t s) {
  if (A.count == 0) return;
  const int nb = (int)blocks_of(A.count);
  hipLaunchKernelGGL(k_vmap_box, dim3(nb), dim3(256), 0, s, A, nb);
}

}  // namespace tl
