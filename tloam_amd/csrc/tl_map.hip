// tl_map.hip -- the device side of the odometry frame's global map (tl_api_map.hip): FrontEnd::updateSubmap's
// mapping branch, global_map += raw.Transform(lidar_odom_pose).VoxelDownSample(1.0) (front_end.cpp:269-274), on the raw scan
// the frame already holds in HBM.
//
// Launches (a later frame with mapping on, after the scan match; no host synchronisation in between):
//   k_map_front       grid x 256   the raw scan transformed (Open3D TransformPoints: map_transform_point) into
//                                  SoA scratch; the same launch empties the hash table and finishes the min bound of the
//                                  transformed cloud (block partials, the last block by ticket) -- k_submap_front's work for one segment
//   k_map_insert      grid x 256   voxel -> hash slot; the slot's member list, count and smallest member (atomics)
//   k_map_emit        grid x 256   leaders in first-occurrence order (the look-back scan of tl_voxel.hpp); a voxel of up to
//                                  kVoxLocal members averaged by its leader, a larger one booked; the count to pinned memory
//   k_map_scatter     grid x 256   the members of the booked voxels into one piece each
//   k_map_big         <= 1024 x 256  one workgroup per booked voxel: members ordered by index, summed in that order
//   k_transform_aos   grid x 256   the registered scan of a frame whose map stage did not run, AoS -> AoS
// The submap's voxel job (tl_submap.hip) finds a leader by walking the member list from every member and heap-sorts a crowded
// voxel in one lane: fine for thinned edge / ground clouds, 13 ms per frame on 1 m cells of a raw scan.
// Compiled with -ffp-contract=off: the transform and voxel_min_bound round as the oracle's pc_transform / pc_voxel_down_sample.
#include <string.h>

#include <algorithm>
#include <atomic>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__device__ __forceinline__ bool in_box(const MapVoxWork& W, double x, double y, double z) {   // inclusive, as Crop
  return x >= W.lo && x <= W.hi && y >= W.lo && y <= W.hi && z >= W.lo && z <= W.hi;
}

__global__ __launch_bounds__(256) void k_map_front(MapFrontArgs A, MapVoxWork W, int emit_blocks) {
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * 256 + tid, stride = (size_t)gridDim.x * 256;
  if (blockIdx.x == 0 && tid == 0) { W.ctl[0] = 0; W.ctl[2] = 0; W.ctl[3] = 0; W.ctl[4] = 0; }
  for (size_t t = i; t <= W.mask; t += stride) {
    W.keys[t] = kFree;
    W.head[t] = -1;
    W.first[t] = 0x7fffffff;
    W.count[t] = 0;
  }
  for (size_t t = i; t <= (size_t)emit_blocks; t += stride) W.leader[t] = 0ull;
  for (size_t t = i; t < (size_t)W.big_max; t += stride) W.bigfill[t] = 0;
  double m[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()};
  if (i < A.n) {
    double x, y, z;
    map_transform_point(A.M, A.aos[3 * i], A.aos[3 * i + 1], A.aos[3 * i + 2], &x, &y, &z);
    W.x[i] = x; W.y[i] = y; W.z[i] = z;
    if (in_box(W, x, y, z)) { m[0] = x; m[1] = y; m[2] = z; }
  }
  // voxel_min_bound of the transformed cloud, finished by the last block (&W.voxel: a one-element array -- with C == 3 columns
  // voxel_min_bound only ever reads voxel[0])
  voxel_min_bound<3, 3>(m, 0, W.min_partial, (int)blockIdx.x, (int)gridDim.x, W.ctl + 1, &W.voxel, W.vmin);
}

// the voxel of every point in the box -> hash slot; the point joins the slot's member list, count and smallest index
__global__ __launch_bounds__(256) void k_map_insert(MapVoxWork W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= W.n) return;
  const double x = W.x[i], y = W.y[i], z = W.z[i];
  if (!in_box(W, x, y, z)) { W.slot_of_pt[i] = -1; return; }
  unsigned long long key = 0ull;
  if (!voxel_key(x, y, z, W.vmin, W.voxel, &key)) {
    W.ctl[0] = 1;   // "[VoxelDownSample] voxel_size is too small." (PointCloud2.cpp:370-372)
    W.slot_of_pt[i] = -1;
    return;
  }
  const unsigned long long h = table_enter(W.keys, W.mask, key);
  W.slot_of_pt[i] = (int)h;
  W.next[i] = atomicExch(&W.head[h], (int)i);
  atomicMin(&W.first[h], (int)i);
  atomicAdd(&W.count[h], 1);
}

// per point: a leader of a voxel of up to kVoxLocal members orders them by index in LDS (the order AddPoint is called in,
// :379-385), sums and averages; its output position -- the leaders in front of it, i.e. first-occurrence order -- comes from a
// single-pass scan over the blocks inside the launch (tl_voxel.hpp).  The leader of a larger voxel books the voxel for
// k_map_big: a number, the output position, a piece of `members`
__global__ __launch_bounds__(256) void k_map_emit(MapVoxWork W, int nblocks) {
  __shared__ int s_mem[kVoxLocal * 256];   // s_mem[k * 256 + t]: member k of thread t's voxel (conflict-free columns)
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const int tid = threadIdx.x;
  // places in the order the blocks start when the grid is larger than the device holds at once: see k_vox_emit
  int bid = (int)blockIdx.x;
  if (W.use_ticket) bid = block_ticket(&W.ctl[2], &s_bid);
  const size_t i = (size_t)bid * 256 + tid;
  const int h = i < W.n ? W.slot_of_pt[i] : -1;
  const bool leader = h >= 0 && W.first[h] == (int)i;
  const int m = leader ? W.count[h] : 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  if (leader && m <= kVoxLocal) {
    int k = 0;
    for (int j = W.head[h]; j >= 0 && k < kVoxLocal; j = W.next[j]) s_mem[(k++) * 256 + tid] = j;
    // AccumulatedPoint: point_ += p in index order, GetAveragePoint = point_ / double(num) (:253-272)
    leader_local_sum(s_mem, k, W.x, W.y, W.z, &sx, &sy, &sz);
    const double dn = (double)m;
    sx /= dn; sy /= dn; sz /= dn;
  }
  // ---- the leader's output position: the leaders in front of it in the block, and in the blocks in front
  unsigned long long before, block_total;
  block_packed_scan(leader ? 1ull : 0ull, s_wave, &before, &block_total);
  if (tid == 0) s_prefix = lookback_prefix(W.leader, bid, block_total, LookFaultHost{W.fault});   // (the host discards a faulted frame)
  __syncthreads();
  if (leader) {
    const unsigned long long p = s_prefix + before;
    if (m <= kVoxLocal) {
      W.ox[p] = sx; W.oy[p] = sy; W.oz[p] = sz;
    } else {
      const int q = atomicAdd(&W.ctl[3], 1);   // (< big_max: a big voxel has more than kVoxLocal members)
      const int off = atomicAdd(&W.ctl[4], m);
      W.bigq[q] = make_int4(h, (int)p, off, m);
      W.bigslot[h] = q;
    }
  }
  if (bid == nblocks - 1 && tid < 8) {   // the block that holds the last point: the total = the size of the down-sampled cloud
    const unsigned long long total = s_prefix + block_total;
    if (tid == 0) W.n_out[0] = total;
    // ... and straight to the host
    post_host_segment(W.host_seg, W.host_seq, tid == 0 ? total : tid == 2 ? (unsigned long long)W.ctl[0] : 0ull, tid);
  }
}

// the members of every big voxel into its piece of `members` (in no particular order: k_map_big orders them)
__global__ __launch_bounds__(256) void k_map_scatter(MapVoxWork W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= W.n) return;
  const int h = W.slot_of_pt[i];
  if (h < 0 || W.count[h] <= kVoxLocal) return;
  const int q = W.bigslot[h];
  const int4 b = W.bigq[q];
  W.members[b.z + atomicAdd(&W.bigfill[q], 1)] = (int)i;
}

// one workgroup per big voxel: its members sorted by index (bitonic, in LDS), then summed in that order by one lane from
// coordinates the workgroup stages in LDS, 256 at a time.  A voxel of more than kMapSortLds members is not sorted: the workgroup
// walks the points from the voxel's first member on, 256 at a time, and picks its members out in index order as it goes
constexpr int kMapSortLds = 8192;
__global__ __launch_bounds__(256) void k_map_big(MapVoxWork W) {
  __shared__ int s_idx[kMapSortLds];
  __shared__ double s_c[3][256];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x;
  const int nbig = W.ctl[3];
  for (int q = (int)blockIdx.x; q < nbig; q += (int)gridDim.x) {
    const int4 b = W.bigq[q];
    const int h = b.x, p = b.y, off = b.z, m = b.w;
    // AccumulatedPoint: point_ += p in index order (:253-272); lane 0 of the workgroup adds, the others stage
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (m <= kMapSortLds) {
      const int* mem = W.members + off;
      int P = 1;
      while (P < m) P <<= 1;
      for (int t = tid; t < P; t += 256) s_idx[t] = t < m ? mem[t] : 0x7fffffff;
      __syncthreads();
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int t = tid; t < P; t += 256) {
            const int u = t ^ j;
            if (u > t) {
              const int a = s_idx[t], c = s_idx[u];
              if ((a > c) == ((t & k) == 0)) { s_idx[t] = c; s_idx[u] = a; }
            }
          }
          __syncthreads();
        }
      for (int c0 = 0; c0 < m; c0 += 256) {
        const int k = c0 + tid;
        if (k < m) {
          const int j = s_idx[k];
          s_c[0][tid] = W.x[j]; s_c[1][tid] = W.y[j]; s_c[2][tid] = W.z[j];
        }
        __syncthreads();
        if (tid == 0) {
          const int e = min(256, m - c0);
          for (int r = 0; r < e; ++r) { sx += s_c[0][r]; sy += s_c[1][r]; sz += s_c[2][r]; }
        }
        __syncthreads();
      }
    } else {
      int found = 0;   // (block-uniform)
      for (size_t base = (size_t)W.first[h]; base < W.n && found < m; base += 256) {
        const size_t j = base + tid;
        const bool hit = j < W.n && W.slot_of_pt[j] == h;
        int pos, total;
        block_flag_scan(hit, s_wave, &pos, &total);
        if (hit) {
          s_c[0][pos] = W.x[j]; s_c[1][pos] = W.y[j]; s_c[2][pos] = W.z[j];
        }
        __syncthreads();
        if (tid == 0)
          for (int r = 0; r < total; ++r) { sx += s_c[0][r]; sy += s_c[1][r]; sz += s_c[2][r]; }
        found += total;
        __syncthreads();
      }
    }
    if (tid == 0) {
      const double dn = (double)m;
      W.ox[p] = sx / dn; W.oy[p] = sy / dn; W.oz[p] = sz / dn;
    }
  }
}

__global__ __launch_bounds__(256) void k_transform_aos(const double* __restrict__ aos, size_t n, MapFrontArgs A,
                                                       double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double x, y, z;
  map_transform_point(A.M, aos[3 * i], aos[3 * i + 1], aos[3 * i + 2], &x, &y, &z);
  out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z;
}

}  // namespace

void launch_map_voxel(const MapFrontArgs& A, const MapVoxWork& W, hipStream_t s) {
  const size_t n = W.n;
  const int emit_blocks = (int)blocks_of(n + 1);   // (n + 1: an empty job still has a block that reports a size of 0)
  hipLaunchKernelGGL(k_map_front, dim3(blocks_of(std::max<size_t>(n, 1))), dim3(256), 0, s, A, W, emit_blocks);
  if (n > 0) hipLaunchKernelGGL(k_map_insert, dim3(blocks_of(n)), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_map_emit, dim3(emit_blocks), dim3(256), 0, s, W, emit_blocks);
  if (n <= (size_t)kVoxLocal) return;   // (no voxel can be big)
  hipLaunchKernelGGL(k_map_scatter, dim3(blocks_of(n)), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_map_big, dim3((unsigned)std::min(W.big_max, 1024)), dim3(256), 0, s, W);
}

int map_emit_resident_blocks(int device_cus) {
  static std::atomic<int> per_cu_cache{-1};
  return emit_resident_blocks(k_map_emit, per_cu_cache, device_cus);
}

void launch_transform_aos(const double* aos, size_t n, const double M[16], double* out, hipStream_t s) {
  if (n == 0) return;
  MapFrontArgs A;
  memset(&A, 0, sizeof(A));
  for (int k = 0; k < 16; ++k) A.M[k] = M[k];
  hipLaunchKernelGGL(k_transform_aos, dim3(blocks_of(n)), dim3(256), 0, s, aos, n, A, out);
}

}  // namespace tl
