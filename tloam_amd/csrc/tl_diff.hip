// tl_diff.hip -- the device side of a scan diffed against the closed map (tl_api_diff.hip): a label per
// point of the scan, and per occupied voxel the number of the scan's rays that passed through it (`through`) beside the number
// of its returns that fell in it (`hits`).
//
// Launches of a diff, the same for any scan and map (no host synchronisation between them; nothing of the closed map, of a
// carve's counts or of the surfels is written):
//   k_diff_clear    grid x 256   zeroes through and hits (left out when the call accumulates)
//   k_diff_points   grid x 256   per point: transform, quantise, the 27 read-only probes of the closed map's slot table
//                                (tl_voxel.hpp: probe27), of a hit one LocRecord (and N and the carve's M when the gate is on:
//                                tl_common.hpp's CarveGate, the one definition of a voxel that counts), the
//                                nearest eligible voxel and the nearest voxel, the label, the id, one int64 atomic on the own
//                                cell's hits; the label counts by ballot, one atomic per label and wave
//   k_diff_rays     grid x 256   per ray: the carve's walk (tl_voxel.hpp: ray_walk) from the pose's translation to the point, an
//                                int64 atomic add on a missed voxel's through; the ray's counters summed over the wave by
//                                shuffles, one atomic per counter and wave
//   k_diff_count    grid x 256   per voxel: through > 0 and hits > 0 counted by ballot, through summed over the wave
// The label counts are wave_count_states, the counters' tails wave_add (tl_voxel.hpp); the scan and the map arrive as the Work's
// ScanAt and MapGrid.
// The read of the voxels seen through is k_diff_box: the box read's one body (tl_voxel.hpp: voxel_box_body).
// No block waits on another block.  No floating-point atomics: every sum is an integer, so two calls give the same bytes.
//
// Compiled with -ffp-contract=off.  The arithmetic of a point (tests/closed_map_diff_np.py restates it):
//   E = map_transform_point(M, p),  (i, q) = vmap_quantise(E): not finite or beyond the grid -> INVALID
//   for dz, dy, dx in -1 .. 1 (dx innermost: probe27) the voxel of cell i + (dx, dy, dz) when it has one and the gate leaves it in:
//   d = E - c, D = (d_x*d_x + d_y*d_y) + d_z*d_z; kept under D < best for the eligible voxels, and under D < best for all
//   r = (n_x*d_x + n_y*d_y) + n_z*d_z of the nearest eligible voxel: SURFACE when fabs(r) <= plane_tol;
//   else OCCUPIED when the nearest voxel has D <= near2; else NEW
// and of a ray: tl_carve.hip's header, with O = (M[12], M[13], M[14]).
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__global__ __launch_bounds__(256) void k_diff_clear(DiffWork W) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t t = i; t < (size_t)W.grid.nv; t += stride) {
    W.through[t] = 0ull;
    W.hits[t] = 0ull;
  }
}

__global__ __launch_bounds__(256) void k_diff_points(DiffWork W) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < W.scan.n;
  int label = TLOAM_DIFF_INVALID;
  if (live) {
    double E[3];
    map_transform_point(W.scan.M, W.scan.pts[3 * g], W.scan.pts[3 * g + 1], W.scan.pts[3 * g + 2], &E[0], &E[1], &E[2]);
    unsigned long long key;
    unsigned q[3];
    int explained = -1;
    if (vmap_quantise(E, W.grid.origin, W.grid.voxel, &key, q) == kVmapInside) {
      int own = -1, be = -1, ba = -1;         // the own cell's voxel, the nearest eligible voxel, the nearest voxel
      double bDe = HUGE_VAL, bDa = HUGE_VAL, r = 0.0;
      probe27(W.grid.map, key, [&](int id, bool is_own) {
        if (is_own) own = id;   // (before the gate: the hits are ungated)
        if (!W.gate.counts(W.grid.map, id)) return;
        const LocRecord* R = W.rec + id;
        const double d0 = E[0] - R->c[0], d1 = E[1] - R->c[1], d2 = E[2] - R->c[2];
        const double D = (d0 * d0 + d1 * d1) + d2 * d2;
        if (R->eligible && D < bDe) {
          be = id; bDe = D;
          r = (R->n[0] * d0 + R->n[1] * d1) + R->n[2] * d2;
        }
        if (D < bDa) { ba = id; bDa = D; }
      });
      if (be >= 0 && fabs(r) <= W.plane_tol) {
        label = TLOAM_DIFF_SURFACE;
        explained = be;
      } else if (ba >= 0 && bDa <= W.near2) {
        label = TLOAM_DIFF_OCCUPIED;
        explained = ba;
      } else {
        label = TLOAM_DIFF_NEW;
      }
      if (own >= 0) atomicAdd(&W.hits[own], 1ull);
    }
    W.labels[g] = (unsigned char)label;
    if (W.ids) W.ids[g] = explained;
  }
  wave_count_states(live, label, W.ctl);
}

__global__ __launch_bounds__(256) void k_diff_rays(DiffWork W) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long skipped = 0ull, steps = 0ull, tested = 0ull, misses = 0ull;
  if (g < W.scan.n) {
    const double* M = W.scan.M;
    double E[3];
    map_transform_point(M, W.scan.pts[3 * g], W.scan.pts[3 * g + 1], W.scan.pts[3 * g + 2], &E[0], &E[1], &E[2]);
    ray_walk(W.grid, W.max_range, W.end_margin, W.radius2, M[12], M[13], M[14], E[0], E[1], E[2], &skipped, &steps, &tested,
             &misses, [&](int id) { atomicAdd(&W.through[id], 1ull); });
  }
  wave_add(&W.ctl[4], skipped);
  wave_add(&W.ctl[5], steps);
  wave_add(&W.ctl[6], tested);
}

__global__ __launch_bounds__(256) void k_diff_count(DiffWork W) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long t = id < W.grid.nv ? W.through[id] : 0ull;
  const unsigned long long bt = __ballot(t > 0ull);
  const unsigned long long bh = __ballot(id < W.grid.nv && W.hits[id] > 0ull);
  wave_add(&W.ctl[7], t);
  if ((threadIdx.x & 63) == 0) {
    if (bt) atomicAdd(&W.ctl[8], (unsigned long long)__popcll(bt));
    if (bh) atomicAdd(&W.ctl[9], (unsigned long long)__popcll(bh));
  }
}

// the box read (the box only when A.boxed) of the voxels seen through; their through and hits beside the counts
struct BoxGone {
  const DiffReadArgs& A;
  __device__ __forceinline__ bool keep(size_t id, long long, const double*) const {
    const long long t = A.through[id], h = A.hits[id];
    return t >= A.min_through && (double)t > A.gone_ratio * (double)h;
  }
  __device__ __forceinline__ long long emit(size_t id, size_t p, long long n) const {
    if (A.out_through) A.out_through[p] = A.through[id];
    if (A.out_hits) A.out_hits[p] = A.hits[id];
    return n;
  }
};
__global__ __launch_bounds__(256) void k_diff_box(DiffReadArgs A, int nblocks) {
  voxel_box_body(A.rows, A.boxed != 0, nblocks, BoxGone{A});
}

}  // namespace

int launch_diff(const DiffWork& W, bool clear, hipStream_t s) {
  const unsigned nv_blocks = blocks_of((size_t)std::max<long long>(W.grid.nv, 1));   // (nothing still launches)
  const unsigned n_blocks = blocks_of((size_t)std::max<long long>(W.scan.n, 1));
  if (clear) hipLaunchKernelGGL(k_diff_clear, dim3(std::min(nv_blocks, 2048u)), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_diff_points, dim3(n_blocks), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_diff_rays, dim3(n_blocks), dim3(256), 0, s, W);
  hipLaunchKernelGGL(k_diff_count, dim3(nv_blocks), dim3(256), 0, s, W);
  return clear ? 4 : 3;
}

void launch_diff_read(const DiffReadArgs& A, hipStream_t s) {
  if (A.rows.count == 0) return;
  const int nb = (int)blocks_of(A.rows.count);
  hipLaunchKernelGGL(k_diff_box, dim3(nb), dim3(256), 0, s, A, nb);
}

}  // namespace tl
