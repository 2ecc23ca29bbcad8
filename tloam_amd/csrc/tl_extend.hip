// tl_extend.hip -- the device side of the closed map's extension (tl_api_extend.hip): the keyframes added
// since the map was built, loaded or last extended are added to its rows in place.
//
// Launches of the row pass, the same five for any number of new keyframes, spans and points:
//   k_cmap_clear, k_cmap_flag, k_cmap_stage   (tl_cmap.hip: launch_cmap_stage) over a span table of the NEW keyframes alone: the
//                                staging table, the slot of every new point and the overflow flags are sized by the new points
//   k_ext_emit      grid x 256   per new point: the leader of a staged voxel (the smallest global index among the new points)
//                                looks its key up in the map's table (read only) and, when it is not there, numbers it behind the
//                                map's voxels in leader order (tl_voxel.hpp: staged_voxel_id, the look-back bounded)
//   k_ext_commit    grid x 256   per staging slot: N and Q added into its id's row; a fresh id's row written, keyed and entered in
//                                the table, its M and its thirteen surfel sums zeroed (tl_voxel.hpp: staged_voxel_commit)
// The emit and the commit are the merged voxel map's (tl_vmap.hip: k_vmap_emit, k_vmap_commit) fed from the build's staging: the
// numbering and the row update have one body each, in tl_voxel.hpp.  The surfels and the carve of an extension are tl_surfel.hip's
// and tl_carve.hip's kernels, launched without their clears.
// Compiled with -ffp-contract=off (tl_voxel.hpp asks for it; these two kernels hold no floating-point arithmetic).
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__global__ __launch_bounds__(256) void k_ext_emit(ExtendWork X, long long nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ long long s_bid;
  const CmapWork& W = X.w;
  const int tid = threadIdx.x;
  const long long bid = block_ticket(&W.ctl[2], &s_bid);
  const long long g = bid * 256 + tid;
  int h = g < W.in.n ? W.slot_of_pt[g] : -1;
  if (h >= 0 && (unsigned long long)h > W.fmask) h = -1;   // (a slot is the stage's: inside the table)
  const bool leader = h >= 0 && W.flead[h] == (unsigned long long)g;
  unsigned long long upto;
  const int id = staged_voxel_id(leader, leader ? W.fkey[h] : 0ull, W.rows.pmask, W.rows.ptab, W.rows.pkey, X.base, W.look, bid,
                                 &W.ctl[3], s_wave, &s_prefix, &upto);
  if (leader) X.fid[h] = id;
  if (bid == nblocks - 1 && tid == 0) W.ctl[4] = upto;
}

// an id beyond the rows (a look-back that timed out numbered it: the host discards the call) is not written
__global__ __launch_bounds__(256) void k_ext_commit(ExtendWork X) {
  const CmapWork& W = X.w;
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (s > W.fmask) return;
  const unsigned long long key = W.fkey[s];
  if (key == kFree) return;
  const int id = X.fid[s];
  if (id < 0 || (long long)id >= W.row_cap) return;
  const size_t T = (size_t)W.fmask + 1;
  const bool fresh = (long long)id >= X.base;
  staged_voxel_commit(W.rows, id, fresh, key, (long long)W.fsum[s], (long long)W.fsum[T + s], (long long)W.fsum[2 * T + s],
                      (long long)W.fsum[3 * T + s]);
  if (fresh && (long long)id < X.side_cap) {
    if (X.miss) X.miss[id] = 0ull;
    if (X.sums) {
#pragma unroll
      for (int k = 0; k < kSurfelSums; ++k) X.sums[(size_t)id * kSurfelSums + k] = 0ull;
    }
  }
}

}  // namespace

int launch_extend_emit(const ExtendWork& X, hipStream_t s) {
  const long long nb = blocks_of((size_t)std::max<long long>(X.w.in.n, 1));   // (the grid of k_cmap_stage: look[] is sized for it)
  hipLaunchKernelGGL(k_ext_emit, dim3((unsigned)nb), dim3(256), 0, s, X, nb);
  return 1;
}

int launch_extend_commit(const ExtendWork& X, hipStream_t s) {
  hipLaunchKernelGGL(k_ext_commit, dim3(blocks_of((size_t)X.w.fmask + 1)), dim3(256), 0, s, X);
  return 1;
}

}  // namespace tl
