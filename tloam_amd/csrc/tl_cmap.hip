// tl_cmap.hip -- the device side of the closed map (tl_api_cmap.hip): every keyframe's stored clouds,
// each under its keyframe's pose, merged into one grid of the voxel map's kind (tl_voxel.hpp: key, q, N, Q, centroid).
//
// Launches of a build, the same four for any number of keyframes, spans and points (no host synchronisation between the first
// three):
//   k_cmap_clear    grid x 256   empties the build table, the look-back words, the control words and the keyframes' flags
//   k_cmap_flag     grid x 256   per point: its span from its global index, transform, quantise; a finite point beyond the grid
//                                raises its keyframe's flag (a plain store of 1: every writer writes the same value)
//   k_cmap_stage    grid x 256   per point of an unflagged keyframe: the same, then runs of equal keys in a wave summed by
//                                shuffles (wave_run_sums), the run's head enters the table and takes the 64-bit atomic minimum of the
//                                global index, its tail adds N and Q with int64 atomics; the distinct voxels are counted
//   k_cmap_emit     grid x 256   per point: the leader of a voxel numbers it after every earlier leader (single-pass look-back scan
//                                over start tickets, bounded) and writes its row and its table entry: the build is the commit
// Reads are k_vmap_read / k_vmap_box on the closed map's rows.
// Compiled with -ffp-contract=off: map_transform_point and vmap_quantise round as DESIGN.md 13 and 14 state them.
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

// point g (< W.in.n): its keyframe, and where it falls in the grid (key and q when inside)
__device__ __forceinline__ VmapCell cmap_point(const CmapWork& W, long long g, const int s_span[2], int* kf, unsigned long long* key,
                                               unsigned q[3]) {
  const double* P;
  double p[3];
  span_point(W.in, g, s_span[0], s_span[1], kf, &P, p);
  return vmap_quantise(p, W.origin, W.voxel, key, q);
}

__global__ __launch_bounds__(256) void k_cmap_clear(CmapWork W, long long emit_blocks) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  const size_t T = (size_t)W.fmask + 1;
  for (size_t t = i; t < T; t += stride) {
    W.fkey[t] = kFree;
    W.flead[t] = ~0ull;
    W.fsum[t] = 0ull; W.fsum[T + t] = 0ull; W.fsum[2 * T + t] = 0ull; W.fsum[3 * T + t] = 0ull;
  }
  for (size_t t = i; t <= (size_t)emit_blocks; t += stride) W.look[t] = 0ull;
  for (size_t t = i; t < (size_t)W.in.nkf; t += stride) W.kf_over[t] = 0;
  if (i < 8) W.ctl[i] = 0ull;
}

__global__ __launch_bounds__(256) void k_cmap_flag(CmapWork W) {
  __shared__ int s_span[2];
  block_spans(W.in, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= W.in.n) return;
  int kf;
  unsigned long long key;
  unsigned q[3];
  if (cmap_point(W, g, s_span, &kf, &key, q) == kVmapBeyond) W.kf_over[kf] = 1;
}

// one point's voxel entered in the build table: its slot; *fresh when the voxel was not there
__device__ __forceinline__ int cmap_enter(const CmapWork& W, unsigned long long key, unsigned long long g, bool* fresh) {
  const unsigned long long h = table_enter(W.fkey, W.fmask, key, fresh);
  atomicMin(&W.flead[h], g);
  return (int)h;
}

template <bool kRuns>
__global__ __launch_bounds__(256) void k_cmap_stage(CmapWork W) {
  __shared__ int s_span[2];
  block_spans(W.in, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool ok = false, fresh = false;
  unsigned long long key = 0ull;
  unsigned q[3] = {0u, 0u, 0u};
  if (g < W.in.n) {
    int kf;
    ok = cmap_point(W, g, s_span, &kf, &key, q) == kVmapInside && W.kf_over[kf] == 0;
  }
  const unsigned long long okb = __ballot(ok);
  const size_t T = (size_t)W.fmask + 1;
  int slot = -1;
  if (kRuns) {
    // a run may cross a span: the keys decide, and its head is still its smallest global index
    const WaveRun r = wave_run_sums(ok, key, q);
    if (r.head) slot = cmap_enter(W, key, (unsigned long long)g, &fresh);
    slot = __shfl(slot, r.head_lane, 64);
    if (r.tail) {
#pragma unroll
      for (int k = 0; k < 4; ++k) atomicAdd(&W.fsum[k * T + slot], (unsigned long long)r.sum[k]);
    }
  } else if (ok) {
    slot = cmap_enter(W, key, (unsigned long long)g, &fresh);
    atomicAdd(&W.fsum[slot], 1ull);
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&W.fsum[(k + 1) * T + slot], (unsigned long long)q[k]);
  }
  if (g < W.in.n) W.slot_of_pt[g] = ok ? slot : -1;
  const unsigned long long freshb = __ballot(fresh);
  if (lane == 0 && okb) {
    atomicAdd(&W.ctl[1], (unsigned long long)__popcll(okb));
    if (freshb) atomicAdd(&W.ctl[0], (unsigned long long)__popcll(freshb));
  }
}

// per point: a voxel's leader numbers it after every earlier leader and writes the closed map's row and table entry (load <= 1/2:
// a free slot is found); the block holding the last point leaves the count
__global__ __launch_bounds__(256) void k_cmap_emit(CmapWork W, long long nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ long long s_bid;
  const int tid = threadIdx.x;
  const long long bid = block_ticket(&W.ctl[2], &s_bid);
  const long long g = bid * 256 + tid;
  const int h = g < W.in.n ? W.slot_of_pt[g] : -1;
  const bool leader = h >= 0 && W.flead[h] == (unsigned long long)g;
  int pos, total;
  block_flag_scan(leader, s_wave, &pos, &total);
  if (tid == 0) s_prefix = lookback_prefix(W.look, bid, (unsigned long long)total, LookFaultDevice{&W.ctl[3]});
  __syncthreads();
  const long long id = (long long)s_prefix + pos;
  if (leader && id < W.row_cap) {
    const VmapTable& P = W.rows;
    const size_t T = (size_t)W.fmask + 1;
    const unsigned long long key = W.fkey[h];
    P.pkey[id] = key;
    P.pn[id] = (long long)W.fsum[h];
    P.pqx[id] = (long long)W.fsum[T + h];
    P.pqy[id] = (long long)W.fsum[2 * T + h];
    P.pqz[id] = (long long)W.fsum[3 * T + h];
    id_table_insert(P.ptab, P.pmask, key, (int)id);
  }
  if (bid == nblocks - 1 && tid == 0) W.ctl[4] = s_prefix + (unsigned long long)total;
}

}  // namespace

int launch_cmap_stage(const CmapWork& W, hipStream_t s) {
  const long long nb = blocks_of((size_t)std::max<long long>(W.in.n, 1));   // (an empty build still launches)
  hipLaunchKernelGGL(k_cmap_clear, dim3(std::min(blocks_of((size_t)W.fmask + 1), 2048u)), dim3(256), 0, s, W, nb);
  hipLaunchKernelGGL(k_cmap_flag, dim3((unsigned)nb), dim3(256), 0, s, W);
  if (W.runs) hipLaunchKernelGGL(k_cmap_stage<true>, dim3((unsigned)nb), dim3(256), 0, s, W);
  else hipLaunchKernelGGL(k_cmap_stage<false>, dim3((unsigned)nb), dim3(256), 0, s, W);
  return 3;
}

int launch_cmap_emit(const CmapWork& W, hipStream_t s) {
  const long long nb = blocks_of((size_t)std::max<long long>(W.in.n, 1));
  hipLaunchKernelGGL(k_cmap_emit, dim3((unsigned)nb), dim3(256), 0, s, W, nb);
  return 1;
}

}  // namespace tl
