// tl_view.hip -- the device side of the closed map's view gain (tl_api_view.hip): per view -- a pose and the
// shared segment ends of a sensor's firing pattern -- the DISTINCT UNKNOWN cells of the frontier field its rays cross before an
// OCCUPIED cell or the box stops them.  Distinct means a set: a bit window of S^3 bits round the view's origin cell, S = 2 W + 1,
// OR-ed by the view's rays and popcounted.
//
// One walk body (view_ray) serves two window homes, a policy that says how a bit is set:
//   LdsHome     the window in the block's dynamic LDS (up to 128 KiB of the CU's 160 by default): a no-return ds_or_b32
//   GlobalHome  the window in device memory: __hip_atomic_fetch_or, relaxed, agent scope
// Launches (nothing of the frontier field, the map or anything else is written):
//   k_view_lds    views x 1024   the LDS form, one block a view: the window zeroed by 16-byte ds_writes, a barrier; the rays strided
//                                over the threads, each ray_begin and the bounded walk of at most n + 1 cells, one tile_index and
//                                one 4-byte load a cell, the counters in registers; a barrier; the popcount strided over the
//                                words; the nine sums folded by shuffles and one LDS round; ONE thread writes the 64-byte record
//                                with plain stores.  No global atomic, no wait on another block
//   k_view_rays   (views of the chunk * blocks_per_view) x 256   the global form: the same walk, a view's rays split over its
//                                blocks (OR is order-free); a block's counters folded and added to the view's by integer atomics
//                                (block_fold)
//   k_view_count  views of the chunk x 256   AFTER the ray launch, never inside it: the popcount of a view's window by plain
//                                loads (the kernel boundary made the ORs visible) and the record
// The cells form (one view) is the same kernels with CELLS: after the popcount the block compacts the set bits in ascending bit
// index -- a thread counts a contiguous range of words, one block scan of the counts, then the scatter of the centres -- one
// block, so no look-back.
// Both forms give the same bytes: every output is an integer (or a centre formed from integers), OR and sum are order-free.
// No run-time indexed private arrays, no scratch.
// Compiled with -ffp-contract=off: the ray's end goes through map_transform_point and the walk through ray_begin (tl_voxel.hpp).
#include <algorithm>

#include "tl_tile.hpp"
#include "tl_voxel.hpp"

namespace tl {
namespace {

struct LdsHome {
  unsigned* win;
  __device__ __forceinline__ void set(unsigned long long word, unsigned mask) const { atomicOr(&win[word], mask); }
};
struct GlobalHome {
  unsigned* win;
  __device__ __forceinline__ void set(unsigned long long word, unsigned mask) const {
    (void)__hip_atomic_fetch_or(&win[word], mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// a thread's counters, named scalars; the records' order is
// [0] unknown visits, [1] free visits, [2] steps, [3] skipped, [4] occupied, [5] left the box, [6] ended, [7] beyond
struct ViewCount {
  unsigned long long unknown = 0ull, free_ = 0ull, steps = 0ull, skipped = 0ull, occupied = 0ull, left = 0ull, ended = 0ull, beyond = 0ull;
};
// One ray of the view at pose M: the walk of the contract (include/tloam_hip.h)
template <class Home>
__device__ __forceinline__ void view_ray(const ViewArgs& A, const double* M, long long r, const Home& home, ViewCount* c) {
  double Ex, Ey, Ez;
  map_transform_point(M, A.ends[3 * r], A.ends[3 * r + 1], A.ends[3 * r + 2], &Ex, &Ey, &Ez);
  RayCells R = {};
  const bool walks = ray_begin(A.grid, A.max_range, M[12], M[13], M[14], Ex, Ey, Ez, &R);
  const int ox = R.cx - A.W, oy = R.cy - A.W, oz = R.cz - A.W;   // (the start cell is c_O)
  const unsigned S = (unsigned)A.S;
  unsigned seen = 0u, unknown = 0u, beyond = 0u;
  int how = 0;   // 0: passed the end cell, 1: an OCCUPIED cell, 2: left the box
  for (int k = 0; walks && k <= R.n; ++k) {
    const long long idx = tile_index(A.f, R.cx, R.cy, R.cz);
    ++seen;
    if (idx < 0) {
      how = 2;
      break;
    }
    const unsigned v = A.f.v[idx];
    if (v == kFrontOccupied) {
      how = 1;
      break;
    }
    if (v == kFrontUnknown) {
      const unsigned dx = (unsigned)(R.cx - ox), dy = (unsigned)(R.cy - oy), dz = (unsigned)(R.cz - oz);
      if (dx < S && dy < S && dz < S) {
        const unsigned long long bit = ((unsigned long long)dz * S + dy) * S + dx;
        home.set(bit >> 5, 1u << (unsigned)(bit & 31ull));
      } else {
        ++beyond;
      }
      ++unknown;
    }
    if (k < R.n) ray_step(&R);
  }
  // every add unconditional (a skipped ray adds zeros but to `skipped`): adds of 1 to one counter or another, picked by a
  // branch, are what the compiler turns into an indexed private array
  c->steps += seen;
  c->unknown += unknown;
  c->free_ += seen - unknown - (how != 0 ? 1u : 0u);   // (every visited cell but the stopping one is unknown or free)
  c->beyond += beyond;
  c->occupied += walks && how == 1 ? 1ull : 0ull;
  c->left += walks && how == 2 ? 1ull : 0ull;
  c->ended += walks && how == 0 ? 1ull : 0ull;
  c->skipped += walks ? 0ull : 1ull;
}

// the sums of v[0 .. N) over a block of NT threads into s_tot[0 .. N) (visible to every thread on return)
template <int NT, int N>
__device__ __forceinline__ void view_fold(const unsigned long long (&v)[N], unsigned long long (*s_part)[N], unsigned long long* s_tot) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned long long w = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) s_part[wave][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    unsigned long long w = 0ull;
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) w += s_part[q][threadIdx.x];
    s_tot[threadIdx.x] = w;
  }
  __syncthreads();
}

// the origin cell of the view at pose M: false when it is none (a translation that is not finite, or beyond the grid)
__device__ __forceinline__ bool view_origin(const ViewArgs& A, const double* M, int* cx, int* cy, int* cz) {
  const double kLimit = (double)(1ll << kVmapBits);
  const double fx = floor((M[12] - A.grid.origin[0]) / A.grid.voxel), fy = floor((M[13] - A.grid.origin[1]) / A.grid.voxel),
               fz = floor((M[14] - A.grid.origin[2]) / A.grid.voxel);
  if (!(fabs(fx) < kLimit && fabs(fy) < kLimit && fabs(fz) < kLimit)) return false;
  *cx = (int)fx; *cy = (int)fy; *cz = (int)fz;
  return true;
}

// the record of view `view`: t[0 .. 7] the counters, `cells` the popcount.  One thread.
__device__ __forceinline__ void view_record(const ViewArgs& A, const double* M, long long view, const unsigned long long* t,
                                            unsigned long long cells) {
  int cx, cy, cz;
  unsigned label = kFrontOutside;
  if (view_origin(A, M, &cx, &cy, &cz)) {
    const long long idx = tile_index(A.f, cx, cy, cz);
    if (idx >= 0) label = A.f.v[idx];
  }
  tloam_closed_map_view_record g;
  g.unknown_cells = (int64_t)cells;
  g.unknown_visits = (int64_t)t[0];
  g.free_visits = (int64_t)t[1];
  g.steps = (int64_t)t[2];
  g.rays_skipped = (int32_t)t[3];
  g.rays_occupied = (int32_t)t[4];
  g.rays_left_box = (int32_t)t[5];
  g.rays_ended = (int32_t)t[6];
  g.origin_label = label;
  g.reserved0 = 0u;
  g.reserved1 = 0;
  A.out[view] = g;
  A.beyond[view] = t[7];
}

// The set bits of the window compacted in ascending bit index and their cells' centres written, at most A.capacity of them: a
// thread takes a contiguous range of words, the block scans the ranges' counts once.  Called by the whole block of NT threads.
template <int NT>
__device__ __forceinline__ void view_compact(const ViewArgs& A, const double* M, const unsigned* win, unsigned long long* s_wave) {
  const long long per = (A.words + NT - 1) / NT;
  const long long w0 = std::min<long long>((long long)threadIdx.x * per, A.words), w1 = std::min<long long>(w0 + per, A.words);
  unsigned long long mine = 0ull;
  for (long long w = w0; w < w1; ++w) mine += (unsigned long long)__popc(win[w]);
  // exclusive scan over the block
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned long long p = incl - mine;
  for (int q = 0; q < wave; ++q) p += s_wave[q];
  int cx, cy, cz;
  if (mine == 0ull || !view_origin(A, M, &cx, &cy, &cz)) return;   // (no bit is set without an origin cell)
  const unsigned long long S = (unsigned long long)A.S;
  for (long long w = w0; w < w1; ++w) {
    unsigned bits = win[w];
    while (bits) {
      const int b = __builtin_ctz(bits);
      bits &= bits - 1u;
      if (p < (unsigned long long)A.capacity) {
        const unsigned long long bit = (unsigned long long)w * 32ull + (unsigned long long)b;
        const unsigned long long row = bit / S, dz = row / S;
        const int x = cx - A.W + (int)(bit - row * S), y = cy - A.W + (int)(row - dz * S), z = cz - A.W + (int)dz;
        A.centres[3 * p] = A.grid.origin[0] + ((double)x + 0.5) * A.grid.voxel;
        A.centres[3 * p + 1] = A.grid.origin[1] + ((double)y + 0.5) * A.grid.voxel;
        A.centres[3 * p + 2] = A.grid.origin[2] + ((double)z + 0.5) * A.grid.voxel;
      }
      ++p;
    }
  }
}

template <bool CELLS>
__global__ __launch_bounds__(kViewLdsThreads) void k_view_lds(ViewArgs A) {
  extern __shared__ uint4 s_window[];
  __shared__ double s_M[16];
  __shared__ unsigned long long s_part[kViewLdsThreads / 64][kViewCounters + 1];
  __shared__ unsigned long long s_tot[kViewCounters + 1];
  __shared__ unsigned long long s_wave[kViewLdsThreads / 64];
  unsigned* win = reinterpret_cast<unsigned*>(s_window);
  const long long view = A.view0 + blockIdx.x;
  const long long quads = (A.words + 3) >> 2;
  for (long long q = threadIdx.x; q < quads; q += kViewLdsThreads) s_window[q] = make_uint4(0u, 0u, 0u, 0u);
  if (threadIdx.x < 16) s_M[threadIdx.x] = A.poses[16 * view + threadIdx.x];
  __syncthreads();
  ViewCount n;
  const LdsHome home{win};
  for (long long r = threadIdx.x; r < A.rays; r += kViewLdsThreads) view_ray(A, s_M, r, home, &n);
  __syncthreads();
  unsigned long long cells = 0ull;
  for (long long w = threadIdx.x; w < A.words; w += kViewLdsThreads) cells += (unsigned long long)__popc(win[w]);
  const unsigned long long c[kViewCounters + 1] = {n.unknown, n.free_, n.steps, n.skipped, n.occupied, n.left, n.ended, n.beyond, cells};
  view_fold<kViewLdsThreads>(c, s_part, s_tot);
  if (threadIdx.x == 0) view_record(A, s_M, view, s_tot, s_tot[kViewCounters]);
  if (CELLS) view_compact<kViewLdsThreads>(A, s_M, win, s_wave);
}

__global__ __launch_bounds__(kViewThreads) void k_view_rays(ViewArgs A) {
  __shared__ double s_M[16];
  const long long local = blockIdx.x / A.bpv;
  const int part = (int)(blockIdx.x - local * A.bpv);
  if (threadIdx.x < 16) s_M[threadIdx.x] = A.poses[16 * (A.view0 + local) + threadIdx.x];
  __syncthreads();
  ViewCount n;
  const GlobalHome home{A.win + (size_t)local * (size_t)A.words};
  const long long stride = (long long)A.bpv * kViewThreads;
  for (long long r = (long long)part * kViewThreads + threadIdx.x; r < A.rays; r += stride) view_ray(A, s_M, r, home, &n);
  unsigned long long v[kViewCounters] = {n.unknown, n.free_, n.steps, n.skipped, n.occupied, n.left, n.ended, n.beyond};
  block_fold<kViewCounters, 0>(v, A.cnt + (size_t)local * kViewCounters);
}

template <bool CELLS>
__global__ __launch_bounds__(kViewThreads) void k_view_count(ViewArgs A) {
  __shared__ double s_M[16];
  __shared__ unsigned long long s_part[kViewThreads / 64][1];
  __shared__ unsigned long long s_tot[1];
  __shared__ unsigned long long s_wave[kViewThreads / 64];
  const long long local = blockIdx.x, view = A.view0 + local;
  const unsigned* win = A.win + (size_t)local * (size_t)A.words;
  if (threadIdx.x < 16) s_M[threadIdx.x] = A.poses[16 * view + threadIdx.x];
  unsigned long long c[1] = {0ull};
  for (long long w = threadIdx.x; w < A.words; w += kViewThreads) c[0] += (unsigned long long)__popc(win[w]);
  view_fold<kViewThreads>(c, s_part, s_tot);   // (its barriers publish s_M too)
  if (threadIdx.x == 0) view_record(A, s_M, view, A.cnt + (size_t)local * kViewCounters, s_tot[0]);
  if (CELLS) view_compact<kViewThreads>(A, s_M, win, s_wave);
}

}  // namespace

size_t view_lds_static() {
  hipFuncAttributes a{}, b{};
  if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_view_lds<false>)) != hipSuccess) return 4096;
  if (hipFuncGetAttributes(&b, reinterpret_cast<const void*>(k_view_lds<true>)) != hipSuccess) return 4096;
  return std::max(a.sharedSizeBytes, b.sharedSizeBytes);
}

hipError_t launch_view_lds(const ViewArgs& A, long long views, bool cells, hipStream_t s) {
  const size_t lds = (size_t)((A.words + 3) >> 2) * 16;
  const void* fn = cells ? reinterpret_cast<const void*>(k_view_lds<true>) : reinterpret_cast<const void*>(k_view_lds<false>);
  // (above 64 KiB a launch needs the attribute; setting it is cheap and idempotent)
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  if (cells) hipLaunchKernelGGL(k_view_lds<true>, dim3((unsigned)views), dim3(kViewLdsThreads), lds, s, A);
  else hipLaunchKernelGGL(k_view_lds<false>, dim3((unsigned)views), dim3(kViewLdsThreads), lds, s, A);
  return hipSuccess;
}

void launch_view_rays(const ViewArgs& A, long long views, hipStream_t s) {
  hipLaunchKernelGGL(k_view_rays, dim3((unsigned)(views * A.bpv)), dim3(kViewThreads), 0, s, A);
}

void launch_view_count(const ViewArgs& A, long long views, bool cells, hipStream_t s) {
  if (cells) hipLaunchKernelGGL(k_view_count<true>, dim3((unsigned)views), dim3(kViewThreads), 0, s, A);
  else hipLaunchKernelGGL(k_view_count<false>, dim3((unsigned)views), dim3(kViewThreads), 0, s, A);
}

}  // namespace tl
