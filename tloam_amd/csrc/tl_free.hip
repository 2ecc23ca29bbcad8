// tl_free.hip -- the device side of the closed map's free space (tl_api_free.hip): a dense grid of bricks
// of 4 x 4 x 4 cells of the closed map's grid, one 64-bit word a brick, bit ((cz & 3) << 4) | ((cy & 3) << 2) | (cx & 3) set when
// a ray saw through the cell.  Brick of a cell: c >> 2 per axis (an arithmetic shift: negative cells floor).
//
// Launches (no host synchronisation between those of one call; nothing of the closed map, of a carve's counts, of the surfels or
// of a diff's counts is written):
//   k_free_clear     grid x 256   zeroes the words (a reset)
//   k_free_rays      grid x 256   a thread per ray: the carve's set-up and step (tl_voxel.hpp: ray_begin, ray_step) and NO lookup in
//   k_free_rays_scan              the map's table; the lane keeps the current brick's index and the bits gathered in it in registers
//                                 and flushes when the walk enters another brick, leaves the box or ends: a plain load of the word,
//                                 and a no-return 64-bit atomic OR only when (word & bits) != bits (bits are only ever set: a stale
//                                 read costs a redundant atomic, never a wrong bit).  The counters summed over the wave by
//                                 shuffles, one atomic per counter and wave.  Two entry points over one body: the keyframes'
//                                 spans (span_point, the carve's rays) and one origin (the diff's rays)
//   k_free_count     grid x 256   popcount of the words and the nonzero words: a wave sum, one atomic per counter and wave
//   k_free_points    grid x 256   the occupancy of a point: one cell_voxel, the carve gate (tl_common.hpp: CarveGate), one word
//                                 read; the states counted by ballot (wave_count_states)
//   k_free_cells     grid x 256   a thread per brick: the bits of the cells that pass (free, not a counting voxel, in the metric
//                                 box), their popcount scanned over the block (block_packed_scan) and the blocks (lookback_prefix
//                                 over start tickets), the centres scattered: brick index ascending, then bit ascending
//   k_free_columns   grid x 256   a thread per column of the box's x-y footprint over a band of z cells
// No block waits on another block except in k_free_cells' look-back (bounded: tl_voxel.hpp).  No floating-point atomics, no
// run-time indexed arrays; no loop of a ray runs longer than the ray's own n.
//
// Compiled with -ffp-contract=off.  The free condition (tests/closed_map_free_np.py restates it): the ray's set-up is
// tl_carve.hip's header word for word.  The visited cells are the carve's: the start cell and the first n - 1 cells stepped into.
// Each has an entry parameter t_in: 0 for the start cell, otherwise the tMax of the axis the step into it took, read before the
// step updates it (the smallest tMax then).  tlim = 1.0 - end_margin / L.  A visited cell is marked when t_in < tlim, whether or
// not the map has a voxel there; t_in never decreases, so the walk stops at the first cell that fails.  A ray with L <= end_margin
// marks nothing.  A marked cell inside the box sets its bit and counts in cells_marked; one outside only counts, in cells_outside.
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__global__ __launch_bounds__(256) void k_free_clear(FreeGrid g) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  for (long long t = i; t < g.nwords; t += stride) g.words[t] = 0ull;
}

// the word of brick `idx` gains `bits`
__device__ __forceinline__ void free_flush(const FreeGrid& g, long long idx, unsigned long long bits) {
  if (idx < 0) return;
  const unsigned long long w = g.words[idx];
  if ((w & bits) != bits) (void)__hip_atomic_fetch_or(&g.words[idx], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one ray from O to E: *skipped, *marked, *outside are set for it (a skipped ray: 1, 0, 0)
__device__ __forceinline__ void free_ray(const FreeWork& W, double Ox, double Oy, double Oz, double Ex, double Ey, double Ez,
                                         unsigned long long* skipped, unsigned long long* marked, unsigned long long* outside) {
  RayCells R;
  if (!ray_begin(W.grid, W.max_range, Ox, Oy, Oz, Ex, Ey, Ez, &R)) {
    *skipped = 1ull;
    return;
  }
  const double tlim = 1.0 - W.end_margin / R.L;
  double t_in = 0.0;
  long long cur = -1;
  unsigned long long bits = 0ull, in = 0ull, out = 0ull;
  for (int k = 0; k < R.n; ++k) {
    if (!(t_in < tlim)) break;
    const long long idx = free_brick(W.g, R.cx, R.cy, R.cz);
    if (idx != cur) {
      free_flush(W.g, cur, bits);
      cur = idx;
      bits = 0ull;
    }
    if (idx >= 0) {
      bits |= free_bit(R.cx, R.cy, R.cz);
      ++in;
    } else {
      ++out;
    }
    t_in = ray_next_t(R);
    ray_step(&R);
  }
  free_flush(W.g, cur, bits);
  *marked = in;
  *outside = out;
}

__device__ __forceinline__ void free_post(const FreeWork& W, unsigned long long skipped, unsigned long long marked,
                                          unsigned long long outside) {
  wave_add(&W.ctl[0], skipped);
  wave_add(&W.ctl[1], marked);
  wave_add(&W.ctl[2], outside);
}

__global__ __launch_bounds__(256) void k_free_rays(FreeWork W) {
  __shared__ int s_span[2];
  block_spans(W.in, s_span);
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long skipped = 0ull, marked = 0ull, outside = 0ull;
  if (g < W.in.n) {
    int kf;
    const double* P;
    double E[3];
    span_point(W.in, g, s_span[0], s_span[1], &kf, &P, E);
    free_ray(W, P[12], P[13], P[14], E[0], E[1], E[2], &skipped, &marked, &outside);
  }
  free_post(W, skipped, marked, outside);
}

__global__ __launch_bounds__(256) void k_free_rays_scan(FreeWork W) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  unsigned long long skipped = 0ull, marked = 0ull, outside = 0ull;
  if (g < W.scan.n) {
    const double* M = W.scan.M;
    double E[3];
    map_transform_point(M, W.scan.pts[3 * g], W.scan.pts[3 * g + 1], W.scan.pts[3 * g + 2], &E[0], &E[1], &E[2]);
    free_ray(W, M[12], M[13], M[14], E[0], E[1], E[2], &skipped, &marked, &outside);
  }
  free_post(W, skipped, marked, outside);
}

__global__ __launch_bounds__(256) void k_free_count(FreeWork W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  unsigned long long cells = 0ull, bricks = 0ull;
  for (long long t = i; t < W.g.nwords; t += stride) {
    const unsigned long long w = W.g.words[t];
    cells += (unsigned long long)__popcll(w);
    bricks += w ? 1ull : 0ull;
  }
  wave_add(&W.ctl[3], cells);
  wave_add(&W.ctl[4], bricks);
}

__global__ __launch_bounds__(256) void k_free_points(FreePointsArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < A.scan.n;
  int state = TLOAM_OCCUPANCY_INVALID;
  if (live) {
    double E[3] = {A.scan.pts[3 * g], A.scan.pts[3 * g + 1], A.scan.pts[3 * g + 2]};
    if (A.posed) map_transform_point(A.scan.M, E[0], E[1], E[2], &E[0], &E[1], &E[2]);
    unsigned long long key;
    unsigned qq[3];
    int id = -1;
    if (vmap_quantise(E, A.q.grid.origin, A.q.grid.voxel, &key, qq) == kVmapInside) {
      const int cx = (int)key_axis(key, 0), cy = (int)key_axis(key, 1), cz = (int)key_axis(key, 2);
      state = free_cell_state(A.q, cx, cy, cz, &id);
    }
    A.state[g] = (unsigned char)state;
    if (A.ids) A.ids[g] = id;
  }
  wave_count_states(live, state, A.ctl);
}

__global__ __launch_bounds__(256) void k_free_cells(FreeCellsArgs A, int nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const int tid = threadIdx.x;
  const int bid = block_ticket(&A.ctl[0], &s_bid);
  const FreeGrid& g = A.q.g;
  const MapGrid& G = A.q.grid;
  const long long i = (long long)bid * 256 + tid;
  unsigned long long pass = 0ull;
  int x0 = 0, y0 = 0, z0 = 0;
  if (i < g.nwords) {
    unsigned long long rem = g.words[i];
    if (rem) {
      const long long plane = i / g.nb[0];
      x0 = ((int)(i - plane * g.nb[0]) + g.blo[0]) * 4;
      y0 = ((int)(plane % g.nb[1]) + g.blo[1]) * 4;
      z0 = ((int)(plane / g.nb[1]) + g.blo[2]) * 4;
    }
    while (rem) {   // (at most 64 rounds: a bit goes each)
      const int b = __builtin_ctzll(rem);
      rem &= rem - 1ull;
      const int cx = x0 + (b & 3), cy = y0 + ((b >> 2) & 3), cz = z0 + (b >> 4);
      if (free_counting_voxel(A.q, cx, cy, cz) >= 0) continue;
      if (A.boxed) {
        const double px = G.origin[0] + ((double)cx + 0.5) * G.voxel, py = G.origin[1] + ((double)cy + 0.5) * G.voxel,
                     pz = G.origin[2] + ((double)cz + 0.5) * G.voxel;
        if (!(px >= A.lo[0] && px <= A.hi[0] && py >= A.lo[1] && py <= A.hi[1] && pz >= A.lo[2] && pz <= A.hi[2])) continue;
      }
      pass |= 1ull << b;
    }
  }
  unsigned long long before, total;
  block_packed_scan((unsigned long long)__popcll(pass), s_wave, &before, &total);
  if (tid == 0) s_prefix = lookback_prefix(A.look, bid, total, LookFaultDevice{&A.ctl[1]});
  __syncthreads();
  size_t p = (size_t)(s_prefix + before);
  while (pass) {
    const int b = __builtin_ctzll(pass);
    pass &= pass - 1ull;
    A.out_c[3 * p] = G.origin[0] + ((double)(x0 + (b & 3)) + 0.5) * G.voxel;
    A.out_c[3 * p + 1] = G.origin[1] + ((double)(y0 + ((b >> 2) & 3)) + 0.5) * G.voxel;
    A.out_c[3 * p + 2] = G.origin[2] + ((double)(z0 + (b >> 4)) + 0.5) * G.voxel;
    ++p;
  }
  if (bid == nblocks - 1 && tid == 0) A.ctl[2] = s_prefix + total;
}

__global__ __launch_bounds__(256) void k_free_columns(FreeColumnsArgs A) {
  const FreeGrid& g = A.q.g;
  const long long nx = 4ll * g.nb[0], ny = 4ll * g.nb[1];
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  if (col >= nx * ny) return;
  const int cx = 4 * g.blo[0] + (int)(col % nx), cy = 4 * g.blo[1] + (int)(col / nx);
  long long free_cells = 0;
  bool occupied = false;
  for (int cz = A.z0; cz <= A.z1; ++cz) {
    if (free_counting_voxel(A.q, cx, cy, cz) >= 0) {
      occupied = true;
      break;
    }
    const long long idx = free_brick(g, cx, cy, cz);
    if (idx >= 0 && (g.words[idx] & free_bit(cx, cy, cz)) != 0ull) ++free_cells;
  }
  A.state[col] = (unsigned char)(occupied ? TLOAM_OCCUPANCY_OCCUPIED
                                          : free_cells >= A.min_free ? TLOAM_OCCUPANCY_FREE : TLOAM_OCCUPANCY_UNKNOWN);
}

}  // namespace

int launch_free_clear(const FreeGrid& g, hipStream_t s) {
  const unsigned blocks = blocks_of((size_t)std::max<long long>(g.nwords, 1));
  hipLaunchKernelGGL(k_free_clear, dim3(std::min(blocks, 4096u)), dim3(256), 0, s, g);
  return 1;
}

int launch_free_rays(const FreeWork& W, bool spans, hipStream_t s) {
  const unsigned n_blocks = blocks_of((size_t)std::max<long long>(spans ? W.in.n : W.scan.n, 1));   // (nothing still launches)
  if (spans) hipLaunchKernelGGL(k_free_rays, dim3(n_blocks), dim3(256), 0, s, W);
  else hipLaunchKernelGGL(k_free_rays_scan, dim3(n_blocks), dim3(256), 0, s, W);
  const unsigned w_blocks = blocks_of((size_t)std::max<long long>(W.g.nwords, 1));
  hipLaunchKernelGGL(k_free_count, dim3(std::min(w_blocks, 2048u)), dim3(256), 0, s, W);
  return 2;
}

void launch_free_points(const FreePointsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_free_points, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

void launch_free_cells(const FreeCellsArgs& A, hipStream_t s) {
  const int nb = (int)blocks_of((size_t)std::max<long long>(A.q.g.nwords, 1));
  hipLaunchKernelGGL(k_free_cells, dim3(nb), dim3(256), 0, s, A, nb);
}

void launch_free_columns(const FreeColumnsArgs& A, hipStream_t s) {
  const long long cols = 16ll * A.q.g.nb[0] * A.q.g.nb[1];
  hipLaunchKernelGGL(k_free_columns, dim3(blocks_of((size_t)std::max<long long>(cols, 1))), dim3(256), 0, s, A);
}

}  // namespace tl
