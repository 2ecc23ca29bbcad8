// tl_clear.hip -- the device side of the closed map's clearance (tl_api_clear.hip): a dense field of
// uint16 over the free-space grid's box, [z][y][x], x fastest: d2, the squared distance in cells from a cell to the nearest
// obstacle cell, exact up to R * R and kClearBeyond above (R <= 128: every sum below fits 16 bits beside the two sentinels).
//
// Launches (no host synchronisation between those of one call; nothing of the closed map, of a carve's counts, of the surfels, of
// a diff's counts or of the free-space grid is written):
//   k_clear_seed      grid x 256   a thread per four cells along x: the brick's word read, 0 (obstacle) or 0xFFFF written -- with
//                                  `wrap` (unknown_is_obstacle) an unset bit is an obstacle, without it no bit is
//   k_clear_voxels    grid x 256   a thread per voxel row of the map: one that counts (CarveGate) and lies in the box writes 0
//   k_clear_x         grid x 256   a wave per window of 512 cells of a row: the nearest obstacle at or before and at or after each
//                                  cell by a max and a min scan of positions over the wave (shuffles), i * i written for
//                                  |i| <= R.  The window's halo of roundup4(R) cells on both sides is loaded again by its
//                                  neighbours: no carry between waves, no loop over a row
//   k_clear_axis      grid x 256   the pass along y (outer = nz, n = ny, inner = nx) and along z (outer = 1, n = nz, inner =
//                                  nx * ny: a plane is one contiguous line): out(t) = min over |j| <= R of g(t + j) + j * j, a
//                                  windowed minimum of 2 R + 1 taps.  A block stages a strip of kClearTile + 2 R positions of the
//                                  pass axis by 64 cells of the contiguous axis in LDS (8 bytes a lane, 128 bytes a strip row) and
//                                  each thread gives four outputs of four cells.  The last pass clamps what exceeds R * R
//   k_clear_count     grid x 256   obstacle cells, finite cells, the sum and the largest d2: a wave sum (a wave max), the block's
//                                  four waves through LDS, one atomic per counter and block, at most 512 blocks
//   k_clear_points    grid x 256   a thread per point: k_free_points' state and the cell's value
//   k_clear_segments  grid x 256   a thread per segment: ray_begin / ray_step, one 2-byte read a cell, no table probe
//   k_clear_col_seed  grid x 256   a column's state (k_free_columns') made 0 or 0xFFFF; then k_clear_x and k_clear_axis on the
//                                  one layer
// Outside the box: with `wrap` every position outside reads 0 (an obstacle) in every pass -- the box behaves as wrapped in one
// layer of obstacles, and the nearest outside cell of an inside cell lies in that layer; without it, 0xFFFF.
// No block waits on another.  No floating-point atomics, no run-time indexed private arrays, no scratch.
// Compiled with -ffp-contract=off (tl_voxel.hpp asks for it: the segments' ray set-up is tl_carve.hip's header word for word).
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

constexpr int kBig = 1 << 28;            // a position no window holds, and a distance beyond every R
constexpr unsigned kInf16 = 0xFFFFu;

// four cells of a row as they are stored: 8 bytes, the lowest cell in the low half of .x
__device__ __forceinline__ uint2 pack4(unsigned a, unsigned b, unsigned c, unsigned d) { return make_uint2(a | (b << 16), c | (d << 16)); }
__device__ __forceinline__ unsigned cell_of(const uint2& v, int j) {   // (j is a compile-time constant at every call)
  return j == 0 ? v.x & 0xFFFFu : j == 1 ? v.x >> 16 : j == 2 ? v.y & 0xFFFFu : v.y >> 16;
}

__global__ __launch_bounds__(256) void k_clear_seed(ClearBuildArgs A) {
  const FreeGrid& g = A.q.g;
  const long long groups = A.f.cells >> 2, stride = (long long)gridDim.x * 256;
  const long long ny = A.f.n[1];
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const long long row = t / g.nb[0];
    const int bx = (int)(t - row * g.nb[0]);
    const long long z = row / ny;
    const int y = (int)(row - z * ny);
    unsigned bits = 0xFu;   // (no bit an obstacle)
    if (A.f.wrap) {
      const unsigned long long w = g.words[((z >> 2) * g.nb[1] + (y >> 2)) * g.nb[0] + bx];
      bits = (unsigned)(w >> ((((int)z & 3) << 4) | ((y & 3) << 2))) & 0xFu;
    }
    reinterpret_cast<uint2*>(A.tmp)[t] = pack4(bits & 1u ? kInf16 : 0u, bits & 2u ? kInf16 : 0u, bits & 4u ? kInf16 : 0u,
                                               bits & 8u ? kInf16 : 0u);
  }
}

// the index of cell (cx, cy, cz) in the field, -1 outside the box
__device__ __forceinline__ long long clear_index(const ClearField& f, int cx, int cy, int cz) {
  const unsigned x = (unsigned)(cx - f.lo[0]), y = (unsigned)(cy - f.lo[1]), z = (unsigned)(cz - f.lo[2]);
  if (!(x < (unsigned)f.n[0] && y < (unsigned)f.n[1] && z < (unsigned)f.n[2])) return -1;
  return ((long long)z * f.n[1] + (long long)y) * f.n[0] + (long long)x;
}
// the value a query reads at cell (cx, cy, cz)
__device__ __forceinline__ unsigned clear_value(const ClearField& f, int cx, int cy, int cz, bool* outside) {
  const long long idx = clear_index(f, cx, cy, cz);
  *outside = idx < 0;
  return idx < 0 ? (f.wrap ? 0u : (unsigned)kClearOutside) : (unsigned)f.d2[idx];
}

__global__ __launch_bounds__(256) void k_clear_voxels(ClearBuildArgs A) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= A.q.grid.nv) return;
  const VmapTableView& map = A.q.grid.map;
  if (!A.q.gate.counts(map, (int)id)) return;
  const unsigned long long key = map.pkey[id];
  const long long idx = clear_index(A.f, (int)key_axis(key, 0), (int)key_axis(key, 1), (int)key_axis(key, 2));
  if (idx >= 0) A.tmp[idx] = 0;
}

// inclusive scans over the wave's lanes, lane 0 first (max) and lane 63 first (min)
__device__ __forceinline__ int wave_scan_max_up(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(v, off, 64);
    if (lane >= off) v = max(v, t);
  }
  return v;
}
__device__ __forceinline__ int wave_scan_min_down(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_down(v, off, 64);
    if (lane + off < 64) v = min(v, t);
  }
  return v;
}

// A row's window of 512 cells held by a wave: lane l has the cells p0 .. p0 + 3 of `v`, p0 the position in the window of its
// first cell.  before / after: the position of the nearest obstacle (value 0) in the lanes' groups before / after this one's
// (-kBig / kBig: none).  The four results: min(i * i) over the obstacles within R, kInf16 without one.
__device__ __forceinline__ uint2 x_distances(const uint2& v, int p0, int before, int after, int R) {
  const bool o0 = cell_of(v, 0) == 0u, o1 = cell_of(v, 1) == 0u, o2 = cell_of(v, 2) == 0u, o3 = cell_of(v, 3) == 0u;
  const int l0 = o0 ? p0 : before, l1 = o1 ? p0 + 1 : l0, l2 = o2 ? p0 + 2 : l1, l3 = o3 ? p0 + 3 : l2;
  const int n3 = o3 ? p0 + 3 : after, n2 = o2 ? p0 + 2 : n3, n1 = o1 ? p0 + 1 : n2, n0 = o0 ? p0 : n1;
  const int d0 = min(p0 - l0, n0 - p0), d1 = min(p0 + 1 - l1, n1 - (p0 + 1)), d2 = min(p0 + 2 - l2, n2 - (p0 + 2)),
            d3 = min(p0 + 3 - l3, n3 - (p0 + 3));
  return pack4(d0 <= R ? (unsigned)(d0 * d0) : kInf16, d1 <= R ? (unsigned)(d1 * d1) : kInf16,
               d2 <= R ? (unsigned)(d2 * d2) : kInf16, d3 <= R ? (unsigned)(d3 * d3) : kInf16);
}

// rows of nx cells (nx a multiple of 4), `rows` of them, src -> dst.  H = roundup4(R) <= 128, a window gives T = 512 - 2 H cells
__global__ __launch_bounds__(256) void k_clear_x(const unsigned short* __restrict__ src, unsigned short* __restrict__ dst, int nx,
                                                 long long rows, int R, int wrap) {
  const int lane = threadIdx.x & 63;
  const int H = (R + 3) & ~3, T = 512 - 2 * H;
  const long long chunks = (nx + T - 1) / T, windows = rows * chunks;
  const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), wstride = (long long)gridDim.x * 4;
  const unsigned fill = wrap ? 0u : kInf16;
  const uint2 fill4 = pack4(fill, fill, fill, fill);
  for (long long w = wave0; w < windows; w += wstride) {   // (wave-uniform: the shuffles below run with every lane)
    const long long row = w / chunks;
    const int c0 = (int)(w - row * chunks) * T;            // the first cell this window writes
    const int xa = c0 - H + 4 * lane, xb = xa + 256;       // the lane's two groups of four cells
    const unsigned short* line = src + row * nx;
    uint2 va = fill4, vb = fill4;   // (assigned under the test, not selected: a select of two aggregates went through scratch)
    if (xa >= 0 && xa < nx) va = *reinterpret_cast<const uint2*>(line + xa);
    if (xb >= 0 && xb < nx) vb = *reinterpret_cast<const uint2*>(line + xb);
    // the last / first obstacle of each group, as positions in the window
    const int pa = 4 * lane, pb = 256 + 4 * lane;
    const int la = cell_of(va, 3) == 0u ? pa + 3 : cell_of(va, 2) == 0u ? pa + 2 : cell_of(va, 1) == 0u ? pa + 1
                   : cell_of(va, 0) == 0u ? pa : -kBig;
    const int lb = cell_of(vb, 3) == 0u ? pb + 3 : cell_of(vb, 2) == 0u ? pb + 2 : cell_of(vb, 1) == 0u ? pb + 1
                   : cell_of(vb, 0) == 0u ? pb : -kBig;
    const int fa = cell_of(va, 0) == 0u ? pa : cell_of(va, 1) == 0u ? pa + 1 : cell_of(va, 2) == 0u ? pa + 2
                   : cell_of(va, 3) == 0u ? pa + 3 : kBig;
    const int fb = cell_of(vb, 0) == 0u ? pb : cell_of(vb, 1) == 0u ? pb + 1 : cell_of(vb, 2) == 0u ? pb + 2
                   : cell_of(vb, 3) == 0u ? pb + 3 : kBig;
    const int sla = wave_scan_max_up(la, lane), slb = wave_scan_max_up(lb, lane);
    const int sfa = wave_scan_min_down(fa, lane), sfb = wave_scan_min_down(fb, lane);
    const int all_la = __shfl(sla, 63, 64), all_fb = __shfl(sfb, 0, 64);
    int before_a = __shfl_up(sla, 1, 64), before_b = __shfl_up(slb, 1, 64);
    int after_a = __shfl_down(sfa, 1, 64), after_b = __shfl_down(sfb, 1, 64);
    if (lane == 0) { before_a = -kBig; before_b = -kBig; }
    if (lane == 63) { after_a = kBig; after_b = kBig; }
    before_b = max(before_b, all_la);                      // group b comes after every group a
    after_a = min(after_a, all_fb);
    const int end = min(c0 + T, nx);
    unsigned short* out = dst + row * nx;
    if (xa >= c0 && xa < end) *reinterpret_cast<uint2*>(out + xa) = x_distances(va, pa, before_a, after_a, R);
    if (xb >= c0 && xb < end) *reinterpret_cast<uint2*>(out + xb) = x_distances(vb, pb, before_b, after_b, R);
  }
}

// src, dst: [outer][n][inner], inner contiguous and a multiple of 4; the pass runs along n.  A block: 16 lanes of four cells
// along inner by 16 rows; the strip in LDS is (kClearTile + 2 R) rows of 16 x 8 bytes, row r the position t0 - R + r.
// final: what exceeds R * R becomes kClearBeyond.
__global__ __launch_bounds__(256) void k_clear_axis(const unsigned short* __restrict__ src, unsigned short* __restrict__ dst,
                                                    long long outer, int n, long long inner, int R, int wrap, int final) {
  extern __shared__ uint2 strip[];   // [kClearTile + 2 R][16]
  const int gx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const long long inner4 = inner >> 2, gtiles = (inner4 + 15) / 16;
  const long long ttiles = (n + kClearTile - 1) / kClearTile;
  const long long tiles = outer * ttiles * gtiles;
  const unsigned fill = wrap ? 0u : kInf16;
  const uint2 fill4 = pack4(fill, fill, fill, fill);
  const unsigned limit = final ? (unsigned)(R * R) : kInf16 - 1u;
  for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {
    const long long gt = b % gtiles, rest = b / gtiles;
    const int t0 = (int)(rest % ttiles) * kClearTile;
    const long long o = rest / ttiles;
    const long long g = gt * 16 + gx;            // this lane's group of four cells along inner
    const bool live = g < inner4;
    const int rows_out = min(kClearTile, n - t0);
    const unsigned short* base = src + o * n * inner + 4 * g;
    for (int r = ry; r < rows_out + 2 * R; r += 16) {
      const int t = t0 - R + r;
      uint2 v = fill4;
      if (live && t >= 0 && t < n) v = *reinterpret_cast<const uint2*>(base + (long long)t * inner);
      strip[r * 16 + gx] = v;
    }
    __syncthreads();
    for (int t = ry; t < rows_out; t += 16) {
      unsigned a0 = kInf16, a1 = kInf16, a2 = kInf16, a3 = kInf16;
      for (int j = -R; j <= R; ++j) {
        const uint2 v = strip[(t + R + j) * 16 + gx];
        const unsigned c = (unsigned)(j * j);
        a0 = min(a0, cell_of(v, 0) + c);
        a1 = min(a1, cell_of(v, 1) + c);
        a2 = min(a2, cell_of(v, 2) + c);
        a3 = min(a3, cell_of(v, 3) + c);
      }
      if (live)
        *reinterpret_cast<uint2*>(dst + (o * n + t0 + t) * inner + 4 * g) =
            pack4(a0 > limit ? kInf16 : a0, a1 > limit ? kInf16 : a1, a2 > limit ? kInf16 : a2, a3 > limit ? kInf16 : a3);
    }
    __syncthreads();   // (the strip is free for the next tile)
  }
}

__global__ __launch_bounds__(256) void k_clear_count(const unsigned short* __restrict__ d2, long long cells, unsigned long long* ctl) {
  const long long groups = cells >> 2, stride = (long long)gridDim.x * 256;
  unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};   // obstacles, finite cells, their sum; the largest
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const uint2 v = reinterpret_cast<const uint2*>(d2)[t];
    const unsigned c0 = cell_of(v, 0), c1 = cell_of(v, 1), c2 = cell_of(v, 2), c3 = cell_of(v, 3);
    c[0] += (c0 == 0u) + (c1 == 0u) + (c2 == 0u) + (c3 == 0u);
    const unsigned f0 = c0 != kInf16 ? c0 : 0u, f1 = c1 != kInf16 ? c1 : 0u, f2 = c2 != kInf16 ? c2 : 0u, f3 = c3 != kInf16 ? c3 : 0u;
    c[1] += (c0 != kInf16) + (c1 != kInf16) + (c2 != kInf16) + (c3 != kInf16);
    c[2] += (unsigned long long)f0 + f1 + f2 + f3;
    c[3] = max(c[3], (unsigned long long)max(max(f0, f1), max(f2, f3)));
  }
  block_fold<3, 1>(c, ctl);
}

__global__ __launch_bounds__(256) void k_clear_points(ClearPointsArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < A.scan.n;
  int state = TLOAM_OCCUPANCY_INVALID;
  if (live) {
    double E[3] = {A.scan.pts[3 * g], A.scan.pts[3 * g + 1], A.scan.pts[3 * g + 2]};
    if (A.posed) map_transform_point(A.scan.M, E[0], E[1], E[2], &E[0], &E[1], &E[2]);
    unsigned long long key;
    unsigned qq[3];
    unsigned d2 = kClearOutside;
    if (vmap_quantise(E, A.q.grid.origin, A.q.grid.voxel, &key, qq) == kVmapInside) {
      const int cx = (int)key_axis(key, 0), cy = (int)key_axis(key, 1), cz = (int)key_axis(key, 2);
      int id;
      bool outside;
      state = free_cell_state(A.q, cx, cy, cz, &id);
      d2 = clear_value(A.f, cx, cy, cz, &outside);
    }
    A.state[g] = (unsigned char)state;
    A.d2[g] = (unsigned short)d2;
    if (A.distance)
      A.distance[g] = d2 == kClearBeyond ? __builtin_huge_val() : d2 == kClearOutside ? __builtin_nan("") : A.q.grid.voxel * sqrt((double)d2);
  }
  wave_count_states(live, state, A.ctl);
}

__global__ __launch_bounds__(256) void k_clear_segments(ClearSegmentsArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < A.scan.n;
  int status = TLOAM_CLEARANCE_SKIPPED;
  if (live) {
    double S[3] = {A.starts[3 * g], A.starts[3 * g + 1], A.starts[3 * g + 2]};
    double E[3] = {A.scan.pts[3 * g], A.scan.pts[3 * g + 1], A.scan.pts[3 * g + 2]};
    if (A.posed) {
      map_transform_point(A.scan.M, S[0], S[1], S[2], &S[0], &S[1], &S[2]);
      map_transform_point(A.scan.M, E[0], E[1], E[2], &E[0], &E[1], &E[2]);
    }
    unsigned least = kClearOutside;
    double t_block = -1.0;
    RayCells R;
    if (ray_begin(A.grid, A.max_segment, S[0], S[1], S[2], E[0], E[1], E[2], &R)) {
      status = TLOAM_CLEARANCE_CLEAR;
      least = kClearBeyond;
      double t_in = 0.0;
      for (int k = 0; k <= R.n; ++k) {
        bool outside;
        const unsigned d2 = clear_value(A.f, R.cx, R.cy, R.cz, &outside);
        if (outside && !A.f.wrap) {
          status = TLOAM_CLEARANCE_LEFT_BOX;
          t_block = t_in;
          break;
        }
        least = min(least, d2);
        if ((int)d2 < A.need) {
          status = TLOAM_CLEARANCE_BLOCKED;
          t_block = t_in;
          break;
        }
        if (k < R.n) {
          t_in = ray_next_t(R);
          ray_step(&R);
        }
      }
    }
    A.status[g] = (unsigned char)status;
    A.min_d2[g] = (unsigned short)least;
    if (A.t_block) A.t_block[g] = t_block;
  }
  wave_count_states(live, status, A.ctl);
}

__global__ __launch_bounds__(256) void k_clear_col_seed(ClearColumnsArgs A) {
  const long long groups = ((long long)A.nx * A.ny) >> 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= groups) return;
  const uchar4 s = reinterpret_cast<const uchar4*>(A.state)[t];
  const unsigned u = A.wrap ? TLOAM_OCCUPANCY_UNKNOWN : TLOAM_OCCUPANCY_OCCUPIED;   // (without wrap: OCCUPIED twice)
  reinterpret_cast<uint2*>(A.out)[t] = pack4(s.x == TLOAM_OCCUPANCY_OCCUPIED || s.x == u ? 0u : kInf16,
                                             s.y == TLOAM_OCCUPANCY_OCCUPIED || s.y == u ? 0u : kInf16,
                                             s.z == TLOAM_OCCUPANCY_OCCUPIED || s.z == u ? 0u : kInf16,
                                             s.w == TLOAM_OCCUPANCY_OCCUPIED || s.w == u ? 0u : kInf16);
}

unsigned capped_blocks(long long blocks) {   // at least one block, at most 2^20 (the kernels stride over the rest)
  return (unsigned)std::min<long long>(std::max<long long>(blocks, 1), 1ll << 20);
}

void launch_x(const unsigned short* src, unsigned short* dst, int nx, long long rows, int R, int wrap, hipStream_t s) {
  const int T = 512 - 2 * ((R + 3) & ~3);
  const long long windows = rows * ((nx + T - 1) / T);
  hipLaunchKernelGGL(k_clear_x, dim3(capped_blocks((windows + 3) / 4)), dim3(256), 0, s, src, dst, nx, rows, R, wrap);
}

void launch_axis(const unsigned short* src, unsigned short* dst, long long outer, int n, long long inner, int R, int wrap, int final,
                 hipStream_t s) {
  const long long tiles = outer * ((n + kClearTile - 1) / kClearTile) * (((inner >> 2) + 15) / 16);
  const size_t lds = (size_t)(kClearTile + 2 * R) * 16 * sizeof(uint2);   // <= 40 960 bytes at R = 128
  hipLaunchKernelGGL(k_clear_axis, dim3(capped_blocks(tiles)), dim3(256), lds, s, src, dst, outer, n, inner, R, wrap, final);
}

}  // namespace

int launch_clear_build(const ClearBuildArgs& A, hipStream_t s) {
  const ClearField& f = A.f;
  const long long groups = f.cells >> 2;
  hipLaunchKernelGGL(k_clear_seed, dim3(std::min(blocks_of((size_t)groups), 4096u)), dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_clear_voxels, dim3(blocks_of((size_t)std::max<long long>(A.q.grid.nv, 1))), dim3(256), 0, s, A);
  launch_x(A.tmp, A.out, f.n[0], (long long)f.n[1] * f.n[2], f.R, f.wrap, s);
  launch_axis(A.out, A.tmp, f.n[2], f.n[1], f.n[0], f.R, f.wrap, 0, s);
  launch_axis(A.tmp, A.out, 1, f.n[2], (long long)f.n[0] * f.n[1], f.R, f.wrap, 1, s);
  hipLaunchKernelGGL(k_clear_count, dim3(std::min(blocks_of((size_t)groups), 512u)), dim3(256), 0, s, A.out, f.cells, A.ctl);
  return 6;
}

void launch_clear_points(const ClearPointsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_clear_points, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

void launch_clear_segments(const ClearSegmentsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_clear_segments, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

int launch_clear_columns(const ClearColumnsArgs& A, hipStream_t s) {
  const long long groups = ((long long)A.nx * A.ny) >> 2;
  hipLaunchKernelGGL(k_clear_col_seed, dim3(blocks_of((size_t)groups)), dim3(256), 0, s, A);
  launch_x(A.out, A.tmp, A.nx, A.ny, A.R, A.wrap, s);
  launch_axis(A.tmp, A.out, 1, A.ny, A.nx, A.R, A.wrap, 1, s);
  return 3;
}

}  // namespace tl
