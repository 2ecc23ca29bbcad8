// tl_route.hip -- the device side of the route through the closed map (tl_api_route.hip): a dense field of
// uint32 over the clearance field's box, [z][y][x], x fastest: the least total 3-4-5 chamfer weight of a chain of 26-connected
// moves over traversable cells to an accepted goal; kRouteUnreached where no goal reaches, kRouteBlocked where the cell is not
// traversable (its d2 < max(need, 1)).  The column form is the same kernels over a layer, n[2] = 1: what lies above and below is
// outside the box, so 8 moves of weight 3 and 4 remain.
//
// Launches (nothing of the closed map, the free-space grid or the clearance field is written):
//   k_route_seed     grid x 256   a thread per four cells along x: d2 read, kRouteUnreached or kRouteBlocked written
//   k_route_goals    grid x 256   a thread per goal: the point's cell, 0 written when it is traversable, its tile flagged
//   k_route_round    tiles x 256  a block per tile of 32 x 8 x 4 cells, gone at once when its flag in `now` is down.  Else the
//                                 tile and a halo of one cell (34 x 10 x 6 words, 8160 bytes) are staged in LDS, the two
//                                 sentinels (and what is outside the box) as kInf; a thread owns the four cells of a column
//                                 along z and keeps which of them are traversable in a register mask -- the field's own
//                                 kRouteBlocked says so, written from d2 by the seed.  It relaxes them in place, min(neighbour + w)
//                                 over the 26 neighbours, until a block-wide vote says nothing fell or kRouteIters passes are
//                                 done; then the tile flags itself for the next round.  Only cells that fell are written back;
//                                 each neighbouring tile that holds a cell next to one that fell is flagged in `next` (an atomic
//                                 OR: a flag found down is a fresh mark) and the fresh marks are added to the round's counter,
//                                 one atomic a block
//   k_route_count    grid x 256   traversable cells, reached cells, the sum and the largest cost: k_clear_count's per-block form
//   k_route_points   grid x 256   a thread per point: the cell's value
//   k_route_paths    grid x 256   a thread per start: the descent, at most max_cells steps
// Why any schedule gives the same bytes: a cell's value only ever falls, and only to some neighbour's value + w, which is the
// weight of a real chain of moves: it never goes below the least weight.  A halo value read while its owner lowers it may be
// old; it is then an upper bound, and the owner's mark runs the reader again in the next round, after the kernel boundary has
// made the new value visible.  The host stops when a round marked nothing: no cell can be lowered, which is the fixpoint, and
// the fixpoint of min-plus relaxation is unique (Dijkstra's distances).  No block waits on another: no spin, no grid barrier.
// All integer: no floating-point atomics, no run-time indexed private arrays, no scratch.
// Compiled with -ffp-contract=off (tl_voxel.hpp asks for it: the points go through vmap_quantise).
#include <algorithm>

#include "tl_route_box.hpp"
#include "tl_voxel.hpp"

namespace tl {
namespace {

constexpr int TX = tlr::kTileX, TY = tlr::kTileY, TZ = tlr::kTileZ;
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2, kHalo = HX * HY * HZ;
static_assert(TX * TY == 256 && TZ == 4, "a thread per column of four cells");
constexpr unsigned kInf = 0xFFFFFFFAu;   // both sentinels inside LDS: kInf + 5 does not wrap, and every cost + 5 is below it
constexpr int kRouteIters = 64;          // passes over a tile in LDS before it hands itself to the next round

// the index of cell (cx, cy, cz) in the field, -1 outside the box
__device__ __forceinline__ long long route_index(const RouteField& f, int cx, int cy, int cz) {
  const unsigned x = (unsigned)(cx - f.lo[0]), y = (unsigned)(cy - f.lo[1]), z = (unsigned)(cz - f.lo[2]);
  if (!(x < (unsigned)f.n[0] && y < (unsigned)f.n[1] && z < (unsigned)f.n[2])) return -1;
  return ((long long)z * f.n[1] + (long long)y) * f.n[0] + (long long)x;
}
__device__ __forceinline__ long long route_tile(const RouteField& f, long long idx) {
  const long long row = idx / f.n[0];
  const int x = (int)(idx - row * f.n[0]);
  const int z = (int)(row / f.n[1]), y = (int)(row - (long long)z * f.n[1]);
  return ((long long)(z / TZ) * f.tiles[1] + y / TY) * f.tiles[0] + x / TX;
}

// a query's point -> its cell; false: an INVALID point
__device__ __forceinline__ bool route_cell(const ScanAt& scan, int posed, const double origin[3], double voxel, long long g,
                                           int* cx, int* cy, int* cz) {
  double E[3] = {scan.pts[3 * g], scan.pts[3 * g + 1], scan.pts[3 * g + 2]};
  if (posed) map_transform_point(scan.M, E[0], E[1], E[2], &E[0], &E[1], &E[2]);
  unsigned long long key;
  unsigned qq[3];
  if (vmap_quantise(E, origin, voxel, &key, qq) != kVmapInside) return false;
  *cx = (int)key_axis(key, 0);
  *cy = (int)key_axis(key, 1);
  *cz = (int)key_axis(key, 2);
  return true;
}

__global__ __launch_bounds__(256) void k_route_seed(RouteSeedArgs A) {
  const long long groups = A.f.cells >> 2, stride = (long long)gridDim.x * 256;
  const unsigned need = (unsigned)A.need;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const uint2 v = reinterpret_cast<const uint2*>(A.d2)[t];
    reinterpret_cast<uint4*>(A.f.cost)[t] =
        make_uint4((v.x & 0xFFFFu) >= need ? kRouteUnreached : kRouteBlocked, (v.x >> 16) >= need ? kRouteUnreached : kRouteBlocked,
                   (v.y & 0xFFFFu) >= need ? kRouteUnreached : kRouteBlocked, (v.y >> 16) >= need ? kRouteUnreached : kRouteBlocked);
  }
}

__global__ __launch_bounds__(256) void k_route_goals(RouteSeedArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < A.goals.n;
  bool accepted = false, fresh = false;
  if (live) {
    int cx, cy, cz;
    if (route_cell(A.goals, A.posed, A.origin, A.voxel, g, &cx, &cy, &cz)) {
      const long long idx = route_index(A.f, cx, cy, A.flat ? A.f.lo[2] : cz);
      if (idx >= 0 && (unsigned)A.d2[idx] >= (unsigned)A.need) {
        accepted = true;
        A.f.cost[idx] = 0u;   // (after k_route_seed; two goals of one cell write the same word)
        fresh = atomicOr(&A.next[route_tile(A.f, idx)], 1u) == 0u;
      }
    }
  }
  wave_add(&A.ctl[0], accepted ? 1ull : 0ull);
  wave_add(&A.ctl[1], live && !accepted ? 1ull : 0ull);
  wave_add(&A.ctl[2], fresh ? 1ull : 0ull);
}

// min(cur, neighbour + w) over the 26 neighbours of the cell at s[at]: w = 3, 4, 5 for a face, an edge, a vertex step
__device__ __forceinline__ unsigned relax_cell(const unsigned* s, int at, unsigned cur) {
  unsigned best = cur;
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dz == 0 && dy == 0 && dx == 0) continue;
        const unsigned w = 2u + (unsigned)((dz != 0) + (dy != 0) + (dx != 0));
        best = min(best, s[at + (dz * HY + dy) * HX + dx] + w);
      }
  return best;
}

// the neighbouring tiles, as bits dz * 9 + dy * 3 + dx of (-1, 0, 1) + 1 each, that hold a cell next to cell (x, y, z) of a tile
__device__ __forceinline__ unsigned tiles_next_to(int x, int y, int z) {
  const unsigned ax = (x == 0 ? 1u : 0u) | 2u | (x == TX - 1 ? 4u : 0u);
  const unsigned ay = (y == 0 ? 1u : 0u) | 2u | (y == TY - 1 ? 4u : 0u);
  const unsigned az = (z == 0 ? 1u : 0u) | 2u | (z == TZ - 1 ? 4u : 0u);
  const unsigned m9 = (ay & 1u ? ax : 0u) | (ax << 3) | (ay & 4u ? ax << 6 : 0u);
  return (az & 1u ? m9 : 0u) | (m9 << 9) | (az & 4u ? m9 << 18 : 0u);
}

__global__ __launch_bounds__(256) void k_route_round(RouteField f, unsigned* __restrict__ now, unsigned* __restrict__ next,
                                                     unsigned long long* __restrict__ marks) {
  __shared__ unsigned s[kHalo];
  __shared__ unsigned s_mask;
  const long long tile = blockIdx.x;
  if (now[tile] == 0u) return;   // (the block's own flag: nobody writes it in this launch before the barrier below)
  const int tx = (int)(tile % f.tiles[0]);
  const long long rest = tile / f.tiles[0];
  const int ty = (int)(rest % f.tiles[1]), tz = (int)(rest / f.tiles[1]);
  const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
  for (int i = threadIdx.x; i < kHalo; i += 256) {
    const int lx = i % HX, r = i / HX, ly = r % HY, lz = r / HY;
    const int gx = x0 + lx - 1, gy = y0 + ly - 1, gz = z0 + lz - 1;
    unsigned v = kInf;
    if ((unsigned)gx < (unsigned)f.n[0] && (unsigned)gy < (unsigned)f.n[1] && (unsigned)gz < (unsigned)f.n[2]) {
      v = f.cost[((long long)gz * f.n[1] + gy) * f.n[0] + gx];
      if (v >= kRouteOutside) v = kInf;
    }
    s[i] = v;
  }
  if (threadIdx.x == 0) s_mask = 0u;
  // this thread's column: the cells (x, y, 0 .. 3) of the tile; which of them are traversable
  const int x = threadIdx.x & (TX - 1), y = threadIdx.x >> 5;
  const int gx = x0 + x, gy = y0 + y;
  const bool in_xy = gx < f.n[0] && gy < f.n[1];
  const long long plane = (long long)f.n[0] * f.n[1];
  const long long g0 = ((long long)z0 * f.n[1] + gy) * f.n[0] + gx;
  unsigned trav = 0u;
  if (in_xy) {
    if (z0 + 0 < f.n[2] && f.cost[g0] != kRouteBlocked) trav |= 1u;
    if (z0 + 1 < f.n[2] && f.cost[g0 + plane] != kRouteBlocked) trav |= 2u;
    if (z0 + 2 < f.n[2] && f.cost[g0 + 2 * plane] != kRouteBlocked) trav |= 4u;
    if (z0 + 3 < f.n[2] && f.cost[g0 + 3 * plane] != kRouteBlocked) trav |= 8u;
  }
  __syncthreads();
  if (threadIdx.x == 0) now[tile] = 0u;   // taken down: the array is all zero when it becomes `next`
  constexpr int kLayer = HY * HX;
  const int at = (HY + y + 1) * HX + x + 1;   // the column's cell z = 0 in the halo
  const unsigned o0 = s[at], o1 = s[at + kLayer], o2 = s[at + 2 * kLayer], o3 = s[at + 3 * kLayer];
  unsigned c0 = o0, c1 = o1, c2 = o2, c3 = o3;
  int again = 0;
  for (int it = 0; it < kRouteIters; ++it) {
    int fell = 0;
    // in place: a neighbour read while its owner writes it is the old or the new value, both upper bounds
    if (trav & 1u) { const unsigned b = relax_cell(s, at, c0); if (b < c0) { c0 = b; s[at] = b; fell = 1; } }
    if (trav & 2u) { const unsigned b = relax_cell(s, at + kLayer, c1); if (b < c1) { c1 = b; s[at + kLayer] = b; fell = 1; } }
    if (trav & 4u) { const unsigned b = relax_cell(s, at + 2 * kLayer, c2); if (b < c2) { c2 = b; s[at + 2 * kLayer] = b; fell = 1; } }
    if (trav & 8u) { const unsigned b = relax_cell(s, at + 3 * kLayer, c3); if (b < c3) { c3 = b; s[at + 3 * kLayer] = b; fell = 1; } }
    again = __syncthreads_or(fell);
    if (!again) break;
  }
  unsigned m = 0u;
  if (c0 < o0) { f.cost[g0] = c0; m |= tiles_next_to(x, y, 0); }
  if (c1 < o1) { f.cost[g0 + plane] = c1; m |= tiles_next_to(x, y, 1); }
  if (c2 < o2) { f.cost[g0 + 2 * plane] = c2; m |= tiles_next_to(x, y, 2); }
  if (c3 < o3) { f.cost[g0 + 3 * plane] = c3; m |= tiles_next_to(x, y, 3); }
  m &= ~(1u << 13);                                   // (the tile itself: only the cap below flags it)
  if (again && threadIdx.x == 0) m |= 1u << 13;       // the cap was met with cells still falling
  if (m) atomicOr(&s_mask, m);
  __syncthreads();
  if (threadIdx.x < 64) {                             // the first wave: a lane per direction
    bool fresh = false;
    const int d = threadIdx.x;
    if (d < 27 && (s_mask >> d & 1u)) {
      const int nx = tx + d % 3 - 1, ny = ty + d / 3 % 3 - 1, nz = tz + d / 9 - 1;
      if ((unsigned)nx < (unsigned)f.tiles[0] && (unsigned)ny < (unsigned)f.tiles[1] && (unsigned)nz < (unsigned)f.tiles[2])
        fresh = atomicOr(&next[((long long)nz * f.tiles[1] + ny) * f.tiles[0] + nx], 1u) == 0u;
    }
    const unsigned long long bal = __ballot(fresh);
    if (threadIdx.x == 0 && bal) atomicAdd(marks, (unsigned long long)__popcll(bal));
  }
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, off, 64));
  return v;
}

__global__ __launch_bounds__(256) void k_route_count(const unsigned* __restrict__ cost, long long cells, unsigned long long* ctl) {
  const long long groups = cells >> 2, stride = (long long)gridDim.x * 256;
  unsigned long long traversable = 0ull, reached = 0ull, sum = 0ull, most = 0ull;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(cost)[t];
    traversable += (v.x != kRouteBlocked) + (v.y != kRouteBlocked) + (v.z != kRouteBlocked) + (v.w != kRouteBlocked);
    const bool r0 = v.x < kRouteOutside, r1 = v.y < kRouteOutside, r2 = v.z < kRouteOutside, r3 = v.w < kRouteOutside;
    const unsigned f0 = r0 ? v.x : 0u, f1 = r1 ? v.y : 0u, f2 = r2 ? v.z : 0u, f3 = r3 ? v.w : 0u;
    reached += r0 + r1 + r2 + r3;
    sum += (unsigned long long)f0 + f1 + f2 + f3;
    most = max(most, (unsigned long long)max(max(f0, f1), max(f2, f3)));
  }
  // the block's four waves through LDS, then one atomic per counter and block (k_clear_count: DESIGN.md section 30 measured why)
  __shared__ unsigned long long s_part[4][4];
  traversable = wave_sum(traversable);
  reached = wave_sum(reached);
  sum = wave_sum(sum);
  most = wave_max(most);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_part[wave][0] = traversable;
    s_part[wave][1] = reached;
    s_part[wave][2] = sum;
    s_part[wave][3] = most;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const unsigned long long v = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
    if (v) atomicAdd(&ctl[threadIdx.x], v);
  } else if (threadIdx.x == 3) {
    const unsigned long long v = max(max(s_part[0][3], s_part[1][3]), max(s_part[2][3], s_part[3][3]));
    if (v) atomicMax(&ctl[3], v);
  }
}

__global__ __launch_bounds__(256) void k_route_points(RoutePointsArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < A.scan.n;
  int kind = 3;
  if (live) {
    unsigned v = kRouteOutside;
    int cx, cy, cz;
    if (route_cell(A.scan, A.posed, A.origin, A.voxel, g, &cx, &cy, &cz)) {
      const long long idx = route_index(A.f, cx, cy, cz);
      if (idx >= 0) v = A.f.cost[idx];
    }
    kind = v < kRouteOutside ? 0 : v == kRouteUnreached ? 1 : v == kRouteBlocked ? 2 : 3;
    A.cost[g] = v;
    if (A.distance) A.distance[g] = kind == 0 ? A.voxel * (double)v / 3.0 : kind == 1 ? __builtin_huge_val() : __builtin_nan("");
  }
  wave_count_states(live, kind, A.ctl);
}

__global__ __launch_bounds__(256) void k_route_paths(RoutePathsArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= A.scan.n) return;
  const RouteField& f = A.f;
  int status = TLOAM_ROUTE_PATH_OUTSIDE, written = 0;
  unsigned v = kRouteOutside;
  int cx, cy, cz;
  long long idx = -1;
  if (route_cell(A.scan, A.posed, A.origin, A.voxel, g, &cx, &cy, &cz)) idx = route_index(f, cx, cy, cz);
  if (idx >= 0) {
    v = f.cost[idx];
    if (v == kRouteBlocked) {
      status = TLOAM_ROUTE_PATH_BLOCKED;
    } else if (v == kRouteUnreached) {
      status = TLOAM_ROUTE_PATH_UNREACHED;
    } else if (v < kRouteOutside) {
      status = TLOAM_ROUTE_PATH_TRUNCATED;
      int x = cx - f.lo[0], y = cy - f.lo[1], z = cz - f.lo[2];
      unsigned k = v;
      double* out = A.centres + 3 * g * A.max_cells;
      for (long long j = 0; j < A.max_cells; ++j) {   // (at most max_cells steps, whatever the field holds)
        out[3 * j] = A.origin[0] + ((double)(f.lo[0] + x) + 0.5) * A.voxel;
        out[3 * j + 1] = A.origin[1] + ((double)(f.lo[1] + y) + 0.5) * A.voxel;
        out[3 * j + 2] = A.origin[2] + ((double)(f.lo[2] + z) + 0.5) * A.voxel;
        written = (int)(j + 1);
        if (k == 0u) {
          status = TLOAM_ROUTE_PATH_REACHED;
          break;
        }
        // the first neighbour, dz outermost, then dy, then dx, with c + w == k
        bool found = false;
        int sx = 0, sy = 0, sz = 0;
        unsigned sc = 0u;
        for (int dz = -1; dz <= 1 && !found; ++dz)
          for (int dy = -1; dy <= 1 && !found; ++dy)
            for (int dx = -1; dx <= 1 && !found; ++dx) {
              if (dz == 0 && dy == 0 && dx == 0) continue;
              const int ux = x + dx, uy = y + dy, uz = z + dz;
              if (!((unsigned)ux < (unsigned)f.n[0] && (unsigned)uy < (unsigned)f.n[1] && (unsigned)uz < (unsigned)f.n[2])) continue;
              const unsigned c = f.cost[((long long)uz * f.n[1] + uy) * f.n[0] + ux];
              const unsigned w = 2u + (unsigned)((dz != 0) + (dy != 0) + (dx != 0));
              if (c < kRouteOutside && c + w == k) {
                found = true;
                sx = ux; sy = uy; sz = uz; sc = c;
              }
            }
        if (!found) break;   // (a damaged field: TRUNCATED)
        x = sx; y = sy; z = sz; k = sc;
      }
    }
  }
  A.status[g] = (unsigned char)status;
  A.n_cells[g] = written;
  A.cost[g] = v;
}

}  // namespace

void launch_route_seed(const RouteSeedArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_route_seed, dim3(std::min(blocks_of((size_t)(A.f.cells >> 2)), 4096u)), dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_route_goals, dim3(blocks_of((size_t)std::max<long long>(A.goals.n, 1))), dim3(256), 0, s, A);
}

void launch_route_round(const RouteField& f, unsigned* now, unsigned* next, unsigned long long* marks, hipStream_t s) {
  const long long tiles = (long long)f.tiles[0] * f.tiles[1] * f.tiles[2];   // (< 2^30: tl_route_box.hpp)
  hipLaunchKernelGGL(k_route_round, dim3((unsigned)tiles), dim3(256), 0, s, f, now, next, marks);
}

void launch_route_count(const RouteField& f, unsigned long long* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_route_count, dim3(std::min(blocks_of((size_t)(f.cells >> 2)), 512u)), dim3(256), 0, s, f.cost, f.cells, ctl);
}

void launch_route_points(const RoutePointsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_route_points, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

void launch_route_paths(const RoutePathsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_route_paths, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

}  // namespace tl
