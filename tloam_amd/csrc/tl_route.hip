// tl_route.hip -- the device side of the route through the closed map (tl_api_route.hip): a dense field of
// uint32 over the clearance field's box, [z][y][x], x fastest: the least total 3-4-5 chamfer weight of a chain of 26-connected
// moves over traversable cells to an accepted goal; kRouteUnreached where no goal reaches, kRouteBlocked where the cell is not
// traversable (its d2 < max(need, 1)).  The column form is the same kernels over a layer, n[2] = 1: what lies above and below is
// outside the box, so 8 moves of weight 3 and 4 remain.
//
// Launches (nothing of the closed map, the free-space grid or the clearance field is written):
//   k_route_seed     grid x 256   a thread per four cells along x: d2 read, kRouteUnreached or kRouteBlocked written
//   k_route_goals    grid x 256   a thread per goal: the point's cell, 0 written when it is traversable, its tile flagged
//   k_route_round    tiles x 256  one round of the tile engine (tl_tile.hpp's tile_round, which states the round and why any
//                                 schedule gives the same bytes) under RouteRound: the two sentinels (and what is outside the
//                                 box) are 0xFFFFFFFA in LDS, a move adds 3, 4 or 5, and a cell may fall when it is
//                                 traversable -- the field's own kRouteBlocked says so, written from d2 by the seed
//   k_route_count    grid x 256   traversable cells, reached cells, the sum and the largest cost: k_clear_count's per-block form
//   k_route_points   grid x 256   a thread per point: the cell's value
//   k_route_paths    grid x 256   a thread per start: the descent, at most max_cells steps
// The operator is monotone and bounded below: a cell only ever falls to some neighbour's value + w, the weight of a real chain
// of moves to a goal, so it never goes below the least such weight; the fixpoint of min-plus relaxation from the goals' zeros is
// unique (Dijkstra's distances).
// Compiled with -ffp-contract=off (tl_voxel.hpp asks for it: the points go through vmap_quantise).
#include <algorithm>

#include "tl_tile.hpp"
#include "tl_voxel.hpp"

namespace tl {
namespace {

struct RouteRound {
  static constexpr unsigned kNothing = 0xFFFFFFFAu;   // kNothing + 5 does not wrap, and every cost + 5 is below it
  static constexpr unsigned kSentinel = kRouteOutside;
  static constexpr int kPasses = 64;
  static constexpr bool kLiveFromField = true;
  static constexpr unsigned kDead = kRouteBlocked;
  static constexpr unsigned weight(int steps) { return 2u + (unsigned)steps; }   // 3, 4, 5 for a face, an edge, a vertex step
};

__global__ __launch_bounds__(256) void k_route_seed(RouteSeedArgs A) {
  const long long groups = A.f.cells >> 2, stride = (long long)gridDim.x * 256;
  const unsigned need = (unsigned)A.need;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const uint2 v = reinterpret_cast<const uint2*>(A.d2)[t];
    reinterpret_cast<uint4*>(A.f.v)[t] =
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
      if (A.flat) cz = A.f.lo[2];
      const long long idx = tile_index(A.f, cx, cy, cz);
      if (idx >= 0 && (unsigned)A.d2[idx] >= (unsigned)A.need) {
        accepted = true;
        A.f.v[idx] = 0u;   // (after k_route_seed; two goals of one cell write the same word)
        fresh = atomicOr(&A.next[tile_of(A.f, cx - A.f.lo[0], cy - A.f.lo[1], cz - A.f.lo[2])], 1u) == 0u;
      }
    }
  }
  wave_add(&A.ctl[0], accepted ? 1ull : 0ull);
  wave_add(&A.ctl[1], live && !accepted ? 1ull : 0ull);
  wave_add(&A.ctl[2], fresh ? 1ull : 0ull);
}

__global__ __launch_bounds__(256) void k_route_round(TileField f, unsigned* __restrict__ now, unsigned* __restrict__ next,
                                                     unsigned long long* __restrict__ marks) {
  tile_round<RouteRound>(f, now, next, marks);
}

__global__ __launch_bounds__(256) void k_route_count(const unsigned* __restrict__ cost, long long cells, unsigned long long* ctl) {
  const long long groups = cells >> 2, stride = (long long)gridDim.x * 256;
  unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};   // traversable cells, reached cells, their sum; the largest
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(cost)[t];
    c[0] += (v.x != kRouteBlocked) + (v.y != kRouteBlocked) + (v.z != kRouteBlocked) + (v.w != kRouteBlocked);
    const bool r0 = v.x < kRouteOutside, r1 = v.y < kRouteOutside, r2 = v.z < kRouteOutside, r3 = v.w < kRouteOutside;
    const unsigned f0 = r0 ? v.x : 0u, f1 = r1 ? v.y : 0u, f2 = r2 ? v.z : 0u, f3 = r3 ? v.w : 0u;
    c[1] += r0 + r1 + r2 + r3;
    c[2] += (unsigned long long)f0 + f1 + f2 + f3;
    c[3] = max(c[3], (unsigned long long)max(max(f0, f1), max(f2, f3)));
  }
  block_fold<3, 1>(c, ctl);
}

__global__ __launch_bounds__(256) void k_route_points(RoutePointsArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < A.scan.n;
  int kind = 3;
  if (live) {
    unsigned v = kRouteOutside;
    int cx, cy, cz;
    if (route_cell(A.scan, A.posed, A.origin, A.voxel, g, &cx, &cy, &cz)) {
      const long long idx = tile_index(A.f, cx, cy, cz);
      if (idx >= 0) v = A.f.v[idx];
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
  const TileField& f = A.f;
  int status = TLOAM_ROUTE_PATH_OUTSIDE, written = 0;
  unsigned v = kRouteOutside;
  int cx, cy, cz;
  long long idx = -1;
  if (route_cell(A.scan, A.posed, A.origin, A.voxel, g, &cx, &cy, &cz)) idx = tile_index(f, cx, cy, cz);
  if (idx >= 0) {
    v = f.v[idx];
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
              const unsigned c = f.v[((long long)uz * f.n[1] + uy) * f.n[0] + ux];
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

void launch_route_round(const TileField& f, unsigned* now, unsigned* next, unsigned long long* marks, hipStream_t s) {
  const long long tiles = (long long)f.tiles[0] * f.tiles[1] * f.tiles[2];   // (< 2^30: tl_tile_box.hpp)
  hipLaunchKernelGGL(k_route_round, dim3((unsigned)tiles), dim3(256), 0, s, f, now, next, marks);
}

void launch_route_count(const TileField& f, unsigned long long* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_route_count, dim3(std::min(blocks_of((size_t)(f.cells >> 2)), 512u)), dim3(256), 0, s, f.v, f.cells, ctl);
}

void launch_route_points(const RoutePointsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_route_points, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

void launch_route_paths(const RoutePathsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_route_paths, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

}  // namespace tl
