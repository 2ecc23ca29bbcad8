// tl_frontier.hip -- the device side of the closed map's frontiers (tl_api_frontier.hip): a dense field of
// uint32 over the free-space grid's box, [z][y][x], x fastest.  A frontier cell -- a FREE cell with an UNKNOWN face neighbour
// inside the box -- holds the least linear index of its 26-connected component of frontier cells; every other cell holds its
// state's sentinel (kFrontFree, kFrontUnknown, kFrontOccupied).  The column form is the same kernels over a layer, n[2] = 1: what
// lies above and below is outside the box, so 4 face neighbours and 8-connectivity remain.
//
// Launches (nothing of the closed map, the free-space grid, the clearance or the route field is written):
//   k_front_seed      grid x 256   a thread per four cells along x: the brick's word read, kFrontFree or kFrontUnknown written
//   k_front_voxels    grid x 256   a thread per voxel row of the map: one that counts (CarveGate) and lies in the box writes
//                                  kFrontOccupied (k_clear_seed / k_clear_voxels: no table probe a cell)
//   k_front_col_seed  grid x 256   the column form's states: a thread per four columns of k_free_columns' layer
//   k_front_mark      grid x 256   a thread per cell: a kFrontFree cell with a kFrontUnknown face neighbour becomes its own index
//                                  and flags its tile.  A neighbour already rewritten to an index was FREE; only equality with
//                                  kFrontUnknown is tested and an UNKNOWN cell never changes: race-free in meaning
//   k_front_round     tiles x 256  one round of the tile engine (tl_tile.hpp's tile_round, which states the round and why any
//                                  schedule gives the same bytes) under FrontRound: everything that is no frontier cell (and
//                                  what is outside the box) is kInf in LDS, a move adds nothing, and a cell may fall when it
//                                  is a frontier cell: its word in LDS is not kInf
//   k_front_count     grid x 256   cells per state, frontier cells, roots (label == own index): k_clear_count's per-block form
//   k_front_roots     grid x 256   the roots compacted in ascending order (block_packed_scan, lookback_prefix, as k_free_cells),
//                                  each with an empty record
//   k_front_accum     grid x 256   a thread per cell: the records accumulated with integer atomics; a wave's runs of equal labels
//                                  along a row are summed by shuffle scans first (k_surfel_accum), the slot found by a bounded
//                                  binary search of the ascending root list
//   k_front_keep      grid x 256   the records with cells >= min_cells compacted in order, a component's kept index written
//   k_front_cells     grid x 256   the centres of the kept clusters' cells (or of one cluster's), ascending in linear index
//   k_front_points    grid x 256   a thread per point: the cell's value and its kept cluster
//   k_front_costs     grid x 256   a thread per cell: a kept cluster's cell scans the route field within `reach` cells and lowers
//                                  its cluster's key, (cost << 32) | linear, by one 64-bit unsigned atomicMin
// The operator is monotone and bounded below: a label only ever falls, and only to the label of a neighbouring frontier cell,
// which is the index of a cell of the same component, so it never goes below the component's least index; at the fixpoint every
// cell holds the minimum over its component, and that is unique.  No block waits on another in the rounds: no spin, no CAS loop,
// no grid barrier; the only wait is the bounded look-back of the three compactions (tl_voxel.hpp).  All integer but the centres;
// no run-time indexed private arrays, no scratch.
// Compiled with -ffp-contract=off (tl_voxel.hpp asks for it: the points go through vmap_quantise).
#include <algorithm>

#include "tl_tile.hpp"
#include "tl_voxel.hpp"

namespace tl {
namespace {

constexpr unsigned kInf = 0xFFFFFFFFu;   // everything that is no frontier cell inside LDS: min never takes it
struct FrontRound {
  static constexpr unsigned kNothing = kInf;
  static constexpr unsigned kSentinel = kFrontOutside;
  static constexpr int kPasses = 64;
  static constexpr bool kLiveFromField = false;
  static constexpr unsigned weight(int) { return 0u; }
};

// the face neighbours of cell idx = (x, y, z), inside the box, that are UNKNOWN
__device__ __forceinline__ unsigned front_faces(const TileField& f, long long idx, int x, int y, int z) {
  const long long nx = f.n[0], plane = nx * f.n[1];
  unsigned faces = 0u;
  if (x > 0 && f.v[idx - 1] == kFrontUnknown) ++faces;
  if (x + 1 < f.n[0] && f.v[idx + 1] == kFrontUnknown) ++faces;
  if (y > 0 && f.v[idx - nx] == kFrontUnknown) ++faces;
  if (y + 1 < f.n[1] && f.v[idx + nx] == kFrontUnknown) ++faces;
  if (z > 0 && f.v[idx - plane] == kFrontUnknown) ++faces;
  if (z + 1 < f.n[2] && f.v[idx + plane] == kFrontUnknown) ++faces;
  return faces;
}
// the slot of root `v` in the ascending list, -1 when it is none: at most 33 halvings
__device__ __forceinline__ long long front_slot(const unsigned* roots, long long nroots, unsigned v) {
  long long lo = 0, hi = nroots;
  for (int it = 0; it < 33 && lo < hi; ++it) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (roots[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < nroots && roots[lo] == v ? lo : -1;
}

__global__ __launch_bounds__(256) void k_front_seed(FrontSeedArgs A) {
  const FreeGrid& g = A.q.g;
  const long long groups = A.f.cells >> 2, stride = (long long)gridDim.x * 256;
  const long long ny = A.f.n[1];
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const long long row = t / g.nb[0];
    const int bx = (int)(t - row * g.nb[0]);
    const long long z = row / ny;
    const int y = (int)(row - z * ny);
    const unsigned long long w = g.words[((z >> 2) * g.nb[1] + (y >> 2)) * g.nb[0] + bx];
    const unsigned bits = (unsigned)(w >> ((((int)z & 3) << 4) | ((y & 3) << 2))) & 0xFu;
    reinterpret_cast<uint4*>(A.f.v)[t] = make_uint4(bits & 1u ? kFrontFree : kFrontUnknown, bits & 2u ? kFrontFree : kFrontUnknown,
                                                    bits & 4u ? kFrontFree : kFrontUnknown, bits & 8u ? kFrontFree : kFrontUnknown);
  }
}

__global__ __launch_bounds__(256) void k_front_voxels(FrontSeedArgs A) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= A.q.grid.nv) return;
  const VmapTableView& map = A.q.grid.map;
  if (!A.q.gate.counts(map, (int)id)) return;
  const unsigned long long key = map.pkey[id];
  const long long idx = tile_index(A.f, (int)key_axis(key, 0), (int)key_axis(key, 1), (int)key_axis(key, 2));
  if (idx >= 0) A.f.v[idx] = kFrontOccupied;
}

__device__ __forceinline__ unsigned state_label(unsigned s) {
  return s == (unsigned)TLOAM_OCCUPANCY_OCCUPIED ? kFrontOccupied : s == (unsigned)TLOAM_OCCUPANCY_FREE ? kFrontFree : kFrontUnknown;
}

__global__ __launch_bounds__(256) void k_front_col_seed(FrontSeedArgs A) {
  const long long groups = A.f.cells >> 2, stride = (long long)gridDim.x * 256;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const unsigned v = reinterpret_cast<const unsigned*>(A.state)[t];
    reinterpret_cast<uint4*>(A.f.v)[t] =
        make_uint4(state_label(v & 0xFFu), state_label((v >> 8) & 0xFFu), state_label((v >> 16) & 0xFFu), state_label(v >> 24));
  }
}

__global__ __launch_bounds__(256) void k_front_mark(FrontSeedArgs A) {
  const TileField& f = A.f;
  const long long stride = (long long)gridDim.x * 256;
  unsigned long long v[2] = {0ull, 0ull};   // fresh tile marks, unknown faces
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < f.cells; idx += stride) {
    if (f.v[idx] != kFrontFree) continue;   // (this cell's word: only this thread writes it)
    int x, y, z;
    tile_xyz(f, idx, &x, &y, &z);
    const unsigned faces = front_faces(f, idx, x, y, z);
    if (faces == 0u) continue;
    f.v[idx] = (unsigned)idx;
    v[1] += faces;
    unsigned* flag = &A.next[tile_of(f, x, y, z)];
    // (a flag read as down may be up by now: the atomic decides who counts the mark)
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && atomicOr(flag, 1u) == 0u) v[0] += 1ull;
  }
  block_fold<2, 0>(v, A.ctl);
}

__global__ __launch_bounds__(256) void k_front_round(TileField f, unsigned* __restrict__ now, unsigned* __restrict__ next,
                                                     unsigned long long* __restrict__ marks) {
  tile_round<FrontRound>(f, now, next, marks);
}

__device__ __forceinline__ void count_cell(unsigned v, unsigned own, unsigned long long (&c)[5]) {
  c[0] += v == kFrontFree || v < kFrontOutside;
  c[1] += v == kFrontUnknown;
  c[2] += v == kFrontOccupied;
  c[3] += v < kFrontOutside;
  c[4] += v == own;
}

__global__ __launch_bounds__(256) void k_front_count(const unsigned* __restrict__ label, long long cells, unsigned long long* ctl) {
  const long long groups = cells >> 2, stride = (long long)gridDim.x * 256;
  unsigned long long c[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < groups; t += stride) {
    const uint4 v = reinterpret_cast<const uint4*>(label)[t];
    const unsigned own = (unsigned)(4 * t);
    count_cell(v.x, own, c);
    count_cell(v.y, own + 1u, c);
    count_cell(v.z, own + 2u, c);
    count_cell(v.w, own + 3u, c);
  }
  block_fold<5, 0>(c, ctl + 2);
}

__global__ __launch_bounds__(256) void k_front_roots(FrontGatherArgs A, int nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const int bid = block_ticket(&A.ctl[8], &s_bid);
  const long long t = (long long)bid * 256 + threadIdx.x;
  const unsigned own = (unsigned)(4 * t);
  unsigned pass = 0u;
  if (t < (A.f.cells >> 2)) {
    const uint4 v = reinterpret_cast<const uint4*>(A.f.v)[t];
    pass = (v.x == own ? 1u : 0u) | (v.y == own + 1u ? 2u : 0u) | (v.z == own + 2u ? 4u : 0u) | (v.w == own + 3u ? 8u : 0u);
  }
  unsigned long long before, total;
  block_packed_scan((unsigned long long)__popc(pass), s_wave, &before, &total);
  if (threadIdx.x == 0) s_prefix = lookback_prefix(A.look, bid, total, LookFaultDevice{&A.ctl[9]});
  __syncthreads();
  long long p = (long long)(s_prefix + before);
  while (pass) {   // (at most four rounds: a bit goes each)
    const int b = __builtin_ctz(pass);
    pass &= pass - 1u;
    if (p < A.nroots) {   // (the count said so; a timed-out look-back must not write past the table)
      A.roots[p] = own + (unsigned)b;
      tloam_closed_map_frontier_cluster r;
      r.sum[0] = 0; r.sum[1] = 0; r.sum[2] = 0;
      r.lo[0] = INT32_MAX; r.lo[1] = INT32_MAX; r.lo[2] = INT32_MAX;
      r.hi[0] = INT32_MIN; r.hi[1] = INT32_MIN; r.hi[2] = INT32_MIN;
      r.root = own + (unsigned)b;
      r.cells = 0u;
      r.unknown_faces = 0u;
      r.reserved = 0u;
      A.rec[p] = r;
    }
    ++p;
  }
  if (bid == nblocks - 1 && threadIdx.x == 0) A.ctl[10] = s_prefix + total;
}

__global__ __launch_bounds__(256) void k_front_accum(FrontGatherArgs A) {
  const TileField& f = A.f;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  unsigned id = kInf;
  int x = 0, y = 0, z = 0;
  bool ok = false;
  if (g < f.cells) {
    id = f.v[g];
    ok = id < kFrontOutside;
  }
  const unsigned long long okb = __ballot(ok);
  if (okb == 0ull) return;   // (wave-uniform)
  unsigned cnt = ok ? 1u : 0u, sx = 0u, faces = 0u;
  if (ok) {
    tile_xyz(f, g, &x, &y, &z);
    sx = (unsigned)x;
    faces = front_faces(f, g, x, y, z);
  }
  // runs of equal labels among consecutive lanes of one row: y and z are the run's, x ascends by one a lane
  const unsigned idprev = __shfl_up(id, 1, 64), idnext = __shfl_down(id, 1, 64);
  const bool ok_prev = lane > 0 && ((okb >> (lane - 1)) & 1ull), ok_next = lane < 63 && ((okb >> (lane + 1)) & 1ull);
  const bool head = ok && !(ok_prev && idprev == id && x != 0);
  const bool tail = ok && !(ok_next && idnext == id && x != f.n[0] - 1);
  const unsigned long long heads = __ballot(head);
  if (heads != okb) {   // (wave-uniform) some run is longer than one cell; 64 * 2^21 fits 32 bits
    const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
    const int hl = (heads & upto) ? 63 - __clzll(heads & upto) : 0;
    cnt = run_sum(wave_scan(cnt, lane), hl);
    sx = run_sum(wave_scan(sx, lane), hl);
    faces = run_sum(wave_scan(faces, lane), hl);
  }
  if (!tail) return;
  const long long slot = front_slot(A.roots, A.nroots, id);
  if (slot < 0) return;   // (a damaged field)
  tloam_closed_map_frontier_cluster* r = A.rec + slot;
  atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum[0]), (unsigned long long)sx);
  atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum[1]), (unsigned long long)y * cnt);
  atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum[2]), (unsigned long long)z * cnt);
  atomicMin(&r->lo[0], f.lo[0] + x - (int)(cnt - 1u));
  atomicMin(&r->lo[1], f.lo[1] + y);
  atomicMin(&r->lo[2], f.lo[2] + z);
  atomicMax(&r->hi[0], f.lo[0] + x);
  atomicMax(&r->hi[1], f.lo[1] + y);
  atomicMax(&r->hi[2], f.lo[2] + z);
  atomicAdd(&r->cells, cnt);
  atomicAdd(&r->unknown_faces, faces);
}

__global__ __launch_bounds__(256) void k_front_keep(FrontGatherArgs A, unsigned long long* look, int nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const int bid = block_ticket(&A.ctl[12], &s_bid);
  const long long slot = (long long)bid * 256 + threadIdx.x;
  unsigned cells = 0u;
  if (slot < A.nroots) cells = A.rec[slot].cells;
  const bool keep = slot < A.nroots && cells >= A.min_cells;
  unsigned long long before, total;
  block_packed_scan(keep ? 1ull : 0ull, s_wave, &before, &total);
  if (threadIdx.x == 0) s_prefix = lookback_prefix(look, bid, total, LookFaultDevice{&A.ctl[13]});
  __syncthreads();
  const long long p = (long long)(s_prefix + before);
  if (slot < A.nroots) A.kept_of[slot] = keep && p < A.nroots ? (int)p : -1;
  if (keep && p < A.nroots) A.kept_rec[p] = A.rec[slot];
  if (bid == nblocks - 1 && threadIdx.x == 0) A.ctl[14] = s_prefix + total;
  // the cells kept: the block's sum, one atomic; the largest component: a wave's, then one atomicMax a wave that has one
  unsigned long long v[1] = {keep ? (unsigned long long)cells : 0ull};
  block_fold<1, 0>(v, &A.ctl[15]);
  unsigned most = cells;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) most = max(most, (unsigned)__shfl_xor(most, off, 64));
  if ((threadIdx.x & 63) == 0 && most) atomicMax(&A.ctl[16], (unsigned long long)most);
}

__global__ __launch_bounds__(256) void k_front_cells(FrontCellsArgs A, int nblocks) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const int bid = block_ticket(&A.ctl[20], &s_bid);
  const TileField& f = A.f;
  const long long t = (long long)bid * 256 + threadIdx.x;
  unsigned pass = 0u;
  uint4 v = make_uint4(kInf, kInf, kInf, kInf);
  if (t < (f.cells >> 2)) {
    v = reinterpret_cast<const uint4*>(f.v)[t];
    if (A.root != kFrontFree) {
      pass = (v.x == A.root ? 1u : 0u) | (v.y == A.root ? 2u : 0u) | (v.z == A.root ? 4u : 0u) | (v.w == A.root ? 8u : 0u);
    } else {
      if (v.x < kFrontOutside) { const long long s = front_slot(A.t.roots, A.t.nroots, v.x); if (s >= 0 && A.t.kept_of[s] >= 0) pass |= 1u; }
      if (v.y < kFrontOutside) { const long long s = front_slot(A.t.roots, A.t.nroots, v.y); if (s >= 0 && A.t.kept_of[s] >= 0) pass |= 2u; }
      if (v.z < kFrontOutside) { const long long s = front_slot(A.t.roots, A.t.nroots, v.z); if (s >= 0 && A.t.kept_of[s] >= 0) pass |= 4u; }
      if (v.w < kFrontOutside) { const long long s = front_slot(A.t.roots, A.t.nroots, v.w); if (s >= 0 && A.t.kept_of[s] >= 0) pass |= 8u; }
    }
  }
  unsigned long long before, total;
  block_packed_scan((unsigned long long)__popc(pass), s_wave, &before, &total);
  if (threadIdx.x == 0) s_prefix = lookback_prefix(A.look, bid, total, LookFaultDevice{&A.ctl[21]});
  __syncthreads();
  size_t p = (size_t)(s_prefix + before);
  if (p + (size_t)__popc(pass) > (size_t)A.m) pass = 0u;   // (a timed-out look-back must not write past the outputs)
  if (pass) {
    int x, y, z;
    tile_xyz(f, 4 * t, &x, &y, &z);   // (n[0] is a multiple of 4: the four cells share a row)
    const double py = A.origin[1] + ((double)(f.lo[1] + y) + 0.5) * A.voxel, pz = A.origin[2] + ((double)(f.lo[2] + z) + 0.5) * A.voxel;
    if (pass & 1u) { A.centres[3 * p] = A.origin[0] + ((double)(f.lo[0] + x) + 0.5) * A.voxel; A.centres[3 * p + 1] = py; A.centres[3 * p + 2] = pz; A.roots_out[p] = v.x; ++p; }
    if (pass & 2u) { A.centres[3 * p] = A.origin[0] + ((double)(f.lo[0] + x + 1) + 0.5) * A.voxel; A.centres[3 * p + 1] = py; A.centres[3 * p + 2] = pz; A.roots_out[p] = v.y; ++p; }
    if (pass & 4u) { A.centres[3 * p] = A.origin[0] + ((double)(f.lo[0] + x + 2) + 0.5) * A.voxel; A.centres[3 * p + 1] = py; A.centres[3 * p + 2] = pz; A.roots_out[p] = v.z; ++p; }
    if (pass & 8u) { A.centres[3 * p] = A.origin[0] + ((double)(f.lo[0] + x + 3) + 0.5) * A.voxel; A.centres[3 * p + 1] = py; A.centres[3 * p + 2] = pz; A.roots_out[p] = v.w; ++p; }
  }
  if (bid == nblocks - 1 && threadIdx.x == 0) A.ctl[22] = s_prefix + total;
}

__global__ __launch_bounds__(256) void k_front_points(FrontPointsArgs A) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < A.scan.n;
  int kind = 4;
  if (live) {
    unsigned v = kFrontOutside;
    int cluster = -1;
    int cx, cy, cz;
    if (route_cell(A.scan, A.posed, A.origin, A.voxel, g, &cx, &cy, &cz)) {
      const long long idx = tile_index(A.f, cx, cy, cz);
      if (idx >= 0) v = A.f.v[idx];
    }
    if (v < kFrontOutside) {
      const long long s = front_slot(A.t.roots, A.t.nroots, v);
      if (s >= 0) cluster = A.t.kept_of[s];
    }
    kind = v < kFrontOutside ? 0 : v == kFrontFree ? 1 : v == kFrontUnknown ? 2 : v == kFrontOccupied ? 3 : 4;
    A.label[g] = v;
    if (A.cluster) A.cluster[g] = cluster;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned long long bal = __ballot(live && kind == k);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.ctl[k], (unsigned long long)__popcll(bal));
  }
}

__global__ __launch_bounds__(256) void k_front_costs(FrontCostsArgs A) {
  const TileField& f = A.f;
  const long long stride = (long long)gridDim.x * 256;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < f.cells; g += stride) {
    const unsigned v = f.v[g];
    if (v >= kFrontOutside) continue;
    const long long s = front_slot(A.t.roots, A.t.nroots, v);
    if (s < 0) continue;
    const int k = A.t.kept_of[s];
    if (k < 0) continue;
    int x, y, z;
    tile_xyz(f, g, &x, &y, &z);
    const int xa = max(x - A.reach, 0), xb = min(x + A.reach, f.n[0] - 1);
    const int ya = max(y - A.reach, 0), yb = min(y + A.reach, f.n[1] - 1);
    const int za = max(z - A.reach, 0), zb = min(z + A.reach, f.n[2] - 1);
    unsigned long long best = ~0ull;
    for (int uz = za; uz <= zb; ++uz)      // (at most 9 x 9 x 9 cells)
      for (int uy = ya; uy <= yb; ++uy) {
        const long long row = ((long long)uz * f.n[1] + uy) * f.n[0];
        for (int ux = xa; ux <= xb; ++ux) {
          const unsigned c = A.cost[row + ux];
          if (c < kRouteOutside) best = min(best, ((unsigned long long)c << 32) | (unsigned long long)(row + ux));
        }
      }
    if (best != ~0ull) atomicMin(&A.keys[k], best);
  }
}

}  // namespace

int launch_front_seed(const FrontSeedArgs& A, hipStream_t s) {
  const unsigned gblocks = std::min(blocks_of((size_t)std::max<long long>(A.f.cells >> 2, 1)), 4096u);
  int launches = 2;
  if (A.state) {
    hipLaunchKernelGGL(k_front_col_seed, dim3(gblocks), dim3(256), 0, s, A);
  } else {
    hipLaunchKernelGGL(k_front_seed, dim3(gblocks), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_front_voxels, dim3(blocks_of((size_t)std::max<long long>(A.q.grid.nv, 1))), dim3(256), 0, s, A);
    launches = 3;
  }
  hipLaunchKernelGGL(k_front_mark, dim3(std::min(blocks_of((size_t)A.f.cells), 16384u)), dim3(256), 0, s, A);
  return launches;
}

void launch_front_round(const TileField& f, unsigned* now, unsigned* next, unsigned long long* marks, hipStream_t s) {
  const long long tiles = (long long)f.tiles[0] * f.tiles[1] * f.tiles[2];   // (< 2^27: tl_tile_box.hpp)
  hipLaunchKernelGGL(k_front_round, dim3((unsigned)tiles), dim3(256), 0, s, f, now, next, marks);
}

void launch_front_count(const TileField& f, unsigned long long* ctl, hipStream_t s) {
  hipLaunchKernelGGL(k_front_count, dim3(std::min(blocks_of((size_t)(f.cells >> 2)), 512u)), dim3(256), 0, s, f.v, f.cells, ctl);
}

int launch_front_gather(const FrontGatherArgs& A, hipStream_t s) {
  const int nb = (int)blocks_of((size_t)(A.f.cells >> 2));
  hipLaunchKernelGGL(k_front_roots, dim3(nb), dim3(256), 0, s, A, nb);
  hipLaunchKernelGGL(k_front_accum, dim3(blocks_of((size_t)A.f.cells)), dim3(256), 0, s, A);
  const int kb = (int)blocks_of((size_t)A.nroots);
  hipLaunchKernelGGL(k_front_keep, dim3(kb), dim3(256), 0, s, A, A.look + nb + 1, kb);
  return 3;
}

void launch_front_cells(const FrontCellsArgs& A, hipStream_t s) {
  const int nb = (int)blocks_of((size_t)(A.f.cells >> 2));
  hipLaunchKernelGGL(k_front_cells, dim3(nb), dim3(256), 0, s, A, nb);
}

void launch_front_points(const FrontPointsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_front_points, dim3(blocks_of((size_t)std::max<long long>(A.scan.n, 1))), dim3(256), 0, s, A);
}

void launch_front_costs(const FrontCostsArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_front_costs, dim3(std::min(blocks_of((size_t)A.f.cells), 16384u)), dim3(256), 0, s, A);
}

}  // namespace tl
