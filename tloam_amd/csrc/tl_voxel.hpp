// tl_voxel.hpp -- what the device voxel grids share: the submap's down-sample (tl_submap.hip), the
// global map (tl_map.hip), the merged voxel map (tl_vmap.hip), the closed map (tl_cmap.hip), its carve (tl_carve.hip), its
// surfels (tl_surfel.hip), the localiser (tl_localise.hip), the diff (tl_diff.hip), the ray-cast (tl_raycast.hip) and the free
// space (tl_free.hip).  One definition each of the key hash,
// the two table inserts and the slot table's lookup, of the wave's integer sum, its add to a control word (wave_add) and the
// four-state ballot count (wave_count_states), of the wave's maximum and a block's counters folded with one atomic each a block
// (wave_max, block_fold: k_clear_count, k_route_count, the frontiers' counts), of a wave's prefix sum and a run's sum from it
// (wave_scan, run_sum: k_surfel_accum, k_front_accum), of a query point's cell (route_cell), of a cell's key and voxel (cell_key, cell_voxel) and the 27-cell probe round a
// point's cell (probe27: k_loc_sweep, k_diff_points), of the block scans, of the single-pass
// look-back with its one bound, of the eight-word post to the host, of the voxel map's key / q arithmetic, its row centroid
// and its run sums, of the compacting box read's body (k_vmap_box, k_carve_box, k_surfel_box, k_diff_box), of the surfel gate,
// of an incremental add's numbering and row update (k_vmap_emit / k_vmap_commit, k_ext_emit / k_ext_commit),
// of the span table's search and its point, and of a ray's set-up, step and walks through a map's grid (MapGrid: k_carve_rays,
// k_diff_rays, k_cast_rays, k_free_rays); the carve gate the queries share is tl_common.hpp's CarveGate; and of
// PointCloud2::VoxelDownSample's arithmetic for the two units that restate it (the min bound's hand-over and finish, the voxel
// key of a point, the leader's local sum, the blocks of an emit kernel the device holds at once).
// Device code, and the launches' blocks_of and emit_resident_blocks.
// An includer must be compiled with -ffp-contract=off: vmap_quantise and centroid are the bit-for-bit contract of DESIGN.md 14,
// voxel_min_bound, voxel_key and leader_local_sum that of the oracle's pc_voxel_down_sample.
#pragma once

#include <atomic>

#include "tl_common.hpp"

namespace tl {

// The key of a free slot in every grid's open-addressing table: a voxel key never has all bits set (the voxel map's has bit 63
// clear; the submap's all-ones key is refused at its insert).
constexpr unsigned long long kFree = ~0ull;

// splitmix64 finaliser: the slot a key starts probing at is mix64(key) & mask.
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// `key` entered in the table keys[mask + 1] (free slots hold kFree, linear probing): the slot that holds it, the same for every
// caller with that key.  The table's load is at most 1/2, so a slot is found.  *was_free: this call took the slot.
__device__ __forceinline__ unsigned long long table_enter(unsigned long long* keys, unsigned long long mask, unsigned long long key,
                                                          bool* was_free) {
  unsigned long long h = mix64(key) & mask;
  for (;;) {
    const unsigned long long prev = atomicCAS(&keys[h], kFree, key);
    if (prev == kFree) { *was_free = true; break; }
    if (prev == key) break;
    h = (h + 1) & mask;
  }
  return h;
}
__device__ __forceinline__ unsigned long long table_enter(unsigned long long* keys, unsigned long long mask, unsigned long long key) {
  bool unused = false;
  return table_enter(keys, mask, key, &unused);
}

// `id` entered in the slot -> id table ptab[pmask + 1] (-1: free) at the first free slot from its key's.  Each id is entered once.
__device__ __forceinline__ void id_table_insert(int* ptab, unsigned long long pmask, unsigned long long key, int id) {
  for (unsigned long long t = mix64(key) & pmask;; t = (t + 1) & pmask)
    if (atomicCAS(&ptab[t], -1, id) == -1) break;
}

// the id of voxel `key` in the slot -> id table of a map (read only), -1 when it has none
__device__ __forceinline__ int id_table_find(const int* ptab, unsigned long long pmask, const unsigned long long* pkey,
                                             unsigned long long key) {
  for (unsigned long long t = mix64(key) & pmask;; t = (t + 1) & pmask) {
    const int id = ptab[t];
    if (id < 0) return -1;
    if (pkey[id] == key) return id;
  }
}

// the sum of `v` over the wave's 64 lanes, in every lane (an integer sum: the order does not show)
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// ... and that sum added to a control word: one atomic per wave, none when the sum is zero.  Called by the whole wave.
__device__ __forceinline__ void wave_add(unsigned long long* ctl_word, unsigned long long v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(ctl_word, v);
}
// the largest `v` over the wave's 64 lanes, in every lane
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, off, 64));
  return v;
}
// A block's (256 threads) counters folded into ctl[0 .. NSUM + NMAX): the sums of v[0 .. NSUM) and the maxima of v[NSUM ..), the
// four waves' partials through LDS, one barrier, then one atomic per counter and BLOCK, none for a zero.  Per block and not per
// wave (wave_add): one per wave (as k_free_count, whose grid is 64 times smaller) was 8192 waves' atomics on k_clear_count's
// four words and cost more than the clearance's three passes together.  Called by the whole block, once
// a kernel (the LDS is its own).
template <int NSUM, int NMAX>
__device__ __forceinline__ void block_fold(unsigned long long (&v)[NSUM + NMAX], unsigned long long* ctl) {
  __shared__ unsigned long long s_part[4][NSUM + NMAX];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NSUM + NMAX; ++k) {
    const unsigned long long w = k < NSUM ? wave_sum(v[k]) : wave_max(v[k]);
    if ((threadIdx.x & 63) == 0) s_part[wave][k] = w;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < NSUM) {
    const unsigned long long w = s_part[0][k] + s_part[1][k] + s_part[2][k] + s_part[3][k];
    if (w) atomicAdd(&ctl[k], w);
  } else if (k < NSUM + NMAX) {
    const unsigned long long w = max(max(s_part[0][k], s_part[1][k]), max(s_part[2][k], s_part[3][k]));
    if (w) atomicMax(&ctl[k], w);
  }
}
// The wave's live lanes counted by `state` (0 .. 3) into ctl[0 .. 3] by ballot: one atomic per state and wave.  Called by the
// whole wave.
__device__ __forceinline__ void wave_count_states(bool live, int state, unsigned long long* ctl) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long bal = __ballot(live && state == k);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&ctl[k], (unsigned long long)__popcll(bal));
  }
}

// 256-thread blocks over n items; a launch that runs for nothing too asks for blocks_of(max(n, 1))
inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

// The block's place in the order the blocks START, from a counter that is zero before the launch; ends in a barrier.  A block
// that looks back over places below its own then only ever waits for blocks that are running.
template <typename Bid, typename Ctr>
__device__ __forceinline__ Bid block_ticket(Ctr* ticket, Bid* s_bid) {
  if (threadIdx.x == 0) *s_bid = (Bid)atomicAdd(ticket, (Ctr)1);
  __syncthreads();
  return *s_bid;
}

// Block-wide (256 threads) exclusive scan of one flag per thread by ballot and popcount: *pos = flags set in the threads below
// this one, *total = flags set in the block.  One barrier; s_wave[4] is free again after the caller's next barrier.
template <typename T>
__device__ __forceinline__ void block_flag_scan(bool flag, T* s_wave, int* pos, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long bal = __ballot(flag);
  if (lane == 0) s_wave[wave] = (T)__popcll(bal);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    before += w < wave ? (int)s_wave[w] : 0;
    all += (int)s_wave[w];
  }
  *pos = before + __popcll(bal & ((1ull << lane) - 1ull));
  *total = all;
}

// The same for a 64-bit word per thread that packs several counts (the submap's two segments in one word), by shuffles:
// *before = the sum of `v` over the threads below this one, *total = over the block.  No field may overflow into the next.
__device__ __forceinline__ void block_packed_scan(unsigned long long v, unsigned long long* s_wave, unsigned long long* before,
                                                  unsigned long long* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  unsigned long long wave_base = 0ull, block_total = 0ull;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) wave_base += s_wave[w];
    block_total += s_wave[w];
  }
  *before = wave_base + (incl - v);
  *total = block_total;
}

// The single-pass look-back: the sum of `block_total` over the blocks of places below `bid`.  look[] (one word per block, zero
// before the launch) carries a status in its top two bits -- 1: the block's own total, 2: the total up to and including the block
// -- over 62 bits of count; all its accesses are relaxed atomics at agent scope.  A block publishes 1, walks down adding totals
// until it meets a 2, then publishes its own 2.  Thread 0 only.
// The wait on a word that is still 0 is BOUNDED, here and nowhere else: kLookTimeout ticks of wall_clock64 (100 MHz: ~1 s),
// the clock polled every 64th spin with s_sleep(1) between spins.  Places come from block_ticket, or from blockIdx while the host
// knows the whole grid resident, so the bound is never met on a healthy device; when it is, `fault.raise()` runs before the
// (wrong) prefix is published, and the host discards the result.  The two ways of raising:
constexpr unsigned long long kLookTimeout = 100000000ull;
struct LookFaultDevice {   // a 64-bit control word in device memory, read by the host after the stream has drained
  unsigned long long* word;
  __device__ __forceinline__ void raise() const {
    __hip_atomic_store(word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
  }
};
struct LookFaultHost {     // a 32-bit word of pinned host memory (null: none), read by the host while the stream runs
  unsigned* word;
  __device__ __forceinline__ void raise() const {
    if (word) { __hip_atomic_store(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); __threadfence_system(); }
  }
};
template <typename Bid, typename Fault>
__device__ __forceinline__ unsigned long long lookback_prefix(unsigned long long* look, Bid bid, unsigned long long block_total,
                                                              Fault fault) {
  unsigned long long prefix = 0ull;
  if (bid == 0) {
    __hip_atomic_store(&look[0], (2ull << 62) | block_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    __hip_atomic_store(&look[bid], (1ull << 62) | block_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = wall_clock64();
    unsigned spins = 0;
    for (Bid p = bid - 1;;) {
      const unsigned long long w = __hip_atomic_load(&look[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned st = (unsigned)(w >> 62);
      if (st == 0u) {
        if ((++spins & 63u) == 0 && wall_clock64() - t0 > kLookTimeout) {   // a block in front never started
          fault.raise();
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        continue;
      }
      prefix += w & ~(3ull << 62);
      if (st == 2u) break;
      --p;
    }
    __hip_atomic_store(&look[bid], (2ull << 62) | (prefix + block_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return prefix;
}

// Eight words to a pinned 64-byte segment the host polls (tlh::wait_segment): lanes 0..6 bring the payload words in `w`, lane 7
// stores check_mix(host_seq) XOR seg_word of the seven, so that a torn or stale segment reads as "not there yet".  One
// system-scope store per lane.  Called by threads 0..7 of one wave, all of them.
__device__ __forceinline__ void post_host_segment(unsigned long long* host_seg, unsigned long long host_seq, unsigned long long w,
                                                  int tid) {
  unsigned long long x = tid < 7 ? seg_word(w, tid) : 0ull;
  x ^= __shfl_xor(x, 1, 64);
  x ^= __shfl_xor(x, 2, 64);
  x ^= __shfl_xor(x, 4, 64);
  if (tid == 7) w = check_mix(host_seq) ^ x;
  __hip_atomic_store(&host_seg[tid], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- PointCloud2::VoxelDownSample (PointCloud2.cpp:358-403): what the submap's job (tl_submap.hip) and the global map's
// (tl_map.hip) restate of it, once.  Bit for bit the oracle's pc_voxel_down_sample; the transformed point they start from is
// map_transform_point (tl_common.hpp) ----
// voxel_min_bound = GetMinBound() - voxel_size * 0.5 (:366), finished inside the launch that finds the minima.  m[]: this
// thread's minima (+inf: none) of columns [col0, col0 + NM) of the C = 3 per segment columns.  The block's minima go to row
// `row` of min_partial[rows][C] (+inf in the other columns) with agent-scope stores, their completion is waited for, then the
// block takes a ticket (zero before the launch); the LAST of the `rows` blocks folds the rows, one wave per column (min is exact
// in any order), writes vmin[a] = min - voxel[a / 3] * 0.5 -- an empty cloud has min bound 0 -- and re-arms the ticket.
// Called by the whole block (256 threads).
template <int NM, int C>
__device__ __forceinline__ void voxel_min_bound(const double (&m)[NM], int col0, double* min_partial, int row, int rows, int* ticket,
                                                const double* voxel, double* vmin) {
  __shared__ double sm[NM][256];
  __shared__ int s_last;
  const int tid = threadIdx.x;
#pragma unroll
  for (int a = 0; a < NM; ++a) sm[a][tid] = m[a];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st)
#pragma unroll
      for (int a = 0; a < NM; ++a) sm[a][tid] = fmin(sm[a][tid], sm[a][tid + st]);
    __syncthreads();
  }
  if (tid < C) {
    const double v = (tid >= col0 && tid < col0 + NM) ? sm[tid - col0][0] : __builtin_inf();
    __hip_atomic_store(min_partial + (size_t)row * C + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) s_last = (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == rows - 1) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  const int wave = tid >> 6, lane = tid & 63;
  for (int a = wave; a < C; a += 4) {
    double v = __builtin_inf();
    for (int b = lane; b < rows; b += 64)
      v = fmin(v, __hip_atomic_load(min_partial + (size_t)b * C + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    if (!(v < __builtin_inf())) v = 0.0;
    if (lane == 0) vmin[a] = v - voxel[(C > 3 && a >= 3) ? 1 : 0] * 0.5;
  }
  if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed
}

// ref_coord = (p - voxel_min_bound) / voxel_size; index = int(floor(ref_coord)) (:380-383), packed 3 x 21 bits.  false: an index
// leaves [0, 2^21) -- "[VoxelDownSample] voxel_size is too small." (:370-372); *key is then not to be used.
__device__ __forceinline__ bool voxel_key(double x, double y, double z, const double* vmin, double voxel, unsigned long long* key) {
  const long long ix = (long long)floor((x - vmin[0]) / voxel);
  const long long iy = (long long)floor((y - vmin[1]) / voxel);
  const long long iz = (long long)floor((z - vmin[2]) / voxel);
  if (ix < 0 || iy < 0 || iz < 0 || ix >= (1ll << 21) || iy >= (1ll << 21) || iz >= (1ll << 21)) return false;
  *key = (unsigned long long)ix | ((unsigned long long)iy << 21) | ((unsigned long long)iz << 42);
  return true;
}

// AccumulatedPoint: point_ += p in index order (:253-272).  s_mem[q * 256 + tid], q < k <= kVoxLocal: the members of this
// thread's voxel in any order (conflict-free columns); they are ordered by index (insertion sort: the order AddPoint is called
// in, :379-385) and the points summed in that order.  GetAveragePoint's division by double(num) is the caller's.
__device__ __forceinline__ void leader_local_sum(int* s_mem, int k, const double* __restrict__ x, const double* __restrict__ y,
                                                 const double* __restrict__ z, double* sx, double* sy, double* sz) {
  const int tid = threadIdx.x;
  for (int a = 1; a < k; ++a) {
    const int key = s_mem[a * 256 + tid];
    int b = a - 1;
    while (b >= 0 && s_mem[b * 256 + tid] > key) { s_mem[(b + 1) * 256 + tid] = s_mem[b * 256 + tid]; --b; }
    s_mem[(b + 1) * 256 + tid] = key;
  }
  double ax = 0.0, ay = 0.0, az = 0.0;
  for (int q = 0; q < k; ++q) {
    const int j = s_mem[q * 256 + tid];
    ax += x[j]; ay += y[j]; az += z[j];
  }
  *sx = ax; *sy = ay; *sz = az;
}

// Blocks of 256 threads of an emit kernel the device holds at once, with room to spare for whatever else is on it: a grid of up
// to that many takes its look-back places from blockIdx.  per_cu_cache: the kernel's own (-1 before the first call; one kernel,
// one architecture: the same for every gfx950 device of the process; contexts are created from several host threads -- an atomic,
// and two threads that both find it unset both store the same value)
template <class Kernel>
inline int emit_resident_blocks(Kernel kernel, std::atomic<int>& per_cu_cache, int device_cus) {
  int per_cu = per_cu_cache.load(std::memory_order_relaxed);
  if (per_cu < 0) {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 256, 0) != hipSuccess || occ < 1) { (void)hipGetLastError(); occ = 1; }
    per_cu = occ;
    per_cu_cache.store(occ, std::memory_order_relaxed);
  }
  const long long all = (long long)device_cus * per_cu;
  return (int)(all - all / 16);
}

// ---- the voxel map's grid (the merged voxel map and the closed map): DESIGN.md 14 states this arithmetic, and here it is ----
// Per axis s = (p - origin) / voxel, i = floor(s), q = floor((s - i) * 2^24 + 0.5) in [0, 2^24] (s - i and the scaling are
// exact); the key packs i + 2^kVmapBits of each axis in 21 bits.  A point with |i| >= 2^kVmapBits on an axis (an infinite s
// too) is beyond the grid: *key and q[] are then not to be used.
enum VmapCell { kVmapNotFinite = 0, kVmapInside = 1, kVmapBeyond = 2 };
__device__ __forceinline__ VmapCell vmap_quantise(const double p[3], const double origin[3], double voxel, unsigned long long* key,
                                                  unsigned q[3]) {
  if (!(__builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]))) return kVmapNotFinite;
  bool over = false;
  unsigned long long k = 0ull;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s = (p[a] - origin[a]) / voxel;
    const double f = floor(s);
    if (!(fabs(f) < (double)(1ll << kVmapBits))) { over = true; continue; }
    q[a] = (unsigned)(long long)floor((s - f) * kVmapQScale + 0.5);
    k |= (unsigned long long)((long long)f + (1ll << kVmapBits)) << (21 * a);
  }
  *key = k;
  return over ? kVmapBeyond : kVmapInside;
}

// the voxel index of axis `a` out of a key
__device__ __forceinline__ long long key_axis(unsigned long long key, int a) {
  return (long long)((key >> (21 * a)) & 0x1fffffull) - (1ll << kVmapBits);
}

// a query's point (point g of the scan, through its pose when `posed`) -> its cell; false: an INVALID point (the route's and the
// frontiers' point queries, the route's goals and starts)
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

// the key of cell (cx, cy, cz), |c| < 2^kVmapBits on every axis (the pack vmap_quantise forms)
__device__ __forceinline__ unsigned long long cell_key(int cx, int cy, int cz) {
  const int lim = 1 << kVmapBits;
  return (unsigned long long)(cx + lim) | ((unsigned long long)(cy + lim) << 21) | ((unsigned long long)(cz + lim) << 42);
}
// the id of the voxel of cell (cx, cy, cz) in a map's slot table (read only); -1: the cell is beyond the grid or has no voxel
__device__ __forceinline__ int cell_voxel(const VmapTableView& map, int cx, int cy, int cz) {
  const int lim = 1 << kVmapBits;
  if (cx <= -lim || cx >= lim || cy <= -lim || cy >= lim || cz <= -lim || cz >= lim) return -1;
  return id_table_find(map.ptab, map.pmask, map.pkey, cell_key(cx, cy, cz));
}
// The 27 cells around the cell of `key`, dz outermost, then dy, dx innermost, each -1 .. 1 (the order decides ties between equal
// distances: k_loc_sweep, k_diff_points): visit(id, own) for every one of them that has a voxel, own: the cell of `key` itself.
// (A built map's slot table is always there, all slots free when the map has no voxel: the probes need no guard.)
template <class Visit>
__device__ __forceinline__ void probe27(const VmapTableView& map, unsigned long long key, Visit visit) {
  const int i0 = (int)key_axis(key, 0), i1 = (int)key_axis(key, 1), i2 = (int)key_axis(key, 2);
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int id = cell_voxel(map, i0 + dx, i1 + dy, i2 + dz);
        if (id >= 0) visit(id, dx == 0 && dy == 0 && dz == 0);
      }
}

// c = o + v * ((double) i + ((double) Q / (double) N) * 2^-24), in that order
__device__ __forceinline__ double centroid(double o, double v, long long i, long long Q, long long N) {
  return o + v * ((double)i + ((double)Q / (double)N) * (1.0 / kVmapQScale));
}

// the row of voxel `id`: its centroid and its count
__device__ __forceinline__ void voxel_centroid(const VmapTableView& T, const double origin[3], double voxel, size_t id, double c[3],
                                               long long* N) {
  const unsigned long long key = T.pkey[id];
  const long long n = T.pn[id];
  const long long Q[3] = {T.pqx[id], T.pqy[id], T.pqz[id]};
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = centroid(origin[a], voxel, key_axis(key, a), Q[a], n);
  *N = n;
}

// The compacting box read of one block: the voxels of ids [R.first, R.first + R.count) with N >= R.min_count, inside the box
// (inclusive) when `boxed`, that X keeps, written in id order (block scan + look-back over start tickets); the last block leaves
// their number in R.ctl[2].  What the three reads differ in is X:
//   X.keep(id, n, c)   the read's own test of a voxel of count n and centroid c
//   X.emit(id, p, n)   writes the read's own columns of voxel id at place p, and returns what goes to R.out_n
struct BoxPlain {   // the plain read: the box and min_count decide, N is the count
  __device__ __forceinline__ bool keep(size_t, long long, const double*) const { return true; }
  __device__ __forceinline__ long long emit(size_t, size_t, long long n) const { return n; }
};
template <class Extra>
__device__ __forceinline__ void voxel_box_body(const VmapReadArgs& R, bool boxed, int nblocks, const Extra& X) {
  __shared__ unsigned long long s_wave[4];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_bid;
  const int tid = threadIdx.x;
  const int bid = block_ticket(&R.ctl[0], &s_bid);
  const size_t id = R.first + (size_t)bid * 256 + tid;
  double c[3] = {0.0, 0.0, 0.0};
  long long n = 0;
  bool sel = false;
  if (id < R.first + R.count) {
    voxel_centroid(R.map, R.origin, R.voxel, id, c, &n);
    sel = n >= R.min_count;
    if (boxed) {
#pragma unroll
      for (int a = 0; a < 3; ++a) sel = sel && c[a] >= R.lo[a] && c[a] <= R.hi[a];
    }
    sel = sel && X.keep(id, n, c);
  }
  int pos, total;
  block_flag_scan(sel, s_wave, &pos, &total);
  if (tid == 0) s_prefix = lookback_prefix(R.look, bid, (unsigned long long)total, LookFaultDevice{&R.ctl[1]});
  __syncthreads();
  if (sel) {
    const size_t p = (size_t)(s_prefix + pos);
    if (R.out_c) { R.out_c[3 * p] = c[0]; R.out_c[3 * p + 1] = c[1]; R.out_c[3 * p + 2] = c[2]; }
    const long long count = X.emit(id, p, n);
    if (R.out_n) R.out_n[p] = count;
  }
  if (bid == nblocks - 1 && tid == 0) R.ctl[2] = s_prefix + total;
}

// the surfel gate, for the box read (k_surfel_box) and the localiser's records (k_loc_prepare) alike: solved, not a point, thin
// enough and planar enough
__device__ __forceinline__ bool surfel_gate(long long ns, const double ev[3], int min_points, double max_sigma2,
                                            double min_planarity) {
  return ns >= (long long)min_points && ev[2] > 0.0 && ev[0] <= max_sigma2 && (ev[1] - ev[0]) >= min_planarity * ev[2];
}

// inclusive prefix sum of `v` over the wave's lanes (k_surfel_accum's moments, k_front_accum's counts)
template <typename T>
__device__ __forceinline__ T wave_scan(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}
// the sum of `v` over lanes [head_lane, this lane] from its inclusive prefix sum
template <typename T>
__device__ __forceinline__ T run_sum(T incl, int head_lane) {
  const T below = __shfl(incl, head_lane > 0 ? head_lane - 1 : 0, 64);
  return incl - (head_lane > 0 ? below : (T)0);
}

// Runs of equal keys among a wave's consecutive `ok` lanes (neighbouring returns of a ring share their voxel), summed by
// shuffles so that a run costs the table one insert and four atomics instead of one each per point.  Called by the whole wave.
// head / tail: this lane begins / ends its run; head_lane: the lane that begins it (the run's smallest point index);
// sum[]: at the tail, the run's N, Qx, Qy, Qz (64 * 2^24 fits 32 bits).  What a lane that is not ok passes in q is ignored.
struct WaveRun {
  bool head, tail;
  int head_lane;
  unsigned sum[4];
};
__device__ __forceinline__ WaveRun wave_run_sums(bool ok, unsigned long long key, const unsigned q[3]) {
  const int lane = threadIdx.x & 63;
  WaveRun r;
  const unsigned long long kprev = __shfl_up(key, 1, 64), knext = __shfl_down(key, 1, 64);
  const unsigned long long okb = __ballot(ok);
  const bool ok_prev = lane > 0 && ((okb >> (lane - 1)) & 1ull);
  const bool ok_next = lane < 63 && ((okb >> (lane + 1)) & 1ull);
  r.head = ok && !(ok_prev && kprev == key);
  r.tail = ok && !(ok_next && knext == key);
  const unsigned long long heads = __ballot(r.head);
  const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
  const int hl = (heads & upto) ? 63 - __clzll(heads & upto) : 0;
  r.head_lane = hl;
  unsigned v[4] = {ok ? 1u : 0u, q[0], q[1], q[2]};   // inclusive prefix sums over the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned o = __shfl_up(v[k], off, 64);
      if (lane >= off) v[k] += o;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned b = __shfl(v[k], hl > 0 ? hl - 1 : 0, 64);
    r.sum[k] = v[k] - (hl > 0 ? b : 0u);
  }
  return r;
}

// ---- an incremental add to a map in id order (the merged voxel map's frame, tl_vmap.hip; the closed map's extension,
// tl_extend.hip): the staged voxels numbered, then committed ----
// The id of a staged voxel, at its leader (-1 in every other thread): the one its key has in the persistent table (read only), or
// base + its place among the fresh leaders of the whole launch, in leader order (block scan + look-back over start tickets `bid`,
// the bounded wait raising *fault).  *upto: the fresh voxels of this block and of every block before it.  Called by the whole block.
template <typename Bid>
__device__ __forceinline__ int staged_voxel_id(bool leader, unsigned long long key, unsigned long long pmask, const int* ptab,
                                               const unsigned long long* pkey, long long base, unsigned long long* look, Bid bid,
                                               unsigned long long* fault, unsigned long long* s_wave, unsigned long long* s_prefix,
                                               unsigned long long* upto) {
  const int found = leader ? id_table_find(ptab, pmask, pkey, key) : -1;
  const bool fresh = leader && found < 0;
  int pos, total;
  block_flag_scan(fresh, s_wave, &pos, &total);
  if (threadIdx.x == 0) *s_prefix = lookback_prefix(look, bid, (unsigned long long)total, LookFaultDevice{fault});
  __syncthreads();
  *upto = *s_prefix + (unsigned long long)total;
  return !leader ? -1 : fresh ? (int)(base + (long long)(*s_prefix + pos)) : found;
}

// A staged voxel's sums into row `id` (one staged voxel per id: plain stores and adds); a fresh one is keyed and entered in the
// table (load <= 1/2: a free slot is found).
__device__ __forceinline__ void staged_voxel_commit(const VmapTable& P, int id, bool fresh, unsigned long long key, long long n,
                                                    long long qx, long long qy, long long qz) {
  if (fresh) {
    P.pkey[id] = key;
    P.pn[id] = n; P.pqx[id] = qx; P.pqy[id] = qy; P.pqz[id] = qz;
    id_table_insert(P.ptab, P.pmask, key, id);
  } else {
    P.pn[id] += n; P.pqx[id] += qx; P.pqy[id] += qy; P.pqz[id] += qz;
  }
}

// ---- a span table in global point order (SpanInput: the closed map's build, its carve and its surfels) ----
// the last span of [lo, hi] that starts at or before g
__device__ __forceinline__ int span_of(const CmapSpan* sp, int lo, int hi, long long g) {
  while (lo < hi) {
    const int m = (lo + hi + 1) >> 1;
    if (sp[m].start <= g) lo = m;
    else hi = m - 1;
  }
  return lo;
}

// the spans of the block's first and last point, found once per block: a point then searches between them (usually one span).
__device__ __forceinline__ void block_spans(const SpanInput& W, int s_span[2]) {
  if (threadIdx.x == 0) {
    const long long first = (long long)blockIdx.x * 256;
    const long long last = first + 255 < W.n ? first + 255 : W.n - 1;
    int lo = 0, hi = 0;
    if (first < W.n) {
      lo = span_of(W.span, 0, W.nspan - 1, first);
      hi = span_of(W.span, lo, W.nspan - 1, last);
    }
    s_span[0] = lo;
    s_span[1] = hi;
  }
  __syncthreads();
}

// point g (< in.n) of the table, its span searched between s_lo and s_hi: its keyframe, that keyframe's pose, the point under it
__device__ __forceinline__ void span_point(const SpanInput& in, long long g, int s_lo, int s_hi, int* kf, const double** P,
                                           double E[3]) {
  const CmapSpan S = in.span[span_of(in.span, s_lo, s_hi, g)];
  const double* x = in.arena + S.off + 3 * (g - S.start);
  *kf = S.kf;
  *P = in.pose + 16 * (size_t)S.kf;
  map_transform_point(*P, x[0], x[1], x[2], &E[0], &E[1], &E[2]);
}

// ---- a ray through a voxel map's grid (the carve, tl_carve.hip; the diff, tl_diff.hip; section 28: the
// ray-cast, tl_raycast.hip) ----
// The ray from O to E through a map's grid (MapGrid): the skip rule, the set-up of the walk through the grid's cells and its step
// exist once (RayCells: ray_begin, ray_key, ray_step); tl_carve.hip's header states their operation order.  The state is held in named scalars (no run-time indexed
// array: no scratch).  Two walks run on it: ray_walk visits the start cell and the first n - 1 cells stepped into and puts the
// miss test to every voxel among them (the carve, the diff); ray_first_hit visits the end cell too and stops at the first voxel
// its test accepts (the ray-cast).
struct RayCells {
  double Dx, Dy, Dz, DD, L;    // D = E - O, DD = |D|^2 summed (x + y) + z, L = sqrt(DD)
  int cx, cy, cz;              // the current cell
  int ex, ey, ez;              // the end cell
  int stx, sty, stz;
  double tx, ty, tz;           // tMax: +inf on an axis that steps no more
  double tdx, tdy, tdz;        // tDelta (not read on an axis that never steps)
  int n;                       // the steps from the start cell to the end cell
};
// false: the ray is skipped (E not finite, L > max_range, L == 0, the cell of O or of E beyond the grid)
__device__ __forceinline__ bool ray_begin(const MapGrid& W, double max_range, double Ox, double Oy, double Oz, double Ex, double Ey,
                                          double Ez, RayCells* R) {
  const double kInf = __builtin_huge_val(), kLimit = (double)(1ll << kVmapBits);
  const double Dx = Ex - Ox, Dy = Ey - Oy, Dz = Ez - Oz;
  const double DD = (Dx * Dx + Dy * Dy) + Dz * Dz;
  const double L = sqrt(DD);
  const double s0x = (Ox - W.origin[0]) / W.voxel, s0y = (Oy - W.origin[1]) / W.voxel, s0z = (Oz - W.origin[2]) / W.voxel;
  const double s1x = (Ex - W.origin[0]) / W.voxel, s1y = (Ey - W.origin[1]) / W.voxel, s1z = (Ez - W.origin[2]) / W.voxel;
  const double fx = floor(s0x), fy = floor(s0y), fz = floor(s0z), gx = floor(s1x), gy = floor(s1y), gz = floor(s1z);
  bool ok = __builtin_isfinite(Ex) && __builtin_isfinite(Ey) && __builtin_isfinite(Ez);
  ok = ok && !(L > max_range) && !(L == 0.0);
  ok = ok && fabs(fx) < kLimit && fabs(fy) < kLimit && fabs(fz) < kLimit && fabs(gx) < kLimit && fabs(gy) < kLimit &&
       fabs(gz) < kLimit;
  if (!ok) return false;
  R->Dx = Dx; R->Dy = Dy; R->Dz = Dz; R->DD = DD; R->L = L;
  const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
  const int ex = (int)gx, ey = (int)gy, ez = (int)gz;
  R->cx = cx; R->cy = cy; R->cz = cz;
  R->ex = ex; R->ey = ey; R->ez = ez;
  const double dx = s1x - s0x, dy = s1y - s0y, dz = s1z - s0z;
  R->stx = dx > 0.0 ? 1 : dx < 0.0 ? -1 : 0; R->sty = dy > 0.0 ? 1 : dy < 0.0 ? -1 : 0; R->stz = dz > 0.0 ? 1 : dz < 0.0 ? -1 : 0;
  R->tx = cx == ex ? kInf : dx > 0.0 ? ((fx + 1.0) - s0x) / dx : dx < 0.0 ? (fx - s0x) / dx : kInf;
  R->ty = cy == ey ? kInf : dy > 0.0 ? ((fy + 1.0) - s0y) / dy : dy < 0.0 ? (fy - s0y) / dy : kInf;
  R->tz = cz == ez ? kInf : dz > 0.0 ? ((fz + 1.0) - s0z) / dz : dz < 0.0 ? (fz - s0z) / dz : kInf;
  R->tdx = (double)R->stx / dx; R->tdy = (double)R->sty / dy; R->tdz = (double)R->stz / dz;
  R->n = abs(ex - cx) + abs(ey - cy) + abs(ez - cz);
  return true;
}
// the current cell's key
__device__ __forceinline__ unsigned long long ray_key(const RayCells& R) { return cell_key(R.cx, R.cy, R.cz); }
// into the next cell: the axis of the smallest tMax, a tie going to the lowest axis
__device__ __forceinline__ void ray_step(RayCells* R) {
  const double kInf = __builtin_huge_val();
  const bool y = R->ty < R->tx;
  const bool z = R->tz < (y ? R->ty : R->tx);
  if (z) {
    R->cz += R->stz;
    R->tz = R->cz == R->ez ? kInf : R->tz + R->tdz;
  } else if (y) {
    R->cy += R->sty;
    R->ty = R->cy == R->ey ? kInf : R->ty + R->tdy;
  } else {
    R->cx += R->stx;
    R->tx = R->cx == R->ex ? kInf : R->tx + R->tdx;
  }
}

// the tMax of the axis ray_step is about to take (its axis choice: the smallest, a tie going to the lowest axis), read before
// the step: the entry parameter t_in of the cell the step leads into (the free walk, tl_free.hip; the clearance's segments)
__device__ __forceinline__ double ray_next_t(const RayCells& R) {
  const bool y = R.ty < R.tx;
  const bool z = R.tz < (y ? R.ty : R.tx);
  return z ? R.tz : y ? R.ty : R.tx;
}

// Every visited cell looked up in the map's slot table, the miss test against an occupied cell's centroid (radius2 = radius *
// radius).  on_miss(id) is what a miss does; *skipped, *steps, *tested, *misses are set for the ray (a skipped ray: 1, 0, 0, 0).
template <class OnMiss>
__device__ __forceinline__ void ray_walk(const MapGrid& W, double max_range, double end_margin, double radius2, double Ox, double Oy,
                                         double Oz, double Ex, double Ey, double Ez, unsigned long long* skipped,
                                         unsigned long long* steps, unsigned long long* tested, unsigned long long* misses,
                                         OnMiss on_miss) {
  const VmapTableView& map = W.map;
  RayCells R;
  if (!ray_begin(W, max_range, Ox, Oy, Oz, Ex, Ey, Ez, &R)) {
    *skipped = 1ull;
    return;
  }
  const double tlim = 1.0 - end_margin / R.L;
  *steps = (unsigned long long)R.n;
  for (int k = 0; k < R.n; ++k) {
    const int id = id_table_find(map.ptab, map.pmask, map.pkey, ray_key(R));
    if (id >= 0) {
      (*tested)++;
      const long long N = map.pn[id];
      const double ux = centroid(W.origin[0], W.voxel, R.cx, map.pqx[id], N) - Ox;
      const double uy = centroid(W.origin[1], W.voxel, R.cy, map.pqy[id], N) - Oy;
      const double uz = centroid(W.origin[2], W.voxel, R.cz, map.pqz[id], N) - Oz;
      const double tt = ((ux * R.Dx + uy * R.Dy) + uz * R.Dz) / R.DD;
      const double wx = ux - tt * R.Dx, wy = uy - tt * R.Dy, wz = uz - tt * R.Dz;
      if (0.0 <= tt && tt < tlim && (wx * wx + wy * wy) + wz * wz <= radius2) {
        (*misses)++;
        on_miss(id);
      }
    }
    ray_step(&R);
  }
}

// The walk that stops: the start cell, then every cell stepped into, the end cell included (n + 1 cells), each looked up in the
// map's slot table; test(id) is put to every voxel among them and the first one it accepts ends the walk.  Returns that voxel's
// id, or -1 when no visited voxel is accepted; *visited: the cells looked up, the accepted one included.
template <class Test>
__device__ __forceinline__ int ray_first_hit(const VmapTableView& map, RayCells* R, unsigned long long* visited, Test test) {
  unsigned long long seen = 0ull;
  int got = -1;
  for (int k = 0; k <= R->n; ++k) {
    const int id = id_table_find(map.ptab, map.pmask, map.pkey, ray_key(*R));
    ++seen;
    if (id >= 0 && test(id)) {
      got = id;
      break;
    }
    if (k < R->n) ray_step(R);
  }
  *visited = seen;
  return got;
}

// ---- the free-space grid's cells (tl_free.hip; section 30: the clearance built from them, tl_clear.hip) ----
// the brick word of cell (cx, cy, cz), -1 outside the box
__device__ __forceinline__ long long free_brick(const FreeGrid& g, int cx, int cy, int cz) {
  const unsigned bx = (unsigned)((cx >> 2) - g.blo[0]), by = (unsigned)((cy >> 2) - g.blo[1]), bz = (unsigned)((cz >> 2) - g.blo[2]);
  if (!(bx < (unsigned)g.nb[0] && by < (unsigned)g.nb[1] && bz < (unsigned)g.nb[2])) return -1;
  return ((long long)bz * g.nb[1] + (long long)by) * g.nb[0] + (long long)bx;
}
__device__ __forceinline__ unsigned long long free_bit(int cx, int cy, int cz) {
  return 1ull << (((cz & 3) << 4) | ((cy & 3) << 2) | (cx & 3));
}
// the id of the voxel of cell (cx, cy, cz) when it has one that counts, else -1
__device__ __forceinline__ int free_counting_voxel(const FreeQuery& q, int cx, int cy, int cz) {
  const int id = cell_voxel(q.grid.map, cx, cy, cz);
  return id >= 0 && q.gate.counts(q.grid.map, id) ? id : -1;
}
// the occupancy of cell (cx, cy, cz), |c| < 2^kVmapBits (TLOAM_OCCUPANCY_*: never INVALID); *id: its counting voxel or -1
__device__ __forceinline__ int free_cell_state(const FreeQuery& q, int cx, int cy, int cz, int* id) {
  *id = free_counting_voxel(q, cx, cy, cz);
  if (*id >= 0) return TLOAM_OCCUPANCY_OCCUPIED;
  const long long idx = free_brick(q.g, cx, cy, cz);
  const bool seen = idx >= 0 && (q.g.words[idx] & free_bit(cx, cy, cz)) != 0ull;
  return seen ? TLOAM_OCCUPANCY_FREE : TLOAM_OCCUPANCY_UNKNOWN;
}

}  // namespace tl
