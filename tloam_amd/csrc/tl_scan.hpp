// tl_scan.hpp -- the device side of the exclusive scans (tl_scan.hip has the kernels and their launchers): the wave-level row
// scan, the tile offsets a fused consumer forms in LDS, and the single-pass tile with its look-back.  Shared with the kernels that
// scan as part of something else: the grid build's single-pass finalize, finalize + scatter and the compaction (tl_nn.hip).
// The size limits, and which scan an array takes, are tl_grid_plan.hpp's.
#pragma once

#include "tl_common.hpp"
#include "tl_grid_plan.hpp"

namespace tl {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
static_assert(kScanTile == kScanThreads * kScanItems, "2048 elements per block, 512 per wave");
constexpr int kScanPer = 4;                            // consecutive elements per lane within a row
constexpr int kScanRowElems = 64 * kScanPer;           // 256 elements = 2 KiB per wave row
constexpr int kScanRows = kScanTile / (kScanThreads / 64) / kScanRowElems;   // rows per wave (2)

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2), aligned(8)));   // (8-byte aligned: any element of a u64 array)
typedef unsigned u32x4 __attribute__((ext_vector_type(4), aligned(16)));              // (the 32-bit tables: every row starts on 16 bytes)
// a lane's four consecutive elements of a row, in 16-byte accesses: two for u64, ONE for 32-bit counts -- what the CU's L1 is
// asked for is accesses per lane, not bytes (64 eight-byte loads per thread of a 16 Ki tile were half of what the single-pass
// scans waited for)
__device__ __forceinline__ void scan_load4(const unsigned long long* __restrict__ p, unsigned long long (&a)[4]) {
  const u64x2* __restrict__ q = reinterpret_cast<const u64x2*>(p);
  const u64x2 lo = q[0], hi = q[1];
  a[0] = lo.x; a[1] = lo.y; a[2] = hi.x; a[3] = hi.y;
}
__device__ __forceinline__ void scan_load4(const unsigned* __restrict__ p, unsigned (&a)[4]) {
  const u32x4 v = *reinterpret_cast<const u32x4*>(p);
  a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
}
__device__ __forceinline__ void scan_store4(unsigned long long* __restrict__ p, unsigned long long r0, unsigned long long r1,
                                            unsigned long long r2, unsigned long long r3) {
  u64x2* __restrict__ q = reinterpret_cast<u64x2*>(p);
  q[0] = u64x2{r0, r1};
  q[1] = u64x2{r2, r3};
}
__device__ __forceinline__ void scan_store4(unsigned* __restrict__ p, unsigned r0, unsigned r1, unsigned r2, unsigned r3) {
  *reinterpret_cast<u32x4*>(p) = u32x4{r0, r1, r2, r3};
}
// Wave-level exclusive scan of ROWS x 256 consecutive elements starting at `wbase`: lane l holds the four
// elements 4l .. 4l+3 of each row, so a wave instruction covers 1-2 KiB (8-16 cache lines) and one shuffle scan
// serves 256 elements.  The fully blocked layout (8-16 consecutive elements per thread) made every wave
// instruction touch 32-64 different lines, serialised by the texture addresser: 11.9 us for a 9.4 k-element
// scan.  Returns the wave total; out[row i, 4l + j] = ex[i] + a[i][0] + .. + a[i][j-1].
// T: unsigned long long (flag scans, the single-pass count scans) or unsigned (the frame-size cell tables: a count never
// exceeds 2^28 points and the four kinds of a frame share one 2^28 slot space, so every prefix fits 32 bits).
template <int ROWS, typename T>
__device__ __forceinline__ T wave_scan_rows(const T* __restrict__ in, size_t n, size_t wbase, int lane, T (&ex)[ROWS],
                                            T (&a)[ROWS][kScanPer]) {
  static_assert(kScanPer == 4, "a lane's elements of a row are loaded in 16-byte accesses");
  if (wbase + (size_t)ROWS * kScanRowElems <= n) {
    // a wave whose rows all lie inside the array (every wave but the last)
#pragma unroll
    for (int i = 0; i < ROWS; ++i) scan_load4(in + wbase + (size_t)i * kScanRowElems + (size_t)lane * kScanPer, a[i]);
  } else {
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
#pragma unroll
      for (int j = 0; j < kScanPer; ++j) {  // unconditional (clamped) loads: all in flight together
        const size_t idx = wbase + (size_t)i * kScanRowElems + (size_t)lane * kScanPer + j;
        const T x = in[idx < n ? idx : n - 1];
        a[i][j] = idx < n ? x : T(0);
      }
  }
  T carry = 0;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    T s = 0;
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) s += a[i][j];
    T inc = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const T t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    ex[i] = carry + inc - s;
    carry += __shfl(inc, 63, 64);
  }
  return carry;
}
template <int ROWS, typename T>
__device__ __forceinline__ void wave_store_rows(T* __restrict__ out, size_t n, size_t wbase, int lane, T add, const T (&ex)[ROWS],
                                                const T (&a)[ROWS][kScanPer]) {
  if (wbase + (size_t)ROWS * kScanRowElems <= n) {   // (as the loads: 16-byte stores)
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const T r0 = add + ex[i], r1 = r0 + a[i][0], r2 = r1 + a[i][1], r3 = r2 + a[i][2];
      scan_store4(out + wbase + (size_t)i * kScanRowElems + (size_t)lane * kScanPer, r0, r1, r2, r3);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    T run = add + ex[i];
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
      const size_t idx = wbase + (size_t)i * kScanRowElems + (size_t)lane * kScanPer + j;
      if (idx < n) out[idx] = run;
      run += a[i][j];
    }
  }
}
// the rows a wave has just scanned, left all-zero (a histogram emptied for the next build while its lines are in hand)
template <int ROWS, typename T>
__device__ __forceinline__ void wave_zero_rows(T* __restrict__ p, size_t n, size_t wbase, int lane) {
  if (wbase + (size_t)ROWS * kScanRowElems <= n) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) scan_store4(p + wbase + (size_t)i * kScanRowElems + (size_t)lane * kScanPer, T(0), T(0), T(0), T(0));
    return;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i)
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
      const size_t idx = wbase + (size_t)i * kScanRowElems + (size_t)lane * kScanPer + j;
      if (idx < n) p[idx] = T(0);
    }
}
// exclusive prefix of (<= kScanLdsTiles) tile totals into LDS, by a block of 256 threads: 4 consecutive tiles per thread.  Ends
// with a barrier: toff[] may be read on return.
template <typename T>
__device__ __forceinline__ void tile_offsets_to_lds(const T* __restrict__ totals, int tiles, T (&toff)[kScanLdsTiles], T (&wtot)[4]) {
  const int t0 = threadIdx.x * 4;
  T v[4], run = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) { v[u] = (t0 + u < tiles) ? totals[t0 + u] : T(0); run += v[u]; }
  T incl = run;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  T pre = incl - run;
  for (int w = 0; w < wave; ++w) pre += wtot[w];
#pragma unroll
  for (int u = 0; u < 4; ++u) { toff[t0 + u] = pre; pre += v[u]; }
  __syncthreads();
}

// ---- single-pass scan of large COUNT arrays (round 4) --------------------------------------------------------------------------
// The 1 M-class frames scan two histograms of ~3 M entries per frame (cells of the target grids, bins of the query sort): tile
// scan + scan of the tile totals + add = three launches and two passes over the array.  Here ONE launch, one pass: a block
// scans its tile, publishes the tile's total in a status word, looks back over the words of the blocks in front of it (a wave
// reads 64 of them at a time) until it meets one that already carries its inclusive prefix, publishes its own, and emits its
// elements with the prefix added.  At most one block per CU OF THIS DEVICE (scan_path looks at the context's CU count: a
// partitioned or CU-masked part takes the multi-launch scan), so every block is resident at once and a block only ever waits
// for blocks that are running; the wait is bounded all the same (~1 s of the wall clock, then the block raises Scan1p::fault --
// a word in pinned host memory -- and goes on with what it has: the host discards the frame's result, switches the context to
// the multi-launch scans and runs the frame again, tl_api_frames.hip check_device_faults).  Status word: [63:62] 0 nothing |
// 1 the tile's own total | 2 inclusive prefix, [61:32] the launch's epoch -- a word of an earlier launch reads as "nothing",
// so the array is never cleared (it is zeroed when it is allocated) --, [31:0] the value: totals below 2^32, i.e. counts.
// Tiles of 16 Ki elements (64 per thread, in registers): ~200 blocks for 3.2 M entries, all resident at once, so that the
// look-back is three or four reads of 64 status words -- with 2 Ki tiles (1563 blocks, not all resident) the prefix crept from
// block to block at a coherence-point round trip per hop and the launch took 52-57 us, longer than the three launches it replaced.
constexpr int kRows1p = 16;                                                  // rows of 256 elements per wave
static_assert(kTile1p == (kScanThreads / 64) * kRows1p * kScanRowElems, "16384 elements per block");
struct Scan1p {
  unsigned long long* status;   // [tiles]
  unsigned epoch;               // 1 .. 2^30 - 1, different from the previous launch's on the same status array
  unsigned* fault;              // pinned host word raised when the look-back timed out (null: nobody to tell)
};
unsigned next_scan_epoch();   // process-wide (contexts on different host threads share it): any two launches differ
// returns the block's place (tile index); ex / a as wave_scan_rows leaves them, *base = sum of everything in front of this wave
__device__ __forceinline__ int scan1p_tile(const unsigned long long* __restrict__ in, size_t n, const Scan1p& C,
                                           unsigned long long (&ex)[kRows1p], unsigned long long (&a)[kRows1p][kScanPer],
                                           unsigned long long* base, size_t* wbase_out) {
  __shared__ unsigned long long wave_tot[kScanThreads / 64];
  __shared__ unsigned long long s_prefix;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // The block's place is its index: the launcher only uses this kernel when the grid is at most one block per CU of the
  // device in use (scan_path), so every block is resident as soon as the device has room for it and nobody waits for a
  // block that cannot start.  (Places handed out by an atomic counter -- the usual guard -- cost ~10 us here: ~200 returning atomics on
  // one address are served one after the other at the memory side, ~50 ns each.)
  const int bid = (int)blockIdx.x;
  const size_t wbase = (size_t)bid * kTile1p + (size_t)wave * (kRows1p * kScanRowElems);
  const unsigned long long tot = wave_scan_rows<kRows1p>(in, n, wbase, lane, ex, a);
  if (lane == 0) wave_tot[wave] = tot;
  __syncthreads();
  unsigned long long wave_off = 0, block_total = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) wave_off += wave_tot[w];
    block_total += wave_tot[w];
  }
  const unsigned long long tag = (unsigned long long)C.epoch << 32;
  if (wave == 0) {
    unsigned long long prefix = 0ull;
    if (bid == 0) {
      if (lane == 0) __hip_atomic_store(&C.status[0], (2ull << 62) | tag | block_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (lane == 0) __hip_atomic_store(&C.status[bid], (1ull << 62) | tag | block_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long t0 = wall_clock64();
      unsigned spins = 0;
      for (int top = bid - 1;;) {   // lanes look at blocks top, top - 1, ..., top - 63
        const int p = top - lane;
        unsigned long long w = 0ull;
        if (p >= 0) w = __hip_atomic_load(&C.status[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool mine = p >= 0 && ((w >> 32) & 0x3fffffffull) == (unsigned long long)C.epoch;
        const unsigned st = mine ? (unsigned)(w >> 62) : 0u;
        const unsigned long long have = __ballot(p < 0 || st != 0u);          // (lanes past block 0 count as ready, value 0)
        const unsigned long long full = __ballot(p >= 0 && st == 2u);
        // the nearest block that carries an inclusive prefix, provided every block nearer than it has published its total
        const int first_full = full ? __ffsll((long long)full) - 1 : 64;
        const unsigned long long need = first_full >= 63 ? ~0ull : ((2ull << first_full) - 1ull);
        if ((have & need) != need) {   // somebody in the window is not there yet
          if ((++spins & 63u) == 0 && wall_clock64() - t0 > 100000000ull) {   // ~1 s: a block in front never started
            if (lane == 0 && C.fault) { __hip_atomic_store(C.fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); __threadfence_system(); }
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        unsigned long long v = (p >= 0 && lane <= first_full) ? (w & 0xffffffffull) : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        prefix += __shfl(v, 0, 64);
        if (first_full < 64 || top - 64 < 0) break;
        top -= 64;
      }
      if (lane == 0)
        __hip_atomic_store(&C.status[bid], (2ull << 62) | tag | (prefix + block_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) s_prefix = prefix;
  }
  __syncthreads();
  *base = s_prefix + wave_off;
  *wbase_out = wbase;
  return bid;
}

}  // namespace tl
