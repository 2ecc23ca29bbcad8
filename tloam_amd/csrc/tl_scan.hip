// tl_scan.hip -- exclusive scans of counts and flags for gfx950: block-local scan + recursive scan of block totals + add, the
// one-block scan of small arrays, and the single-pass scan of large count arrays.  Which of them an array takes is
// tl_grid_plan.hpp's scan_path; the device templates they share with the grid build and the compaction are tl_scan.hpp's.
// Compiled with tl_nn.hip's flags.
#include <atomic>

#include "tl_scan.hpp"

namespace tl {

// tile-local exclusive scans + the tiles' totals.  REZERO: the tile of `in` is left all-zero once it has been read -- the cell
// histogram of a grid build, empty again for the next one (`in` is then written through and promises no aliasing).
template <typename T, bool REZERO> struct ScanIn { typedef const T* __restrict__ type; };
template <typename T> struct ScanIn<T, true> { typedef T* type; };
template <typename T, bool REZERO>
__global__ __launch_bounds__(kScanThreads) void k_scan_tile(typename ScanIn<T, REZERO>::type in, T* __restrict__ out, size_t n,
                                                            T* __restrict__ tile_total, const int* __restrict__ gate) {
  __shared__ T wave_tot[kScanThreads / 64];
  if (gate && *gate == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t wbase = (size_t)blockIdx.x * kScanTile + (size_t)wave * (kScanRows * kScanRowElems);
  T ex[kScanRows], a[kScanRows][kScanPer];
  const T tot = wave_scan_rows<kScanRows>(in, n, wbase, lane, ex, a);
  if constexpr (REZERO) wave_zero_rows<kScanRows>(in, n, wbase, lane);
  if (lane == 0) wave_tot[wave] = tot;
  __syncthreads();
  T wave_off = 0;
  for (int w = 0; w < wave; ++w) wave_off += wave_tot[w];
  wave_store_rows<kScanRows>(out, n, wbase, lane, wave_off, ex, a);
  if (threadIdx.x == kScanThreads - 1) tile_total[blockIdx.x] = wave_off + tot;
}
__global__ __launch_bounds__(kScanThreads) void k_scan_add(unsigned long long* __restrict__ out, size_t n,
                                                           const unsigned long long* __restrict__ tile_off,
                                                           const int* __restrict__ gate) {
  if (gate && *gate == 0) return;
  const unsigned long long add = tile_off[blockIdx.x];
  const size_t base = (size_t)blockIdx.x * kScanTile + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i)
    if (base + (size_t)i * kScanThreads < n) out[base + (size_t)i * kScanThreads] += add;
}
// small inputs (<= 16 Ki elements, e.g. the flag scan of a KITTI-size frame): ONE block of 1024 threads, a
// single pass with every load in flight at once
constexpr int kSmallThreads = 1024;
constexpr int kSmallRows = 4;                                   // 1024 elements per wave
static_assert(kSmallTile == (kSmallThreads / 64) * kSmallRows * kScanRowElems, "16384 elements per round of the block");
__global__ __launch_bounds__(kSmallThreads) void k_scan_small(const unsigned long long* __restrict__ in,
                                                              unsigned long long* __restrict__ out, size_t n,
                                                              const int* __restrict__ gate) {
  __shared__ unsigned long long wave_tot[kSmallThreads / 64];
  __shared__ unsigned long long carry_s;
  if (gate && *gate == 0) return;
  if (threadIdx.x == 0) carry_s = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (size_t tile0 = 0; tile0 < n; tile0 += kSmallTile) {
    const size_t wbase = tile0 + (size_t)wave * (kSmallRows * kScanRowElems);
    unsigned long long ex[kSmallRows], a[kSmallRows][kScanPer];
    const unsigned long long tot = wave_scan_rows<kSmallRows>(in, n, wbase, lane, ex, a);
    if (lane == 0) wave_tot[wave] = tot;
    __syncthreads();
    unsigned long long wave_off = carry_s;
    for (int w = 0; w < wave; ++w) wave_off += wave_tot[w];
    wave_store_rows<kSmallRows>(out, n, wbase, lane, wave_off, ex, a);
    __syncthreads();
    if (threadIdx.x == kSmallThreads - 1) carry_s = wave_off + tot;
    __syncthreads();
  }
}
// medium inputs: every block sums the totals of the tiles before it itself (<= kScanLdsTiles loads) -- two
// launches instead of three
__global__ __launch_bounds__(kScanThreads) void k_scan_add_direct(unsigned long long* __restrict__ out, size_t n,
                                                                  const unsigned long long* __restrict__ tile_total,
                                                                  const int* __restrict__ gate) {
  __shared__ unsigned long long red[kScanThreads / 64];
  if (gate && *gate == 0) return;
  unsigned long long acc = 0;
  for (int t = threadIdx.x; t < (int)blockIdx.x; t += kScanThreads) acc += tile_total[t];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  unsigned long long add = 0;
  for (int w = 0; w < kScanThreads / 64; ++w) add += red[w];
  const size_t base = (size_t)blockIdx.x * kScanTile + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kScanItems; ++i)
    if (base + (size_t)i * kScanThreads < n) out[base + (size_t)i * kScanThreads] += add;
}
// (never the single-pass scan: that one takes control words instead of scratch -- launch_scan_counts_1p, for the caller who asked)
void launch_exclusive_scan_u64(const unsigned long long* in, unsigned long long* out, size_t n,
                               unsigned long long* tmp, hipStream_t s, const int* gate) {
  if (n == 0) return;
  const size_t tiles = scan_tiles(n);
  const ScanPath path = scan_path(n, 0, false).path;
  if (path == ScanPath::ONE_BLOCK) {
    hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(kSmallThreads), 0, s, in, out, n, gate);
    return;
  }
  unsigned long long* totals = tmp;
  unsigned long long* totals_scan = tmp + tiles;
  hipLaunchKernelGGL((k_scan_tile<unsigned long long, false>), dim3((unsigned)tiles), dim3(kScanThreads), 0, s, in, out, n, totals, gate);
  if (path == ScanPath::TILES) {
    hipLaunchKernelGGL(k_scan_add_direct, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, out, n, totals, gate);
  } else {
    launch_exclusive_scan_u64(totals, totals_scan, tiles, tmp + 2 * tiles, s, gate);
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)tiles), dim3(kScanThreads), 0, s, out, n, totals_scan, gate);
  }
}

// the single-pass scan (tl_scan.hpp has how it works)
__global__ __launch_bounds__(kScanThreads) void k_scan_1p(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                          size_t n, Scan1p C) {
  unsigned long long ex[kRows1p], a[kRows1p][kScanPer], base;
  size_t wbase;
  (void)scan1p_tile(in, n, C, ex, a, &base, &wbase);
  wave_store_rows<kRows1p>(out, n, wbase, threadIdx.x & 63, base, ex, a);
}
unsigned next_scan_epoch() {
  static std::atomic<unsigned> e{0};
  return e.fetch_add(1u, std::memory_order_relaxed) % 0x3ffffffeu + 1u;
}
void launch_scan_counts_1p(const unsigned long long* in, unsigned long long* out, size_t n, unsigned long long* ctl, unsigned* fault,
                           hipStream_t s) {
  Scan1p C{ctl, next_scan_epoch(), fault};
  hipLaunchKernelGGL(k_scan_1p, dim3((unsigned)scan_1p_tiles(n)), dim3(kScanThreads), 0, s, in, out, n, C);
}

// first half of the medium-size scan only: tile-local exclusive scans + per-tile totals (the consumer adds the tiles'
// offsets itself, see k_compact and k_grid_finalize_scatter_all).  Returns the number of tiles; 0 = not applicable (use the full scan).
int scan_tiles_only(const unsigned long long* in, unsigned long long* out, size_t n, unsigned long long* totals, hipStream_t s,
                    const int* gate) {
  const int tiles = scan_path(n, 0, false).tiles;
  if (tiles > 0)
    hipLaunchKernelGGL((k_scan_tile<unsigned long long, false>), dim3((unsigned)tiles), dim3(kScanThreads), 0, s, in, out, n, totals, gate);
  return tiles;
}
void launch_grid_scan_tiles(unsigned* cell_cnt, unsigned* cell_scan, size_t n, unsigned* totals, hipStream_t s) {
  hipLaunchKernelGGL((k_scan_tile<unsigned, true>), dim3((unsigned)scan_tiles(n)), dim3(kScanThreads), 0, s, cell_cnt, cell_scan, n,
                     totals, (const int*)nullptr);
}

}  // namespace tl
