// tl_snapshot.hip -- the device side of the closed map's snapshot (tl_api_snapshot.hip).
//
// A section of the blob is m 64-bit words w_i, and its checksum is sum_i mix64(w_i + kSnapGolden * (i + 1)) mod 2^64: an integer
// sum, the same in any order.  Both kernels walk a list of pieces (SnapPiece: a run of words of one section) with a thread per
// word -- blockIdx.y is the piece, a grid-stride loop covers its words -- sum per wave by shuffles and add the wave's partial
// to the section's control word with one integer atomic.
//   k_snap_pack    grid (blocks, pieces) x 256   copies every piece to its place in the blob and sums it
//   k_snap_check   grid (blocks, pieces) x 256   sums every piece of an uploaded blob and tests its words: database doubles
//                                                finite; the key's three 21-bit axis fields in [1, 2^21 - 1], bit 63 clear;
//                                                1 <= N <= 2^30 (and the sum of N); 0 <= Q <= N * 2^24 against the N of the
//                                                same row; M >= 0; Ns, Sxx, Syy, Szz >= 0.  Failures are counted, never acted on
//   k_snap_table   grid x 256, twice             id_table_insert of every id, then id_table_find(key_i) == i
// The same launches for every blob.  Nothing read from a blob is ever an index: a word's row, axis and column come from its
// position, every bound from the launch arguments the host has checked.
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__device__ __forceinline__ unsigned long long snap_term(unsigned long long w, unsigned long long i) {
  return mix64(w + kSnapGolden * (i + 1ull));
}

// 1 when word j of piece P fails the piece's test; *n_add: what an N adds to the sum of N
__device__ __forceinline__ unsigned snap_test(const SnapPiece& P, unsigned long long j, unsigned long long w, unsigned long long* n_add) {
  const long long v = (long long)w;
  switch (P.test) {
    case kSnapTestFinite: return ((w >> 52) & 0x7ffull) == 0x7ffull;
    case kSnapTestKey: {
      unsigned bad = (w >> 63) != 0ull;
#pragma unroll
      for (int a = 0; a < 3; ++a) bad |= ((w >> (21 * a)) & 0x1fffffull) == 0ull;
      return bad;
    }
    case kSnapTestN: {
      const bool ok = v >= 1 && v <= kSnapMaxN;
      if (ok) *n_add = w;
      return !ok;
    }
    case kSnapTestQ: {
      const long long N = P.aux[j % P.aux_n];
      if (N < 1 || N > kSnapMaxN) return 0u;   // (counted where N is tested)
      return v < 0 || v > (N << 24);
    }
    case kSnapTestMiss: return v < 0;
    case kSnapTestSums: {
      const unsigned k = (unsigned)(j % (unsigned long long)kSurfelSums);
      return (k == 0u || k == 4u || k == 7u || k == 9u) && v < 0;
    }
    default: return 0u;
  }
}

// the control word that counts the failures of test t (SnapTest 1 .. 6 -> kSnapBadFinite .. kSnapBadSums, in that order)
__device__ __forceinline__ int snap_fail_word(int t) { return kSnapBadFinite - 1 + t; }
static_assert(kSnapBadFinite - 1 + kSnapTestSums == kSnapBadSums, "SnapTest and SnapCtl are listed in the same order");

template <bool kCheck>
__device__ __forceinline__ void snap_body(const SnapPieces& A) {
  const SnapPiece& P = A.piece[blockIdx.y];
  const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
  unsigned long long sum = 0ull, bad = 0ull, nsum = 0ull;
  for (unsigned long long j = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; j < P.words; j += stride) {
    const unsigned long long w = P.src[j];
    sum += snap_term(w, P.first + j);
    if (kCheck) bad += snap_test(P, j, w, &nsum);
    else if (P.dst) P.dst[j] = w;
  }
  sum = wave_sum(sum);
  if (kCheck) {
    bad = wave_sum(bad);
    nsum = wave_sum(nsum);
  }
  if ((threadIdx.x & 63) == 0) {
    if (sum) atomicAdd(&A.ctl[P.section], sum);
    if (kCheck && bad) atomicAdd(&A.ctl[snap_fail_word(P.test)], bad);
    if (kCheck && nsum) atomicAdd(&A.ctl[kSnapSumN], nsum);
  }
}

__global__ __launch_bounds__(256) void k_snap_pack(SnapPieces A) { snap_body<false>(A); }
__global__ __launch_bounds__(256) void k_snap_check(SnapPieces A) { snap_body<true>(A); }

template <bool kVerify>
__global__ __launch_bounds__(256) void k_snap_table(VmapTable T, long long n, unsigned long long* ctl) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) {
    if (kVerify) bad = id_table_find(T.ptab, T.pmask, T.pkey, T.pkey[i]) != (int)i;
    else id_table_insert(T.ptab, T.pmask, T.pkey[i], (int)i);
  }
  if (kVerify) {
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctl[kSnapBadFind], (unsigned long long)__popcll(b));
  }
}

dim3 snap_grid(const SnapPieces& A) {
  unsigned long long most = 1;
  for (int p = 0; p < A.npieces; ++p) most = std::max(most, A.piece[p].words);
  return dim3(std::min(blocks_of((size_t)most), 2048u), (unsigned)std::max(A.npieces, 1));
}

}  // namespace

void launch_snap_pack(const SnapPieces& A, hipStream_t s) {
  hipLaunchKernelGGL(k_snap_pack, snap_grid(A), dim3(256), 0, s, A);
}

void launch_snap_check(const SnapPieces& A, hipStream_t s) {
  hipLaunchKernelGGL(k_snap_check, snap_grid(A), dim3(256), 0, s, A);
}

void launch_snap_table(const VmapTable& T, size_t n, unsigned long long* ctl, hipStream_t s) {
  const dim3 grid(blocks_of(std::max<size_t>(n, 1)));   // (nothing still launches)
  hipLaunchKernelGGL(k_snap_table<false>, grid, dim3(256), 0, s, T, (long long)n, ctl);
  hipLaunchKernelGGL(k_snap_table<true>, grid, dim3(256), 0, s, T, (long long)n, ctl);
}

}  // namespace tl
