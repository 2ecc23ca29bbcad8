// tl_place.hip -- the device side of place recognition (tl_api_place.hip): the Scan Context descriptor of a
// scan, its keys, the keyframe database's commit, and the search of a new keyframe against the earlier ones.
//
// Launches per keyframe (after the frame's last wait, not waited for; none of them reads anything the frame still writes):
//   k_place_bin    grid x 256   per return: ring and sector in fp64, v = z + height_offset as an order-preserving integer image;
//                               runs of equal bins among a wave's consecutive lanes (returns arrive in firing order) folded by
//                               a segmented max over shuffles, one 64-bit atomic maximum per run
//   k_place_keys   1 x 512      the images decoded into the descriptor (an empty bin, image 0, is 0.0) and zeroed for the next
//                               scan; ring keys (one lane per ring) and sector keys (one lane per sector) summed in index order;
//                               the commit: the keyframe's frame number and pose
// when keyframes 0 .. q - exclude_recent exist:
//   k_place_rank   1 x 256      squared ring-key distances summed over rings in order; the ncand smallest, ties to the lower
//                               id, by ncand rounds of a block argmin
//   k_place_shift  ncand x 64k  a workgroup per candidate, a lane per shift: column norms in LDS, d(s) summed over columns in
//                               order; the block's argmin (ties to the lower shift)
//                               (the relocalisation of DESIGN.md section 24 runs these two with a query that is no keyframe:
//                               q_desc, q_ring_key)
//   k_place_pick   1 x 64       the best pair over the candidates (d, then shift, then keyframe id); d < dist_thres appends a
//                               loop record
// Compiled with -ffp-contract=off: every sum, product and quotient rounds as tests/place_np.py restates it.
#include <algorithm>

#include "tl_common.hpp"

namespace tl {
namespace {

constexpr double kTwoPi = 2.0 * kPi;

__device__ __forceinline__ unsigned long long okey(double v) {   // order-preserving: larger v, larger image; 0 is below all
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double from_okey(unsigned long long k) {
  if (k == 0ull) return 0.0;
  return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}

__global__ __launch_bounds__(256) void k_place_bin(PlaceDescArgs A) {
  const int lane = threadIdx.x & 63;
  const double ring_w = A.max_radius / (double)A.R, sector_w = kTwoPi / (double)A.S;
  const long long stride = (long long)gridDim.x * 256;
  // every lane of a wave takes the same number of turns: the shuffles below see the whole wave
  for (long long base = (long long)blockIdx.x * 256; base < A.n; base += stride) {
    const long long i = base + threadIdx.x;
    int bin = -1;
    unsigned long long key = 0ull;
    if (i < A.n) {
      const double x = A.aos[3 * i], y = A.aos[3 * i + 1], z = A.aos[3 * i + 2];
      const double r = sqrt(x * x + y * y);
      if (x - x == 0.0 && y - y == 0.0 && z - z == 0.0 && r > 0.0 && r < A.max_radius) {
        const int ring = min((int)floor(r / ring_w), A.R - 1);
        const int sector = min((int)floor((atan2(y, x) + kPi) / sector_w), A.S - 1);
        bin = ring * A.S + sector;
        key = okey(z + A.height_offset);
      }
    }
    const int bprev = __shfl_up(bin, 1, 64), bnext = __shfl_down(bin, 1, 64);
    const bool head = bin >= 0 && !(lane > 0 && bprev == bin);
    const bool tail = bin >= 0 && !(lane < 63 && bnext == bin);
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
    const int hl = (heads & upto) ? 63 - __clzll(heads & upto) : lane;   // the head of this lane's run
    // inclusive max over [hl, lane]: after the step of `off`, lane covers [max(hl, lane - 2 off + 1), lane]
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long o = __shfl_up(key, off, 64);
      if (lane - off >= hl) key = o > key ? o : key;
    }
    if (tail) atomicMax(&A.bins[bin], key);
  }
}

__global__ __launch_bounds__(512) void k_place_keys(PlaceDescArgs A) {
  const int t = threadIdx.x, RS = A.R * A.S;
  for (int b = t; b < RS; b += 512) {
    A.desc[b] = from_okey(A.bins[b]);
    A.bins[b] = 0ull;   // (ready for the next scan)
  }
  __syncthreads();   // (the block's global writes are visible to the block after the barrier)
  if (t < A.R) {
    double acc = 0.0;
    for (int j = 0; j < A.S; ++j) acc = acc + A.desc[t * A.S + j];
    A.ring_key[t] = acc / (double)A.S;
  } else if (t < A.R + A.S) {
    const int j = t - A.R;
    double acc = 0.0;
    for (int i = 0; i < A.R; ++i) acc = acc + A.desc[i * A.S + j];
    A.sector_key[j] = acc / (double)A.R;
  }
  if (A.pose_out && t < 16) A.pose_out[t] = A.pose[t];
  if (A.frame_out && t == 0) *A.frame_out = A.frame;
}

// (d, id) lexicographic: a before b
__device__ __forceinline__ bool before(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

__global__ __launch_bounds__(256) void k_place_rank(PlaceSearchArgs A) {
  __shared__ double s_d[4];
  __shared__ int s_i[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const double* kq = A.q_ring_key ? A.q_ring_key : A.ring_key + (size_t)A.q * A.R;
  for (int j = t; j < A.m; j += 256) {
    const double* kc = A.ring_key + (size_t)j * A.R;
    double acc = 0.0;
    for (int i = 0; i < A.R; ++i) {
      const double e = kq[i] - kc[i];
      acc = acc + e * e;
    }
    A.kdist[j] = acc;
    A.taken[j] = 0;
  }
  __syncthreads();
  for (int r = 0; r < A.ncand; ++r) {
    double bd = 0.0;
    int bi = -1;
    for (int j = t; j < A.m; j += 256) {
      if (A.taken[j]) continue;
      const double d = A.kdist[j];
      if (bi < 0 || before(d, j, bd, bi)) { bd = d; bi = j; }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (oi >= 0 && (bi < 0 || before(od, oi, bd, bi))) { bd = od; bi = oi; }
    }
    if (lane == 0) { s_d[wave] = bd; s_i[wave] = bi; }
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < 4; ++w)
        if (s_i[w] >= 0 && (bi < 0 || before(s_d[w], s_i[w], bd, bi))) { bd = s_d[w]; bi = s_i[w]; }
      A.cand[r].keyframe = bi;   // (ncand <= m: always one left)
      A.taken[bi] = 1;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(384) void k_place_shift(PlaceSearchArgs A) {
  __shared__ double s_nq[kPlaceMaxSectors], s_nc[kPlaceMaxSectors];
  __shared__ double s_d[6];
  __shared__ int s_s[6];
  const int s = threadIdx.x, lane = s & 63, wave = s >> 6, S = A.S, R = A.R;
  const size_t RS = (size_t)R * S;
  const int c = A.cand[blockIdx.x].keyframe;
  const double* __restrict__ dq = A.q_desc ? A.q_desc : A.desc + (size_t)A.q * RS;
  const double* __restrict__ dc = A.desc + (size_t)c * RS;
  if (s < S) {
    double aq = 0.0, ac = 0.0;
    for (int i = 0; i < R; ++i) {
      const double vq = dq[(size_t)i * S + s], vc = dc[(size_t)i * S + s];
      aq = aq + vq * vq;
      ac = ac + vc * vc;
    }
    s_nq[s] = sqrt(aq);
    s_nc[s] = sqrt(ac);
  }
  __syncthreads();
  double d = __builtin_inf();   // (lanes past the last shift never win: d is finite for every real shift)
  int shift = 0x7fffffff;
  if (s < S) {
    double total = 0.0;
    int nv = 0;
    for (int j = 0; j < S; ++j) {
      int js = j + s;
      if (js >= S) js -= S;
      const double nq = s_nq[j], nc = s_nc[js];
      if (nq == 0.0 || nc == 0.0) continue;
      double dot = 0.0;
      for (int i = 0; i < R; ++i) dot = dot + dq[(size_t)i * S + j] * dc[(size_t)i * S + js];
      total = total + dot / (nq * nc);
      ++nv;
    }
    d = nv ? 1.0 - total / (double)nv : 1.0;
    shift = s;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(d, off, 64);
    const int os = __shfl_xor(shift, off, 64);
    if (before(od, os, d, shift)) { d = od; shift = os; }
  }
  if (lane == 0) { s_d[wave] = d; s_s[wave] = shift; }
  __syncthreads();
  if (s == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
      if (before(s_d[w], s_s[w], d, shift)) { d = s_d[w]; shift = s_s[w]; }
    A.cand[blockIdx.x].d = d;
    A.cand[blockIdx.x].shift = shift;
  }
}

__global__ __launch_bounds__(64) void k_place_pick(PlaceSearchArgs A) {
  if (threadIdx.x != 0) return;
  PlaceCandidate b = A.cand[0];
  for (int r = 1; r < A.ncand; ++r) {
    const PlaceCandidate o = A.cand[r];
    if (o.d < b.d || (o.d == b.d && (o.shift < b.shift || (o.shift == b.shift && o.keyframe < b.keyframe)))) b = o;
  }
  if (!(b.d < A.dist_thres)) return;
  const unsigned long long at = *A.n_loops;
  tloam_place_loop L;
  L.query_keyframe = A.q;
  L.query_frame = A.frames[A.q];
  L.match_keyframe = b.keyframe;
  L.match_frame = A.frames[b.keyframe];
  L.shift = b.shift;
  L.reserved0 = 0;
  L.dist = b.d;
  double yaw = (double)b.shift * (kTwoPi / (double)A.S);
  if (yaw > kPi) yaw = yaw - kTwoPi;
  L.yaw = yaw;
  A.loops[at] = L;
  *A.n_loops = at + 1ull;
}

}  // namespace

void launch_place_describe(const PlaceDescArgs& A, hipStream_t s) {
  if (A.n > 0) {
    const unsigned blocks = (unsigned)std::min<long long>((A.n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_place_bin, dim3(blocks), dim3(256), 0, s, A);
  }
  hipLaunchKernelGGL(k_place_keys, dim3(1), dim3(512), 0, s, A);
}

void launch_place_candidates(const PlaceSearchArgs& A, hipStream_t s) {
  if (A.m <= 0 || A.ncand <= 0) return;
  hipLaunchKernelGGL(k_place_rank, dim3(1), dim3(256), 0, s, A);
  const unsigned threads = (unsigned)((A.S + 63) / 64 * 64);
  hipLaunchKernelGGL(k_place_shift, dim3((unsigned)A.ncand), dim3(threads), 0, s, A);
}

void launch_place_search(const PlaceSearchArgs& A, hipStream_t s) {
  if (A.m <= 0 || A.ncand <= 0) return;
  launch_place_candidates(A, s);
  hipLaunchKernelGGL(k_place_pick, dim3(1), dim3(64), 0, s, A);
}

}  // namespace tl
