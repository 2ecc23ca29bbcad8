// tl_deskew.hip -- the device side of the odometry frame's deskew (tl_api_deskew.hip): every return of
// the scan moved from the sensor frame of its firing time to the sensor frame at the pose's instant, under constant velocity.
//
// One launch, grid-stride over the returns (a later frame with deskew on, after the upload, before the first gather):
//   k_deskew     grid x 256   per return: its sweep time s (from the azimuth, or from its time), exp(s xi) applied with the
//                             Sophus branches of tl_se3.hpp, the corrected return written; the largest |p' - p| of a wave
//                             reduced by shuffles and taken into one device word with an atomic maximum of its bits
// Compiled with -ffp-contract=off: s, the exponential and the point action round as tests/deskew_np.py restates them.
#include <algorithm>

#include "tl_common.hpp"

namespace tl {
namespace {

constexpr double kTwoPi = 2.0 * kPi;

__device__ __forceinline__ bool finite3(double x, double y, double z) {
  return x - x == 0.0 && y - y == 0.0 && z - z == 0.0;   // false for NaN and +-Inf
}

__global__ __launch_bounds__(256) void k_deskew(DeskewArgs A) {
  double worst = 0.0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += stride) {
    const double x = A.in[3 * i], y = A.in[3 * i + 1], z = A.in[3 * i + 2];
    double s;
    if (A.t) {
      s = A.t[i] / A.period;
      if (!(fabs(s) <= 2.0)) {   // a non-finite time, or one more than two sweeps away: the frame is refused
        *A.bad = 1ull;
        s = 0.0;
      }
    } else {
      const double f = A.direction * (atan2(y, x) - A.start);
      double w = f - kTwoPi * floor(f / kTwoPi);
      if (w >= kTwoPi) w = 0.0;   // (a tiny negative f rounds up to 2 pi)
      s = w / kTwoPi - A.ref;
    }
    if (!A.out) continue;
    double qx = x, qy = y, qz = z;
    if (s != 0.0 && finite3(x, y, z)) {
      double a[6];
      for (int k = 0; k < 6; ++k) a[k] = s * A.xi[k];
      const Vec3 q = act(se3_exp(a), Vec3{x, y, z});
      qx = q.x; qy = q.y; qz = q.z;
      const double dx = qx - x, dy = qy - y, dz = qz - z;
      worst = fmax(worst, sqrt(dx * dx + dy * dy + dz * dz));
    }
    A.out[3 * i] = qx; A.out[3 * i + 1] = qy; A.out[3 * i + 2] = qz;
  }
  if (!A.max_shift) return;
  for (int off = 32; off > 0; off >>= 1) worst = fmax(worst, __shfl_xor(worst, off, 64));
  // (a non-negative double orders as its bits do)
  if ((threadIdx.x & 63) == 0 && worst > 0.0) atomicMax(A.max_shift, (unsigned long long)__double_as_longlong(worst));
}

}  // namespace

void launch_deskew(const DeskewArgs& A, hipStream_t s) {
  if (A.n <= 0) return;
  const unsigned blocks = (unsigned)std::min<long long>((A.n + 255) / 256, 2048);
  hipLaunchKernelGGL(k_deskew, dim3(blocks), dim3(256), 0, s, A);
}

}  // namespace tl
