// tl_odom.hip -- the device side of the odometry frame (tl_api_odom.hip): what the stage chain's host
// glue did with numpy between the stages, done where the clouds already are.
//
// Launches:
//   k_gather_lists  grid x jobs  up to eight index lists -> point rows at once (blockIdx.y = job): the general points for the
//                                PCA stage, the edge / ground points for the per-scan voxel job, the four source clouds into
//                                the registered frame's block, the planar selection + edge / ground into the submap update's
//                                ring block.  Pure copies: the rows are the bytes the host glue would have uploaded.
//   k_odom_counts   1 x 256      the lengths of the scan selections of extractPlanarSphere (:178-190) from the ranked lists,
//                                and the sizes of the voxel job, into one control block the host reads with the PCA sizes
#include "tl_common.hpp"

namespace tl {
namespace {

__global__ __launch_bounds__(256) void k_gather_lists(GatherArgs A) {
  const GatherJob& J = A.j[blockIdx.y];
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  const int m = J.count ? min(J.n, *J.count) : J.n;
  if (i >= m) return;
  int p = J.idx1 ? J.idx1[i] : i;
  if (J.idx2) {
    if (p < 0 || p >= J.n1) return;
    p = J.idx2[p];
  }
  if (p < 0 || p >= J.src_n) return;
  const size_t s = (size_t)p * J.ss, d = (size_t)i * J.ds;
  const double x = J.sx[s], y = J.sy[s], z = J.sz[s];
  J.dx[d] = x; J.dy[d] = y; J.dz[d] = z;
}

// the planar scan selection keeps rank id where id < planar_num || flatness[id] > planar_scan_thres; the sphere one where
// id < sphere_num || flatness[id] > cvr_scan (:178-190).  Both lists are ranked by flatness, descending: the kept ranks are a
// prefix, whose length is the first rank that fails
__device__ __forceinline__ int kept_prefix(const double* f, int m, int num, double thr, int* s_min) {
  if (threadIdx.x == 0) *s_min = m;
  __syncthreads();
  int first = m;
  for (int id = (int)threadIdx.x; id < m; id += 256)
    if (!(id < num || f[id] > thr)) { first = id; break; }
  if (first < m) atomicMin(s_min, first);
  __syncthreads();
  const int r = *s_min;
  __syncthreads();
  return r;
}
__global__ __launch_bounds__(256) void k_odom_counts(OdomCountArgs A) {
  __shared__ int s_min;
  const unsigned long long t = *A.total;
  const int np = (int)(t >> 32), ns = (int)(t & 0xffffffffull);
  const int nps = kept_prefix(A.ranked, np, A.planar_num, A.planar_scan_thres, &s_min);
  const int nss = kept_prefix(A.ranked + np, ns, A.sphere_num, A.cvr_scan, &s_min);
  if (threadIdx.x == 0) {
    A.ctl[0] = np; A.ctl[1] = ns; A.ctl[2] = nps; A.ctl[3] = nss;
    A.ctl[4] = A.vox_n ? (int)A.vox_n[0] : 0;
    A.ctl[5] = A.vox_n ? (int)A.vox_n[1] : 0;
    A.ctl[6] = A.vox_overflow ? *A.vox_overflow : 0;
    A.ctl[7] = 0;
  }
}

}  // namespace

void launch_gather_lists(const GatherArgs& A, int jobs, hipStream_t s) {
  int nmax = 0;
  for (int j = 0; j < jobs; ++j) nmax = std::max(nmax, A.j[j].n);
  if (jobs <= 0 || nmax <= 0) return;
  hipLaunchKernelGGL(k_gather_lists, dim3((unsigned)((nmax + 255) / 256), (unsigned)jobs), dim3(256), 0, s, A);
}
void launch_odom_counts(const OdomCountArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(k_odom_counts, dim3(1), dim3(256), 0, s, A);
}

}  // namespace tl
