// tl_raycast.hip -- the device side of the closed map's ray-cast (tl_api_raycast.hip): per segment from the
// pose's translation the first voxel of the closed map it meets, where, and by which test.
//
// One launch, the same for any rays and map (nothing of the closed map, of a carve's counts, of the surfels or of a diff's counts
// is written):
//   k_cast_rays     ceil(n / 256) x 256   per ray: the end transformed, the carve's skip rule and set-up (tl_voxel.hpp: ray_begin),
//                                the walk that stops (ray_first_hit): the start cell, every cell stepped into and the end cell
//                                looked up in the closed map's slot table (id_table_find, read only); of a voxel one LocRecord
//                                (and N and the carve's M when min_count > 1 or the gate is on: CarveGate::counts); status (1 B), range (8 B) and
//                                the optional id (4 B) stored; the four status counts by ballot, steps and tested summed over
//                                the wave by shuffles, one integer atomic per counter and wave
// No block waits on another block.  No floating-point atomics: every sum is an integer, so two calls give the same bytes.  Lanes
// of a wave leave the walk at different steps; the wave runs as long as its longest ray.
//
// Compiled with -ffp-contract=off.  The arithmetic of a ray (tests/closed_map_raycast_np.py restates it):
//   O = (M[12], M[13], M[14]),  E = map_transform_point(M, p);  skip rule, D, DD, L and the walk: tl_carve.hip's header
//   a visited voxel counts when the carve gate says so (tl_common.hpp: CarveGate, the one definition the carved read, the diff and
//   the free space share)
//   R = rec[id]:  u = R.c - O,  tt = ((ux*Dx + uy*Dy) + uz*Dz) / DD,  w = u - tt * D
//   centroid test: 0 <= tt && tt <= 1 && (wx*wx + wy*wy) + wz*wz <= radius2 -> t = tt
//   plane test, instead, when planes != 0 && R.eligible && (den = (nx*Dx + ny*Dy) + nz*Dz) != 0:
//     tp = ((nx*ux + ny*uy) + nz*uz) / den,  e = tp * D - u,  0 <= tp && tp <= 1 && (ex*ex + ey*ey) + ez*ez <= radius2 -> t = tp
//   planes == 2: a voxel that gets no plane test is passed through, and is not `tested`
//   the first hit ends the walk: range = t * L
#include <algorithm>

#include "tl_voxel.hpp"

namespace tl {
namespace {

__global__ __launch_bounds__(256) void k_cast_rays(RaycastWork W) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = g < W.scan.n;
  int status = TLOAM_RAYCAST_SKIPPED;
  unsigned long long steps = 0ull, tested = 0ull;
  if (live) {
    const double* M = W.scan.M;
    double Ex, Ey, Ez;
    map_transform_point(M, W.scan.pts[3 * g], W.scan.pts[3 * g + 1], W.scan.pts[3 * g + 2], &Ex, &Ey, &Ez);
    const double Ox = M[12], Oy = M[13], Oz = M[14];
    RayCells R;
    double range = -1.0;
    int hit = -1;
    if (ray_begin(W.grid, W.max_range, Ox, Oy, Oz, Ex, Ey, Ez, &R)) {
      double t = 0.0;
      status = TLOAM_RAYCAST_MISS;
      hit = ray_first_hit(W.grid.map, &R, &steps, [&](int id) -> bool {
        if (!W.gate.counts(W.grid.map, id)) return false;
        const LocRecord* V = W.rec + id;
        const double ux = V->c[0] - Ox, uy = V->c[1] - Oy, uz = V->c[2] - Oz;
        if (W.planes != 0 && V->eligible) {
          const double nx = V->n[0], ny = V->n[1], nz = V->n[2];
          const double den = (nx * R.Dx + ny * R.Dy) + nz * R.Dz;
          if (den != 0.0) {
            ++tested;
            const double tp = ((nx * ux + ny * uy) + nz * uz) / den;
            const double ex = tp * R.Dx - ux, ey = tp * R.Dy - uy, ez = tp * R.Dz - uz;
            if (0.0 <= tp && tp <= 1.0 && (ex * ex + ey * ey) + ez * ez <= W.radius2) {
              t = tp;
              status = TLOAM_RAYCAST_HIT_PLANE;
              return true;
            }
            return false;
          }
        }
        if (W.planes == 2) return false;
        ++tested;
        const double tt = ((ux * R.Dx + uy * R.Dy) + uz * R.Dz) / R.DD;
        const double wx = ux - tt * R.Dx, wy = uy - tt * R.Dy, wz = uz - tt * R.Dz;
        if (0.0 <= tt && tt <= 1.0 && (wx * wx + wy * wy) + wz * wz <= W.radius2) {
          t = tt;
          status = TLOAM_RAYCAST_HIT_CENTROID;
          return true;
        }
        return false;
      });
      if (hit >= 0) range = t * R.L;
    }
    W.status[g] = (unsigned char)status;
    W.range[g] = range;
    if (W.ids) W.ids[g] = hit;
  }
  wave_count_states(live, status, W.ctl);
  wave_add(&W.ctl[4], steps);
  wave_add(&W.ctl[5], tested);
}

}  // namespace

void launch_raycast(const RaycastWork& W, hipStream_t s) {
  hipLaunchKernelGGL(k_cast_rays, dim3(blocks_of((size_t)std::max<long long>(W.scan.n, 1))), dim3(256), 0, s, W);
}

}  // namespace tl
