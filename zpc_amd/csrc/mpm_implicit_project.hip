// mpm_implicit_project.hip -- ImplicitMPMSystem::project (Projector, simulation/mpm/ImplicitMPM.hpp:61-124) on a dof vector: a node
// with mass gets collider.resolveCollision(pos, vel) at pos = (block key * side + cell) * dx, a node without mass is zeroed.
// A translation unit of its own because it is built with -ffp-contract=off like collider.hip (collider_device.hpp: the finite-difference
// normals must round like the reference's); the rest of the implicit system (mpm_implicit.hip) calls zsr::implicit_project_enqueue.
#include "common.hpp"
#include "bht.hpp"
#include "../../include/zensim_rocm/collider_device.hpp"

namespace zsr {

template <int SIDE, bool COLLIDE>
__global__ __launch_bounds__(256) void implicit_project_kernel(ColliderDev col, const int *activeKeys, const float *grid, float *dof, size_t nblocks,
                                                               float dx, int kscale) {
  constexpr int NC = SIDE * SIDE * SIDE;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nblocks * NC) return;
  const size_t blk = gid / NC;
  const int cell = (int)(gid % NC);
  float *v = dof + 3 * gid;
  if (!(grid[blk * 7 * NC + cell] > 0.f)) {  // clear non-dof nodes as well (ImplicitMPM.hpp:85-88)
    v[0] = v[1] = v[2] = 0.f;
    return;
  }
  if constexpr (COLLIDE) {
    const int cc[3] = {cell / (SIDE * SIDE), (cell / SIDE) % SIDE, cell % SIDE};
    float pos[3], vel[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int node = activeKeys[3 * blk + d] / kscale * SIDE + cc[d];  // as apply_boundary_kernel forms it
      pos[d] = (float)node * dx;
      vel[d] = v[d];
    }
    if (col.resolveCollision(pos, vel)) {
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d] = vel[d];
    }
  }
}

void implicit_project_enqueue(hipStream_t stream, const zs_rocm_mpm_params *p, const int *activeKeys, const float *grid, size_t nblocks,
                              const zs_rocm_collider *collider, float *inout) {
  if (!nblocks) return;
  const size_t nc = (size_t)p->side * p->side * p->side;
  const int kscale = p->keyIsOrigin ? p->side : 1;
  const dim3 g(ceil_div(nblocks * nc, 256)), b(256);
  const ColliderDev col = collider ? ColliderDev(*collider) : ColliderDev(zs_rocm_collider{});
#define CALL_PROJECT(S)                                                                                                        \
  do {                                                                                                                         \
    if (collider) hipLaunchKernelGGL((implicit_project_kernel<S, true>), g, b, 0, stream, col, activeKeys, grid, inout, nblocks, p->dx, kscale); \
    else hipLaunchKernelGGL((implicit_project_kernel<S, false>), g, b, 0, stream, col, activeKeys, grid, inout, nblocks, p->dx, kscale);        \
  } while (0)
  if (p->side == 4) CALL_PROJECT(4);
  else CALL_PROJECT(8);
#undef CALL_PROJECT
}

}  // namespace zsr
