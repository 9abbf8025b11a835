#pragma once
// mpm_update_stress_kernel.hpp -- update_stress_kernel, launched by zs_rocm_mpm_update_stress (mpm.hip) and by the two-pass P2G
// (mpm_p2g.hip); included by these two units only
#include "mpm_arena.hpp"

namespace zsr {

// stand-alone constitutive update (first step, or after the host changed F / logJp)
template <int SMODEL> __global__ __launch_bounds__(256) void update_stress_kernel(MpmDev mp, ParticlesDev ps) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ps.n) return;
  float F[9], C[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  load_state<model_is_fluid(SMODEL)>(ps.F, i, F);
  if constexpr (model_is_fluid(SMODEL)) load_attr<9>(ps.C, i, C);
  update_stress<SMODEL, 0>(mp, ps, particle_offset<0>(0u, i), F, C);
}

}  // namespace zsr
