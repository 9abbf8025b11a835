#pragma once
// mpm_particles.hpp -- how the MPM kernels see a particle: the B-spline arena of its position, attribute loads / stores (generic ports
// and the one-TileVector fast path), the deformation state, ParticlesDev / MpmDev, and the host side of both (make_dev, make_particles,
// the lane-width / side / model dispatch macros).  No kernel lives here.
#include "mpm_math.hpp"

namespace zsr {

// ======================================================================================= arena
// node k (0, 1, 2) of the stencil minus the local position, k dx - lp -- written without the product (k dx is a loop invariant the compiler
// would keep in a VGPR; 2 dx is exact, so the fma returns the same bits, and 0 dx - lp = -lp up to the sign of a zero)
__device__ __forceinline__ float node_off(float dx, int k, float lp) { return k == 0 ? -lp : (k == 1 ? dx - lp : fmaf(2.f, dx, -lp)); }
// LocalArena<collocated, quadratic> (simulation/Utils.hpp:47-75, InterpolationKernel.hpp:47-55,93-130)
struct Arena {
  int corner[3];
  float lp[3];    // local position * dx
  float w[3][3];  // w[axis][k]
};
// X = pos * (1/dx): the reference divides (simulation/Utils.hpp:52-55); the product differs by <= 1 ulp, which moves
// a weight by O(1e-7) and never changes which bin a particle is stored in because the binning kernel uses this
// same expression.
__device__ __forceinline__ void make_arena(float dx, float dxinv, const float (&pos)[3], Arena &a) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float X = pos[d] * dxinv;
    const float fl = floorf(X - 0.5f);
    a.corner[d] = (int)fl;
    const float lpn = X - fl;
    const float d0 = lpn - floorf(lpn - 0.5f);
    a.w[d][0] = 0.5f * (1.5f - d0) * (1.5f - d0);
    const float d1 = d0 - 1.0f;
    a.w[d][1] = 0.75f - d1 * d1;
    const float zz = 0.5f + d1;
    a.w[d][2] = 0.5f * zz * zz;
    a.lp[d] = lpn * dx;
  }
}
__device__ __forceinline__ void make_arena(float dx, const float (&pos)[3], Arena &a) { make_arena(dx, 1.0f / dx, pos, a); }

__device__ __forceinline__ int floordiv(int a, int b) { return (a + (a < 0 ? -b + 1 : 0)) / b; }

template <int N> __device__ __forceinline__ void load_attr(const Port<float> &p, size_t i, float (&out)[N]) {
  const float *b = p.base + p.off(i);
  const size_t cs = p.cstride();
#pragma unroll
  for (int d = 0; d < N; ++d) out[d] = b[d * cs];
}
template <int N> __device__ __forceinline__ void store_attr(const Port<float> &p, size_t i, const float (&v)[N]) {
  float *b = p.base + p.off(i);
  const size_t cs = p.cstride();
#pragma unroll
  for (int d = 0; d < N; ++d) b[d * cs] = v[d];
}

// Fast particle addressing for the binned kernels.  When every attribute lives in ONE TileVector<f32, LW> (same tile
// width / channel count, iterator index 0 -- the host checks this) the element offset of particle i,
// ((i / LW) * chns) * LW + i % LW, is computed once per particle and every component load/store becomes
// base(SGPR) + offset(VGPR) + d * LW * 4 (immediate): ~1 VALU per attribute instead of ~3 per component.
// LW == 0: generic iterator ports (AoS vectors, mixed layouts).
template <int LW> struct POff { size_t o; };
template <int LW> __device__ __forceinline__ POff<LW> particle_offset(unsigned chns, size_t i) {
  POff<LW> r;
  if constexpr (LW != 0) r.o = ((i / LW) * (size_t)chns) * LW + (i % LW);
  else r.o = i;
  return r;
}
template <int LW, int N> __device__ __forceinline__ void pload(const Port<float> &p, POff<LW> o, float (&out)[N]) {
  if constexpr (LW != 0) {
    const float *b = p.base + o.o;
#pragma unroll
    for (int d = 0; d < N; ++d) {
      out[d] = b[d * LW];
    }
  } else
    load_attr<N>(p, o.o, out);
}
template <int LW> __device__ __forceinline__ float pload1(const Port<float> &p, POff<LW> o, int comp = 0) {
  if constexpr (LW != 0) return p.base[o.o + comp * LW];
  else return p.base[p.off(o.o) + comp * p.cstride()];
}
// NT: tiled particle state written with non-temporal stores (see g2p_packed_kernel)
template <int LW, int N, bool NT = false> __device__ __forceinline__ void pstore(const Port<float> &p, POff<LW> o, const float (&v)[N]) {
  if constexpr (LW != 0) {
    float *b = p.base + o.o;
#pragma unroll
    for (int d = 0; d < N; ++d) {
      if constexpr (NT) __builtin_nontemporal_store(v[d], b + d * LW);
      else b[d * LW] = v[d];
    }
  } else
    store_attr<N>(p, o.o, v);
}
template <int LW, bool NT = false> __device__ __forceinline__ void pstore1(const Port<float> &p, POff<LW> o, float v) {
  if constexpr (LW != 0) {
    if constexpr (NT) __builtin_nontemporal_store(v, p.base + o.o);
    else p.base[o.o] = v;
  } else p.base[p.off(o.o)] = v;
}
// deformation state of a particle: F (9 components) for the solids, the volume ratio J = component 0 of the same attribute
// for the EquationOfState fluid (Structurefree.hpp: particles.F / particles.J)
template <int LW, bool FLUID> __device__ __forceinline__ void pload_state(const Port<float> &p, POff<LW> o, float (&F)[9]) {
  if constexpr (FLUID) {
#pragma unroll
    for (int d = 1; d < 9; ++d) F[d] = 0.f;
    F[0] = pload1<LW>(p, o);
  } else
    pload<LW, 9>(p, o, F);
}
template <int LW, bool FLUID, bool NT = false> __device__ __forceinline__ void pstore_state(const Port<float> &p, POff<LW> o, const float (&F)[9]) {
  if constexpr (FLUID) pstore1<LW, NT>(p, o, F[0]);
  else pstore<LW, 9, NT>(p, o, F);
}
template <bool FLUID> __device__ __forceinline__ void load_state(const Port<float> &p, size_t i, float (&F)[9]) {
  if constexpr (FLUID) {
#pragma unroll
    for (int d = 1; d < 9; ++d) F[d] = 0.f;
    F[0] = p.base[p.off(i)];
  } else
    load_attr<9>(p, i, F);
}
// G2P: F <- (I + dt C) F (G2P.hpp:75-78, MatrixUtils.h:136-146) or J <- (1 + tr(C) dt) J (:70-74)
template <bool FLUID> __device__ __forceinline__ void advance_state(const float (&oldF)[9], const float (&C)[9], float dt, float (&F)[9]) {
  if constexpr (FLUID) {
#pragma unroll
    for (int d = 1; d < 9; ++d) F[d] = 0.f;
    F[0] = (1 + (C[0] + C[4] + C[8]) * dt) * oldF[0];
  } else {
    float tmp[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) tmp[d] = C[d] * dt + ((d & 0x3) ? 0.f : 1.f);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) F[r + 3 * c] = tmp[r] * oldF[3 * c] + tmp[r + 3] * oldF[3 * c + 1] + tmp[r + 6] * oldF[3 * c + 2];
  }
}

struct ParticlesDev {
  Port<float> mass, pos, vel, C, F, logJp, stress;
  size_t n;
};
// third "model" of the P2G kernels: P F^T * vol is read from the particles' `stress` attribute (written by the G2P of
// the previous step, or by zs_rocm_mpm_update_stress) instead of being recomputed
constexpr int MPM_CACHED_STRESS = 100;

struct MpmDev {
  Material mat;
  int model;
  float dx, dt;
  float dxi, D_inv;  // 1 / dx, 4 / dx^2 (host-derived: see Material)
  float fscale, fscaleDx;  // -dt D_inv (contrib = -dt D_inv P F^T vol, P2G.hpp:105), and that times dx
  int kscale;  // partition keys are block coordinates (1: Grids + HashTable/bht convention) or block ORIGINS in cells
               // (SIDE: SparseGrid convention, geometry/SparseGrid.hpp:305-309)
};

// per-particle constitutive update -> contrib = -dt * D_inv * (P F^T vol)   (P2G.hpp:60-105)
template <int MODEL>
__device__ __forceinline__ void particle_contrib(const MpmDev &mp, const ParticlesDev &ps, size_t i, float D_inv, float (&contrib)[9]) {
  float F[9];
  if constexpr (MODEL == MPM_CACHED_STRESS) {
    float S[STRESS_N];
    load_attr<STRESS_N>(ps.stress, i, S);
    stress_unpack(S, contrib);
  } else {
    load_state<model_is_fluid(MODEL)>(ps.F, i, F);
    float Cp[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (model_is_fluid(MODEL)) load_attr<9>(ps.C, i, Cp);
    float lj = 0.f;
    if constexpr (model_uses_logjp(MODEL)) lj = ps.logJp.base[ps.logJp.off(i)];
    model_stress<MODEL>(mp.mat, lj, F, contrib, Cp);
    if constexpr (model_uses_logjp(MODEL)) ps.logJp.base[ps.logJp.off(i)] = lj;  // P2G.hpp:101; the projected F is not written back
  }
#pragma unroll
  for (int d = 0; d < 9; ++d) contrib[d] = contrib[d] * -mp.dt * D_inv;
}

// ======================================================================================= host helpers
// exact-path kernels: grid-stride over a device-side count.  The walk of one particle is a chain of 27 dependent hash
// queries, so the kernel is latency-bound and wants every wave slot of the chip: 8 blocks of 256 per CU (with 256 blocks a
// queue of 640 k particles took 0.37 ms, i.e. half of an 8 M-particle step)
constexpr unsigned STALE_BLOCKS = 2048;
static MpmDev make_dev(const zs_rocm_mpm_params *p) {
  MpmDev d;
  d.model = p->model;
  d.dx = p->dx;
  d.dt = p->dt;
  d.mat.volume = p->volume;
  d.mat.mu = (float)(0.5 * p->E / (1 + p->nu));  // lame_parameters (physics/ConstitutiveModel.hpp:34-38)
  d.mat.lam = (float)(p->E * p->nu / ((1 + p->nu) * (1 - 2 * p->nu)));
  d.mat.cohesion = p->cohesion;
  d.mat.beta = p->beta;
  d.mat.yieldSurface = p->yieldSurface;
  d.mat.volCorrection = p->volCorrection;
  d.mat.yieldStress = p->yieldStress;
  // NACCConfig::bulk() (physics/ConstitutiveModel.hpp:767-769), float arithmetic as written there
  d.mat.bm = 2.f / 3.f * (p->E / (2 * (1 + p->nu))) + (p->E * p->nu / ((1 + p->nu) * (1 - 2 * p->nu)));
  d.mat.xi = p->xi;
  d.mat.Msqr = p->Msqr;
  d.mat.hardeningOn = p->hardeningOn;
  d.mat.bulk = p->bulk;
  d.mat.viscosity = p->viscosity;
  d.kscale = p->keyIsOrigin ? p->side : 1;
  // derived values, in the float arithmetic the kernels used to repeat (IEEE division; fma where the device contracted)
  d.dxi = 1.0f / d.dx;
  d.D_inv = 4.f * d.dxi * d.dxi;
  d.fscale = -d.dt * d.D_inv;
  d.fscaleDx = d.fscale * d.dx;
  d.mat.smu = 2.f * d.mat.mu;
  d.mat.dpCoef = fmaf(3.f, d.mat.lam, d.mat.smu) / d.mat.smu;
  d.mat.expCohesion = expf(d.mat.cohesion);
  return d;
}
static ParticlesDev make_particles(const zs_rocm_particles &p) {
  ParticlesDev d;
  d.mass = make_port<float>(p.mass);
  d.pos = make_port<float>(p.pos);
  d.vel = make_port<float>(p.vel);
  d.C = make_port<float>(p.C);
  d.F = make_port<float>(p.F);
  d.logJp = make_port<float>(p.logJp);
  d.stress = make_port<float>(p.stress);
  d.n = p.n;
  return d;
}

// lane width LW of the fast addressing path (64 or 32) when all used attributes share one TileVector layout, else 0
static int uniform_lane_width(const zs_rocm_particles &p, bool useLogJp, bool useStress) {
  const zs_rocm_attr *a[7] = {&p.mass, &p.pos, &p.vel, &p.C, &p.F, useLogJp ? &p.logJp : nullptr, useStress ? &p.stress : nullptr};
  const zs_rocm_attr &r = p.pos;
  if (r.tileMask != 63u && r.tileMask != 31u) return 0;
  for (auto *q : a) {
    if (!q) continue;
    if (!q->base || q->idx != 0 || q->numTileBits != r.numTileBits || q->tileMask != r.tileMask || q->numChns != r.numChns) return 0;
  }
  if ((1u << r.numTileBits) != r.tileMask + 1u) return 0;
  return (int)r.tileMask + 1;
}
#define ZSR_DISPATCH_LW(lw, CALL, S, M)          \
  do {                                           \
    if ((lw) == 64) { CALL(S, M, 64); }          \
    else if ((lw) == 32) { CALL(S, M, 32); }     \
    else { CALL(S, M, 0); }                      \
  } while (0)

// CALL(SIDE, MODEL) for the runtime (side, model); `other` = the template value for anything that is not one of the four
// constitutive models (MPM_CACHED_STRESS for P2G, -1 = "no constitutive update" for G2P)
#define ZSR_DISPATCH_MODEL_(S, model, other, CALL)                                                        \
  switch (model) {                                                                                        \
    case ZS_MPM_FIXED_COROTATED: { CALL(S, ZS_MPM_FIXED_COROTATED); } break;                              \
    case ZS_MPM_DRUCKER_PRAGER: { CALL(S, ZS_MPM_DRUCKER_PRAGER); } break;                                \
    case ZS_MPM_VONMISES_FIXED_COROTATED: { CALL(S, ZS_MPM_VONMISES_FIXED_COROTATED); } break;            \
    case ZS_MPM_NACC: { CALL(S, ZS_MPM_NACC); } break;                                                    \
    case ZS_MPM_EQUATION_OF_STATE: { CALL(S, ZS_MPM_EQUATION_OF_STATE); } break;                          \
    case MPM_FLUID_NO_STRESS: { CALL(S, MPM_FLUID_NO_STRESS); } break;                                    \
    default: { CALL(S, other); } break;                                                                   \
  }
// the five constitutive models only (callers reject anything else first)
#define ZSR_DISPATCH_PURE_(S, model, CALL)                                                                \
  switch (model) {                                                                                        \
    case ZS_MPM_FIXED_COROTATED: { CALL(S, ZS_MPM_FIXED_COROTATED); } break;                              \
    case ZS_MPM_DRUCKER_PRAGER: { CALL(S, ZS_MPM_DRUCKER_PRAGER); } break;                                \
    case ZS_MPM_VONMISES_FIXED_COROTATED: { CALL(S, ZS_MPM_VONMISES_FIXED_COROTATED); } break;            \
    case ZS_MPM_NACC: { CALL(S, ZS_MPM_NACC); } break;                                                    \
    default: { CALL(S, ZS_MPM_EQUATION_OF_STATE); } break;                                                \
  }
#define ZSR_DISPATCH_SIDE_PURE(side, model, CALL)        \
  do {                                                   \
    if ((side) == 4) { ZSR_DISPATCH_PURE_(4, model, CALL) } \
    else { ZSR_DISPATCH_PURE_(8, model, CALL) }          \
  } while (0)
#define ZSR_DISPATCH_SIDE_MODEL(side, model, CALL)                          \
  do {                                                                      \
    if ((side) == 4) { ZSR_DISPATCH_MODEL_(4, model, MPM_CACHED_STRESS, CALL) } \
    else { ZSR_DISPATCH_MODEL_(8, model, MPM_CACHED_STRESS, CALL) }         \
  } while (0)
// G2P: third argument = stress model to evaluate at the end (-1: none)
#define ZSR_DISPATCH_SIDE_SMODEL(side, smodel, CALL)                        \
  do {                                                                      \
    if ((side) == 4) { ZSR_DISPATCH_MODEL_(4, smodel, -1, CALL) }           \
    else { ZSR_DISPATCH_MODEL_(8, smodel, -1, CALL) }                       \
  } while (0)

}  // namespace zsr
