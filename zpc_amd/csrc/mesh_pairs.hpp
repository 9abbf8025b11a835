// mesh_pairs.hpp -- what the kernels over a proximity list share between mesh_barrier.hip (barrier and friction: energy, gradient, product)
// and mesh_solve.hip (their diagonal blocks and the fused operator): the operations, the argument block of a pair kernel, the corners of a
// pair, the friction record's loads and stores, and the launchers of mesh_barrier.hip that another translation unit may call inside its
// own Launch.
#pragma once
#include "mesh.hpp"
#include "../../include/zensim_rocm/barrier_device.hpp"
#include "../../include/zensim_rocm/friction_device.hpp"

namespace zsr {

enum {
  BARRIER_OP_ENERGY,
  BARRIER_OP_GRADIENT,
  BARRIER_OP_PRODUCT,
  BARRIER_OP_PRODUCT_PSD,
  BARRIER_OP_LAG,                // friction: the lagged record at verts
  BARRIER_OP_FRICTION_ENERGY,    // friction at the displacement verts, from the record
  BARRIER_OP_FRICTION_GRADIENT,
  BARRIER_OP_FRICTION_PRODUCT
};

// the friction record of pair i: 32-byte records in a 256-byte aligned array, as two float4
__device__ __forceinline__ void friction_store(float *record, size_t pair, const FrictionRecord &r) {
  float4 *o = reinterpret_cast<float4 *>(record + 8 * pair);
  o[0] = make_float4(r.n[0], r.n[1], r.n[2], r.lambda);
  o[1] = make_float4(r.w[0], r.w[1], r.w[2], r.w[3]);
}
__device__ __forceinline__ FrictionRecord friction_load(const float *record, size_t pair) {
  const float4 *in = reinterpret_cast<const float4 *>(record + 8 * pair);
  const float4 a = in[0], b = in[1];
  return FrictionRecord{{a.x, a.y, a.z}, a.w, {b.x, b.y, b.z, b.w}};
}

// one pair list of one kind and what the pair kernel reads and writes for it
struct BarrierPairs {
  const float *verts;  // [nv][3] positions; a friction evaluation: the displacement u
  const int *prims;    // the kind's primitives: tris [np][3] (PT) or edges [np][2] (EE)
  int nv, np;
  const float *rest;  // EE: the squared rest lengths [np]; null: unmollified
  const int *pairs;   // [n][2]: (vertex, triangle) or (edge, edge)
  int n;
  float dHat2, kappa;
  const float *dir;         // [nv][3], a product only
  float *energy, *contrib;  // [n] (energy, gradient) and the [n][4][3] records (all but energy); a block kernel: the [n][4][6] blocks
  int *status;              // [2] zero-distance (a friction evaluation: overflow) counts, PT then EE
  float *record;            // friction: the [n][8] records, written by the lag step and read by the evaluations
  float mu, epsv;           // a friction evaluation: the coefficient and the static-friction threshold
};

// the four corner vertices of pair i (pair_corners of mesh.hpp; false: the pair is inactive) and the mollifier threshold (0: none)
template <bool EE>
__device__ __forceinline__ bool barrier_corners(const BarrierPairs &a, int i, int (&idx)[4], float &eps) {
  eps = 0.f;
  if (!pair_corners<EE>(a.pairs, a.prims, a.nv, a.np, i, idx)) return false;
  if constexpr (EE)
    if (a.rest) eps = barrier_ee_eps(a.rest[a.pairs[2 * (size_t)i]], a.rest[a.pairs[2 * (size_t)i + 1]]);
  return true;
}

// what the friction operations add to a launch: the [npt + nee][8] records (PT pairs first), mu and the threshold
struct FrictionArgs {
  float *record;
  float mu, epsv;
};

// ---- mesh_barrier.hip
// the checks the barrier entries (the friction evaluations) have in common
bool barrier_args_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, const int *ptPairs, size_t npt, const int *eePairs, size_t nee, float dHat,
                     float kappa, int mollify);
bool friction_args_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *u, const int *ptPairs, size_t npt, const int *eePairs,
                      size_t nee, const float *record, float mu, float epsv);
// the argument blocks of one operation over the PT and the EE list, the EE list's scratch (stride floats per pair) and records behind the
// PT list's; status: two zeroed counts
void barrier_pair_args(const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs, size_t nee, float dHat,
                       float kappa, int mollify, const float *dir, float *ptEnergy, float *eeEnergy, float *scratch, size_t stride, int *status,
                       const FrictionArgs &fr, BarrierPairs &pt, BarrierPairs &ee);
// the pair kernels of one operation (BARRIER_OP_*) on such blocks: the PT list, then the EE list
void barrier_launch_args(Launch &L, int op, const BarrierPairs &pt, const BarrierPairs &ee);
// both, with the status words (the caller's or a temporary) zeroed first
void barrier_launch_pairs(Launch &L, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs, size_t nee,
                          float dHat, float kappa, int mollify, int op, const float *dir, float *ptEnergy, float *eeEnergy, float *scratch,
                          int *status, const FrictionArgs &fr);

}  // namespace zsr
