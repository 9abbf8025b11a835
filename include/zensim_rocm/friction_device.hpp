// friction_device.hpp -- lagged IPC friction (Li et al. 2020) of one point-triangle or edge-edge pair: the job of the smoothed static-friction
// functions f0_SF / f1_SF_div_rel_dx_norm / f2_SF_term and of the per-feature tangent bases and relative displacements of
// geometry/Friction.hpp, written from the math on top of tri_closest / ee_closest and barrier_eval.
//
//   lag       at the positions the normal forces are frozen at, one record of 8 floats per pair: n[3], lambda, w[4].
//             r = P - Q, d2 and the parameters are the barrier's own (tri_closest / ee_closest, barrier_ee_frame): w = (1, -bary) for PT,
//             (1 - s, s, -(1 - t), -t) for EE, the weights of the barrier gradient, which sum to zero.  d = sqrt(d2), n = r / d,
//             lambda = m (-b'(d2)) 2 d: the size of the contact force, b' from barrier_eval, m the edge-edge mollifier (1 for PT and
//             where the pair is not mollified).  Inactive (d2 >= dHat2): an all-zero record.  Zero distance, or a lambda or n beyond
//             the float range: an all-zero record and status BARRIER_ZERO for the caller to count.  Exactly parallel mollified edges:
//             m = 0, lambda = 0.
//   tangent   no per-feature 3 x 2 basis.  Every basis of the reference (point_point_ / point_edge_ / point_triangle_ /
//             edge_edge_tangent_basis) spans the plane across P - Q on the feature it belongs to, and energy, gradient and product
//             depend on the relative displacement ur = sum_k w_k u_k only through |T^T ur| = |(I - n n^T) ur|: the projector I - n n^T
//             gives the same numbers on every feature.
//   evaluate  at a displacement u (x - x at the start of the step) of the four corners, with mu and the threshold eps_v in displacement
//             units; from the record alone, no positions and no distance code:
//                 ur = sum_k w_k u_k,   ut = ur - (n . ur) n,   y = |ut|
//                 energy    mu lambda f0(y),       f0 = y for y >= eps_v, else y^2 (eps_v - y / 3) / eps_v^2 + eps_v / 3
//                 gradient  mu lambda c1 w_k ut,   c1 = f0' / y = 1 / y for y >= eps_v, else (2 eps_v - y) / eps_v^2
//                 product   z = sum_k w_k x_k, zt = z - (n . z) n:  (H x)_k = mu lambda w_k (c1 zt + c2 (ut . zt) ut),
//                           c2 = c1' / y = -1 / y^3 for y >= eps_v, else -1 / (eps_v^2 y); the c2 term is exactly zero at y = 0.
//             This is the derivative of the energy.  (The comment on the reference's f2_SF_term claims the constant -1 / eps_v^2 on both
//             branches; the derivative of c1 ut is what is written here.)  H is positive semi-definite by construction: along ut its
//             eigenvalue is c1 + c2 y^2 = 2 (eps_v - y) / eps_v^2 below the threshold and 0 above, across ut it is c1 > 0.
//   overflow  a y^2 (for the product: a y^3), an energy or a term beyond the float range: the pair contributes exactly zero and the
//             function returns BARRIER_ZERO for the caller to count.  No NaN comes from finite inputs.  A record with mu lambda = 0 (an
//             idle pair, mu = 0) contributes exactly zero and is BARRIER_INACTIVE.
// Float32 throughout.  Translation units that use this are built with -ffp-contract=off, as for barrier_device.hpp: the evaluation has only
// + - * / and sqrt, so a float32 chain in numpy reproduces it bit for bit.
#pragma once
#include "barrier_device.hpp"

namespace zsr {

// n[3], lambda, w[4]: 32 bytes, read and written as two float4
struct FrictionRecord {
  float n[3], lambda, w[4];
};

__host__ __device__ __forceinline__ FrictionRecord friction_record_zero() { return FrictionRecord{{0.f, 0.f, 0.f}, 0.f, {0.f, 0.f, 0.f, 0.f}}; }

// the record from r = P - Q, d2, the weights, b' and the mollifier m; ACTIVE, or ZERO with an all-zero record
__host__ __device__ __forceinline__ int friction_lag_finish(const float (&r)[3], float d2, const float (&w)[4], float bp, float m, FrictionRecord &rec) {
  const float d = sqrtf(d2);
  rec.lambda = (m * -bp) * (2.f * d);
  bool ok = fabsf(rec.lambda) <= FLT_MAX;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    rec.n[k] = r[k] / d;
    ok = ok && fabsf(rec.n[k]) <= FLT_MAX;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) rec.w[k] = w[k];
  if (ok) return BARRIER_ACTIVE;
  rec = friction_record_zero();
  return BARRIER_ZERO;
}

// the record of a point-triangle pair (p, a, b, c); returns BARRIER_*
__host__ __device__ __forceinline__ int friction_lag_pt(const float (&p)[3], const float (&a)[3], const float (&b)[3], const float (&c)[3], float dHat2,
                                                        float kappa, FrictionRecord &rec) {
  const TriClosest cl = tri_closest(p, a, b, c);
  float bb, bp;
  const int status = barrier_eval(cl.dist2, dHat2, kappa, bb, bp);
  rec = friction_record_zero();
  if (status != BARRIER_ACTIVE) return status;
  const float w[4] = {1.f, -cl.bary[0], -cl.bary[1], -cl.bary[2]};
  const float r[3] = {p[0] - cl.cp[0], p[1] - cl.cp[1], p[2] - cl.cp[2]};
  return friction_lag_finish(r, cl.dist2, w, bp, 1.f, rec);
}

// the record of an edge-edge pair (a0, a1, b0, b1); eps: barrier_ee_eps, 0 = unmollified; returns BARRIER_*
__host__ __device__ __forceinline__ int friction_lag_ee(const float (&a0)[3], const float (&a1)[3], const float (&b0)[3], const float (&b1)[3],
                                                        float dHat2, float kappa, float eps, FrictionRecord &rec) {
  const EdgeClosest cl = ee_closest(a0, a1, b0, b1);
  float bb, bp;
  const int status = barrier_eval(cl.dist2, dHat2, kappa, bb, bp);
  rec = friction_record_zero();
  if (status != BARRIER_ACTIVE) return status;
  BarrierEEFrame f = barrier_ee_frame(cl, a0, a1, b0, b1);
  barrier_ee_mollifier(f, eps);
  return friction_lag_finish(f.r, cl.dist2, f.w, bp, f.m, rec);
}

// what the three evaluations share: the tangential relative displacement ut of the rows u and its length
struct FrictionSlip {
  float ut[3], y2, y;
};
// (I - n n^T) sum_k w_k x_k
__host__ __device__ __forceinline__ void friction_tangent(const FrictionRecord &rec, const float (&x)[4][3], float (&t)[3]) {
  float z[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) z[d] = rec.w[0] * x[0][d] + rec.w[1] * x[1][d] + rec.w[2] * x[2][d] + rec.w[3] * x[3][d];
  const float nz = barrier_dot(rec.n, z);
#pragma unroll
  for (int d = 0; d < 3; ++d) t[d] = z[d] - nz * rec.n[d];
}
__host__ __device__ __forceinline__ FrictionSlip friction_slip(const FrictionRecord &rec, const float (&u)[4][3]) {
  FrictionSlip s;
  friction_tangent(rec, u, s.ut);
  s.y2 = barrier_dot(s.ut, s.ut);
  s.y = sqrtf(s.y2);
  return s;
}
// c1 = f0'(y) / y
__host__ __device__ __forceinline__ float friction_c1(float y, float epsv) { return y >= epsv ? 1.f / y : (2.f * epsv - y) / (epsv * epsv); }

// energy mu lambda f0(y) of a pair from its record and the rows u of its corners; returns BARRIER_* (ZERO: overflow, energy 0)
__host__ __device__ __forceinline__ int friction_energy(const FrictionRecord &rec, const float (&u)[4][3], float mu, float epsv, float &energy) {
  energy = 0.f;
  const float scale = mu * rec.lambda;
  if (scale == 0.f) return BARRIER_INACTIVE;
  const FrictionSlip s = friction_slip(rec, u);
  if (!(s.y2 <= FLT_MAX)) return BARRIER_ZERO;
  const float f0 = s.y >= epsv ? s.y : (s.y2 * (epsv - s.y / 3.f)) / (epsv * epsv) + epsv / 3.f;
  const float e = scale * f0;
  if (!(fabsf(e) <= FLT_MAX)) return BARRIER_ZERO;
  energy = e;
  return BARRIER_ACTIVE;
}

// energy and gradient g[k] = mu lambda c1 w_k ut on the four corners; returns BARRIER_* (ZERO: overflow, energy and gradient 0)
__host__ __device__ __forceinline__ int friction_gradient(const FrictionRecord &rec, const float (&u)[4][3], float mu, float epsv, float &energy,
                                                          float (&g)[4][3]) {
  barrier_zero(g);
  const int status = friction_energy(rec, u, mu, epsv, energy);
  if (status != BARRIER_ACTIVE) return status;
  const FrictionSlip s = friction_slip(rec, u);
  const float a = (mu * rec.lambda) * friction_c1(s.y, epsv);
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) g[k][d] = (a * rec.w[k]) * s.ut[d];
  if (barrier_hvp_finish(g) == BARRIER_ACTIVE) return BARRIER_ACTIVE;
  energy = 0.f;
  return BARRIER_ZERO;
}

// h[k] = (H x)_k on the four corners for the direction x[k] at those vertices; returns BARRIER_* (ZERO: overflow, h = 0)
__host__ __device__ __forceinline__ int friction_product(const FrictionRecord &rec, const float (&u)[4][3], const float (&x)[4][3], float mu, float epsv,
                                                         float (&h)[4][3]) {
  barrier_zero(h);
  const float scale = mu * rec.lambda;
  if (scale == 0.f) return BARRIER_INACTIVE;
  const FrictionSlip s = friction_slip(rec, u);
  const float y3 = s.y2 * s.y;
  if (!(y3 <= FLT_MAX)) return BARRIER_ZERO;
  float zt[3];
  friction_tangent(rec, x, zt);
  const float c1 = friction_c1(s.y, epsv);
  const float c2 = s.y > 0.f ? (s.y >= epsv ? -1.f / y3 : -1.f / ((epsv * epsv) * s.y)) : 0.f;
  const float q = s.y > 0.f ? c2 * barrier_dot(s.ut, zt) : 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) h[k][d] = (scale * rec.w[k]) * (c1 * zt[d] + q * s.ut[d]);
  return barrier_hvp_finish(h);
}

}  // namespace zsr
