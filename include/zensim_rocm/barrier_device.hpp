// barrier_device.hpp -- the IPC contact potential of one point-triangle or edge-edge pair, energy and gradient with respect to its four
// vertices: the job of barrier / barrier_gradient (geometry/SpatialQuery.hpp:502-531), dist_grad_pt / _pe / _pp / _ee and mollifier_ee /
// mollifier_grad_ee / mollifier_threshold_ee (geometry/Distance.hpp), written from the geometry on top of tri_closest / ee_closest.
//
//   barrier    with t = d2 - dHat2:  b(d2) = -kappa t^2 log(d2 / dHat2) for d2 < dHat2, else 0 (the unnormalised form);
//              b'(d2) = kappa (-2 t log(d2 / dHat2) - t^2 / d2).
//   grad d2    No per-feature formulas.  d2 is the minimum of f(x, lambda) = |P(x, lambda) - Q(x, lambda)|^2 over the parameters lambda of
//              the closest points (barycentrics of the triangle, s and t of the edges), x the 12 coordinates.  On the feature the minimum
//              is realised on, every parameter is either free -- then df/dlambda = 0 there -- or clamped to a constant of its range --
//              then dlambda/dx = 0.  Either way the parameters contribute nothing to the total derivative (the envelope theorem), and what
//              is left is the partial derivative at fixed parameters: P - Q is linear in the vertices with weights w_k, so
//                  d(d2)/d(x_k) = 2 w_k (P - Q)
//              PT: w = (1, -bary0, -bary1, -bary2), P the point, Q the closest point of the triangle;
//              EE: w = (1 - s, s, -(1 - t), -t), P and Q the closest points on edge i and edge j.
//              With the parameters of a vertex / an edge / the face substituted this is g_PP / g_PE / g_PT / g_EE wherever those are
//              defined; where two features tie the distance has no gradient and this is one of its one-sided limits.  No case split.
//   mollifier  EE only.  u, v the edge vectors, n = u x v, c = |n|^2, eps = 1e-2 restLen2_i restLen2_j:
//              m(c) = (2 - c / eps)(c / eps) for c < eps, else 1;  m'(c) = (2 / eps)(1 - c / eps) for c < eps, else 0;
//              dc/du = 2 (v x n), dc/dv = 2 (n x u), so grad c = (-dc/du, +dc/du, -dc/dv, +dc/dv) on (a0, a1, b0, b1).
//              energy = m b, gradient = m' b grad c + m b' grad d2.  Exactly parallel edges: c = 0, n = 0, m = 0: exactly zero.
//              eps = 0 (unmollified, or an edge of zero rest length; also an eps below the smallest normal float): m = 1.
//   zero       d2 == 0 (or d2 / dHat2 underflowing to 0, or a b' beyond the float range): energy +inf, no gradient, status BARRIER_ZERO for the
//              caller to count.  Nothing else divides by d2 and 2 / eps is finite, so no NaN reaches the gradient from finite coordinates.
// Float32 throughout; the logarithm is the platform's logf.  Translation units that use this are built with -ffp-contract=off, as for
// distance_device.hpp: a float32 chain in numpy then reproduces it operation by operation.
#pragma once
#include <cfloat>
#include <cmath>

#include "distance_device.hpp"

namespace zsr {

enum { BARRIER_INACTIVE = 0, BARRIER_ACTIVE = 1, BARRIER_ZERO = 2 };

// b and b' at d2; INACTIVE: both 0; ZERO: b = +inf, b' = 0
__host__ __device__ __forceinline__ int barrier_eval(float d2, float dHat2, float kappa, float &b, float &bp) {
  b = 0.f;
  bp = 0.f;
  if (!(d2 < dHat2)) return BARRIER_INACTIVE;
  const float ratio = d2 / dHat2;
  if (!(ratio > 0.f)) {
    b = INFINITY;
    return BARRIER_ZERO;
  }
  const float t = d2 - dHat2, lg = logf(ratio), t2 = t * t;
  const float e = (-kappa * t2) * lg, de = kappa * ((-2.f * t) * lg - t2 / d2);
  if (!(fabsf(de) <= FLT_MAX)) {
    b = INFINITY;
    return BARRIER_ZERO;
  }
  b = e;
  bp = de;
  return BARRIER_ACTIVE;
}

// the mollifier threshold of an edge pair from the squared rest lengths
__host__ __device__ __forceinline__ float barrier_ee_eps(float restLen2I, float restLen2J) { return (1e-2f * restLen2I) * restLen2J; }

// energy and (GRAD) gradient g[k] on (p, a, b, c) of a point-triangle pair; returns BARRIER_*
template <bool GRAD>
__host__ __device__ __forceinline__ int barrier_pt(const float (&p)[3], const float (&a)[3], const float (&b)[3], const float (&c)[3], float dHat2,
                                                   float kappa, float &energy, float (&g)[4][3]) {
  const TriClosest r = tri_closest(p, a, b, c);
  float bb, bp;
  const int status = barrier_eval(r.dist2, dHat2, kappa, bb, bp);
  energy = bb;
  if constexpr (GRAD) {
    const float w[4] = {1.f, -r.bary[0], -r.bary[1], -r.bary[2]};
    const float A = 2.f * bp;  // 0 unless ACTIVE
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int d = 0; d < 3; ++d) g[k][d] = status == BARRIER_ACTIVE ? (A * w[k]) * (p[d] - r.cp[d]) : 0.f;
  }
  return status;
}

// energy and (GRAD) gradient g[k] on (a0, a1, b0, b1) of an edge-edge pair; eps: barrier_ee_eps, 0 = unmollified; returns BARRIER_*
template <bool GRAD>
__host__ __device__ __forceinline__ int barrier_ee(const float (&a0)[3], const float (&a1)[3], const float (&b0)[3], const float (&b1)[3], float dHat2,
                                                   float kappa, float eps, float &energy, float (&g)[4][3]) {
  const EdgeClosest r = ee_closest(a0, a1, b0, b1);
  float bb, bp;
  const int status = barrier_eval(r.dist2, dHat2, kappa, bb, bp);
  energy = bb;
  if constexpr (GRAD) {
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k][0] = g[k][1] = g[k][2] = 0.f;
  }
  if (status != BARRIER_ACTIVE) return status;
  const float u[3] = {a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]}, v[3] = {b1[0] - b0[0], b1[1] - b0[1], b1[2] - b0[2]};
  const float n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const float c = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  float m = 1.f, mp = 0.f;
  if (eps >= FLT_MIN && c < eps) {
    const float x = c / eps;
    m = (2.f - x) * x;
    mp = (2.f / eps) * (1.f - x);
  }
  energy = m * bb;
  if constexpr (GRAD) {
    const float w[4] = {1.f - r.s, r.s, -(1.f - r.t), -r.t};
    const float A = m * (2.f * bp), B = mp * bb;
    const float vn[3] = {v[1] * n[2] - v[2] * n[1], v[2] * n[0] - v[0] * n[2], v[0] * n[1] - v[1] * n[0]};
    const float nu[3] = {n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float diff = (a0[d] + r.s * u[d]) - (b0[d] + r.t * v[d]);
      const float dcu = 2.f * vn[d], dcv = 2.f * nu[d];
      g[0][d] = B * -dcu + (A * w[0]) * diff;
      g[1][d] = B * dcu + (A * w[1]) * diff;
      g[2][d] = B * -dcv + (A * w[2]) * diff;
      g[3][d] = B * dcv + (A * w[3]) * diff;
    }
  }
  return status;
}

}  // namespace zsr
