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
//   mollifier  EE only (barrier_ee_frame / _mollifier).  u, v the edge vectors, n = u x v, c = |n|^2, eps = 1e-2 restLen2_i restLen2_j:
//              m(c) = (2 - c / eps)(c / eps) for c < eps, else 1;  m'(c) = (2 / eps)(1 - c / eps) for c < eps, else 0;
//              dc/du = 2 (v x n), dc/dv = 2 (n x u), so grad c = (-dc/du, +dc/du, -dc/dv, +dc/dv) on (a0, a1, b0, b1).
//              energy = m b, gradient = m' b grad c + m b' grad d2.  Exactly parallel edges: c = 0, n = 0, m = 0: exactly zero.
//              eps = 0 (unmollified, or an edge of zero rest length; also an eps below the smallest normal float): m = 1.
//   zero       d2 == 0 (or d2 / dHat2 underflowing to 0, or a b' beyond the float range): energy +inf, no gradient, status BARRIER_ZERO for the
//              caller to count.  Nothing else divides by d2 and 2 / eps is finite, so no NaN reaches the gradient from finite coordinates.
//   hessian    matrix-free: barrier_pt_hvp / barrier_ee_hvp return (H_pair x) on the four corners for a direction x, never the 12 x 12 block.
//              d2 = min over lambda of |r(x, lambda)|^2, r = sum_k w_k(lambda) x_k.  The envelope argument one order up: a clamped parameter
//              is a constant, a free one solves df/dlambda_j = 0, and differentiating that condition gives dlambda/dx = -A^-1 F:
//                  (hess d2 . v)_k = 2 w_k (W v) - (F^T A^-1 F v)_k,   W v = sum_k w_k v_k
//                  r_j = dr/dlambda_j = sum_k (dw_k/dlambda_j) x_k                    (an edge vector up to sign)
//                  A_ij = 2 r_i . r_j,   (F v)_j = 2 (r_j . (W v) + r . sum_k (dw_k/dlambda_j) v_k)
//                  (F^T y)_k = 2 sum_j y_j (w_k r_j + (dw_k/dlambda_j) r)
//              The free parameters follow from the feature tri_closest / ee_closest return: the face has two (bary1, bary2), an edge
//              region one, a vertex region none; an edge pair one per side that is EE_INTERIOR.  No per-feature formulas: the feature
//              only selects the rows dw/dlambda.  With two free parameters det A = 4 |r_1 x r_2|^2 is taken from the cross product, not
//              from |r_1|^2 |r_2|^2 - (r_1 . r_2)^2, which cancels in float32.  A degenerate free system (det A, or the single A_11, not
//              above zero) falls back to the clamped form: the term F^T A^-1 F is dropped.
//              barrier: with g = grad d2:  H_b v = b'' (g . v) g + b' (hess d2 . v),
//                  b''(d2) = kappa (-2 log(d2 / dHat2) - 4 t / d2 + t^2 / d2^2)
//              mollified EE, E = m(c) b(d2):  H v = m H_b v + m' b' ((grad c . v) g + (g . v) grad c) + b (m'' (grad c . v) grad c + m' (hess c . v)),
//                  m'' = -2 / eps^2 for c < eps, else 0;  dn = du x v + u x dv, du = v_1 - v_0, dv = v_3 - v_2;
//                  (hess c . v) = 2 (dv x n + v x dn) on the u side, 2 (dn x u + n x du) on the v side, signs (-, +, -, +) as for grad c.
//              Exactly parallel edges: m = 0 and grad c = 0, what is left is b m' hess c . v, which does not depend on (s, t).
//   psd        PSD = true: every indefinite term is discarded analytically, no eigen-decomposition:
//                  H+_b v = b'' (g . v) g + |b'| F^T A^-1 F v          (b'' > 0, b' < 0 on (0, dHat2), A positive definite)
//                  H+ v   = m H+_b v + b m' 2 J^T J v,  J = dn/dx:  2 v x dn on the u side, 2 dn x u on the v side
//              positive semi-definite by construction, and without the mollifier H+ - H = 2 |b'| W^T W: H+ majorises H.  This is not the
//              eigenvalue projection of the 12 x 12 block.
//   zero (hvp) as for the gradient; also a b'' or a product beyond the float range: status BARRIER_ZERO, the pair contributes exactly zero.
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

__host__ __device__ __forceinline__ float barrier_dot(const float (&a)[3], const float (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__host__ __device__ __forceinline__ void barrier_cross(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ __forceinline__ void barrier_zero(float (&g)[4][3]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k][0] = g[k][1] = g[k][2] = 0.f;
}

// what the gradient and the product of an edge pair share, so that both see the same bits, in two steps (the product runs
// barrier_hvp_core between them, which keeps its registers down): the edge vectors u, v, the weights w and r = P - Q ...
struct BarrierEEFrame {
  float u[3], v[3], w[4], r[3], n[3], c, m = 1.f, mp = 0.f;  // m, m' where c is not below the threshold eps (on)
  bool on;
};
__host__ __device__ __forceinline__ BarrierEEFrame barrier_ee_frame(const EdgeClosest &cl, const float (&a0)[3], const float (&a1)[3],
                                                                    const float (&b0)[3], const float (&b1)[3]) {
  BarrierEEFrame f = {{a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]}, {b1[0] - b0[0], b1[1] - b0[1], b1[2] - b0[2]},
                      {1.f - cl.s, cl.s, -(1.f - cl.t), -cl.t}};
#pragma unroll
  for (int d = 0; d < 3; ++d) f.r[d] = (a0[d] + cl.s * f.u[d]) - (b0[d] + cl.t * f.v[d]);
  return f;
}
// ... and n = u x v, c = |n|^2 and the mollifier m(c), m'(c)
__host__ __device__ __forceinline__ void barrier_ee_mollifier(BarrierEEFrame &f, float eps) {
  barrier_cross(f.u, f.v, f.n);
  f.c = barrier_dot(f.n, f.n);
  f.on = eps >= FLT_MIN && f.c < eps;
  if (!f.on) return;
  const float x = f.c / eps;
  f.m = (2.f - x) * x;
  f.mp = (2.f / eps) * (1.f - x);
}

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
  if constexpr (GRAD) barrier_zero(g);
  if (status != BARRIER_ACTIVE) return status;
  BarrierEEFrame f = barrier_ee_frame(r, a0, a1, b0, b1);
  barrier_ee_mollifier(f, eps);
  energy = f.m * bb;
  if constexpr (GRAD) {
    const float A = f.m * (2.f * bp), B = f.mp * bb;
    float vn[3], nu[3];
    barrier_cross(f.v, f.n, vn);
    barrier_cross(f.n, f.u, nu);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float dcu = 2.f * vn[d], dcv = 2.f * nu[d];
      g[0][d] = B * -dcu + (A * f.w[0]) * f.r[d];
      g[1][d] = B * dcu + (A * f.w[1]) * f.r[d];
      g[2][d] = B * -dcv + (A * f.w[2]) * f.r[d];
      g[3][d] = B * dcv + (A * f.w[3]) * f.r[d];
    }
  }
  return status;
}

// b, b' and b'' at d2: barrier_eval, and ZERO as well when b'' leaves the float range (then b = +inf, b' = b'' = 0)
__host__ __device__ __forceinline__ int barrier_eval2(float d2, float dHat2, float kappa, float &b, float &bp, float &bpp) {
  bpp = 0.f;
  const int status = barrier_eval(d2, dHat2, kappa, b, bp);
  if (status != BARRIER_ACTIVE) return status;
  const float t = d2 - dHat2, lg = logf(d2 / dHat2), q = t / d2;
  const float dd = kappa * ((-2.f * lg - 4.f * q) + q * q);
  if (!(fabsf(dd) <= FLT_MAX)) {
    b = INFINITY;
    bp = 0.f;
    return BARRIER_ZERO;
  }
  bpp = dd;
  return status;
}

// H_b x (PSD: H+_b x) on the four corners from the weights w, r = P - Q and up to two free parameters: f1 / f2 say whether slot 1 / 2 is
// free, d1 / d2 are its rows dw/dlambda, r1 / r2 its vectors dr/dlambda (all zero for a slot that is not free).  Returns g . x.
template <bool PSD>
__host__ __device__ __forceinline__ float barrier_hvp_core(const float (&w)[4], const float (&r)[3], bool f1, bool f2, const float (&d1)[4],
                                                           const float (&d2)[4], const float (&r1)[3], const float (&r2)[3],
                                                           const float (&x)[4][3], float bp, float bpp, float (&h)[4][3]) {
  float Wx[3], D1[3], D2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    Wx[d] = w[0] * x[0][d] + w[1] * x[1][d] + w[2] * x[2][d] + w[3] * x[3][d];
    D1[d] = d1[0] * x[0][d] + d1[1] * x[1][d] + d1[2] * x[2][d] + d1[3] * x[3][d];
    D2[d] = d2[0] * x[0][d] + d2[1] * x[1][d] + d2[2] * x[2][d] + d2[3] * x[3][d];
  }
  const float gx = 2.f * barrier_dot(r, Wx);
  const float F1 = 2.f * (barrier_dot(r1, Wx) + barrier_dot(r, D1)), F2 = 2.f * (barrier_dot(r2, Wx) + barrier_dot(r, D2));
  const float A11 = 2.f * barrier_dot(r1, r1), A22 = 2.f * barrier_dot(r2, r2), A12 = 2.f * barrier_dot(r1, r2);
  float y1 = 0.f, y2 = 0.f;
  if (f1 && f2) {
    float c12[3];
    barrier_cross(r1, r2, c12);
    const float det = 4.f * barrier_dot(c12, c12);
    if (det > 0.f) {
      y1 = (A22 * F1 - A12 * F2) / det;
      y2 = (A11 * F2 - A12 * F1) / det;
    }
  } else if (f1) {
    if (A11 > 0.f) y1 = F1 / A11;
  } else if (f2) {
    if (A22 > 0.f) y2 = F2 / A22;
  }
  const float cg = bpp * gx, abp = fabsf(bp);
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float gk = (2.f * w[k]) * r[d];
      const float ft = 2.f * (y1 * (w[k] * r1[d] + d1[k] * r[d]) + y2 * (w[k] * r2[d] + d2[k] * r[d]));
      h[k][d] = PSD ? cg * gk + abp * ft : cg * gk + bp * ((2.f * w[k]) * Wx[d] - ft);
    }
  return gx;
}

// a product beyond the float range (or a NaN out of inf - inf on the way): the pair counts as ZERO and contributes nothing
__host__ __device__ __forceinline__ int barrier_hvp_finish(float (&h)[4][3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) ok = ok && fabsf(h[k][d]) <= FLT_MAX;
  if (!ok) barrier_zero(h);
  return ok ? BARRIER_ACTIVE : BARRIER_ZERO;
}

// h[k] = (H x)_k on (p, a, b, c) of a point-triangle pair for the direction x[k] at those vertices; PSD: the H+ of the header; returns BARRIER_*
template <bool PSD>
__host__ __device__ __forceinline__ int barrier_pt_hvp(const float (&p)[3], const float (&a)[3], const float (&b)[3], const float (&c)[3],
                                                       const float (&x)[4][3], float dHat2, float kappa, float (&h)[4][3]) {
  const TriClosest cl = tri_closest(p, a, b, c);
  float bb, bp, bpp;
  const int status = barrier_eval2(cl.dist2, dHat2, kappa, bb, bp, bpp);
  barrier_zero(h);
  if (status != BARRIER_ACTIVE) return status;
  const int ft = cl.feature;
  const bool face = ft == TRI_FACE, eab = ft == TRI_EDGE_AB, ebc = ft == TRI_EDGE_BC, eca = ft == TRI_EDGE_CA;
  // slot 1: bary1 of the face or the parameter of the edge region, slot 2: bary2 of the face
  const float d1[4] = {0.f, (face || eab) ? 1.f : (eca ? -1.f : 0.f), (face || eab) ? -1.f : (ebc ? 1.f : 0.f), ebc ? -1.f : (eca ? 1.f : 0.f)};
  const float d2[4] = {0.f, face ? 1.f : 0.f, 0.f, face ? -1.f : 0.f};
  const float w[4] = {1.f, -cl.bary[0], -cl.bary[1], -cl.bary[2]};
  float r[3], r1[3], r2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    r[d] = p[d] - cl.cp[d];
    r1[d] = (face || eab) ? a[d] - b[d] : (ebc ? b[d] - c[d] : (eca ? c[d] - a[d] : 0.f));
    r2[d] = face ? a[d] - c[d] : 0.f;
  }
  barrier_hvp_core<PSD>(w, r, face || eab || ebc || eca, face, d1, d2, r1, r2, x, bp, bpp, h);
  return barrier_hvp_finish(h);
}

// the same on (a0, a1, b0, b1) of an edge-edge pair; eps: barrier_ee_eps, 0 = unmollified
template <bool PSD>
__host__ __device__ __forceinline__ int barrier_ee_hvp(const float (&a0)[3], const float (&a1)[3], const float (&b0)[3], const float (&b1)[3],
                                                       const float (&x)[4][3], float dHat2, float kappa, float eps, float (&h)[4][3]) {
  const EdgeClosest cl = ee_closest(a0, a1, b0, b1);
  float bb, bp, bpp;
  const int status = barrier_eval2(cl.dist2, dHat2, kappa, bb, bp, bpp);
  barrier_zero(h);
  if (status != BARRIER_ACTIVE) return status;
  const bool fs = cl.category / 3 == EE_INTERIOR, ft = cl.category % 3 == EE_INTERIOR;
  BarrierEEFrame f = barrier_ee_frame(cl, a0, a1, b0, b1);
  const float d1[4] = {fs ? -1.f : 0.f, fs ? 1.f : 0.f, 0.f, 0.f}, d2[4] = {0.f, 0.f, ft ? 1.f : 0.f, ft ? -1.f : 0.f};
  float r1[3], r2[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    r1[d] = fs ? f.u[d] : 0.f;
    r2[d] = ft ? b0[d] - b1[d] : 0.f;
  }
  float hb[4][3];
  const float gx = barrier_hvp_core<PSD>(f.w, f.r, fs, ft, d1, d2, r1, r2, x, bp, bpp, hb);
  barrier_ee_mollifier(f, eps);
  const float du[3] = {x[1][0] - x[0][0], x[1][1] - x[0][1], x[1][2] - x[0][2]}, dv[3] = {x[3][0] - x[2][0], x[3][1] - x[2][1], x[3][2] - x[2][2]};
  float duv[3], udv[3], dn[3], vdn[3], dnu[3];
  barrier_cross(du, f.v, duv);
  barrier_cross(f.u, dv, udv);
#pragma unroll
  for (int d = 0; d < 3; ++d) dn[d] = duv[d] + udv[d];
  barrier_cross(f.v, dn, vdn);
  barrier_cross(dn, f.u, dnu);
  const float c3 = bb * f.mp;
  if constexpr (PSD) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float tu = c3 * (2.f * vdn[d]), tv = c3 * (2.f * dnu[d]);
      h[0][d] = f.m * hb[0][d] - tu;
      h[1][d] = f.m * hb[1][d] + tu;
      h[2][d] = f.m * hb[2][d] - tv;
      h[3][d] = f.m * hb[3][d] + tv;
    }
  } else {
    float vn[3], nu[3], dvn[3], ndu[3];
    barrier_cross(f.v, f.n, vn);
    barrier_cross(f.n, f.u, nu);
    barrier_cross(dv, f.n, dvn);
    barrier_cross(f.n, du, ndu);
    const float dcu[3] = {2.f * vn[0], 2.f * vn[1], 2.f * vn[2]}, dcv[3] = {2.f * nu[0], 2.f * nu[1], 2.f * nu[2]};
    const float gcx = barrier_dot(dcu, du) + barrier_dot(dcv, dv);
    const float c1 = f.mp * bp, c2 = f.on ? bb * ((-2.f * (gcx / eps)) / eps) : 0.f;  // c2 = b m'' (grad c . x)
    const float c1c = c1 * gcx, c1g = c1 * gx;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float tu = c1g * dcu[d] + (c2 * dcu[d] + c3 * (2.f * (dvn[d] + vdn[d])));
      const float tv = c1g * dcv[d] + (c2 * dcv[d] + c3 * (2.f * (dnu[d] + ndu[d])));
      h[0][d] = (f.m * hb[0][d] + c1c * ((2.f * f.w[0]) * f.r[d])) - tu;
      h[1][d] = (f.m * hb[1][d] + c1c * ((2.f * f.w[1]) * f.r[d])) + tu;
      h[2][d] = (f.m * hb[2][d] + c1c * ((2.f * f.w[2]) * f.r[d])) - tv;
      h[3][d] = (f.m * hb[3][d] + c1c * ((2.f * f.w[3]) * f.r[d])) + tv;
    }
  }
  return barrier_hvp_finish(h);
}

}  // namespace zsr
