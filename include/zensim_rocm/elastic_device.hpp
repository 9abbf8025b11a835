// elastic_device.hpp -- the internal energy of a triangle mesh, one element at a time: the St. Venant-Kirchhoff membrane energy of a triangle
// and the quadratic (isometric) bending energy of Bergou et al. 2006 of a hinge (an edge with two incident triangles), each with its
// gradient and its matrix-free Hessian-vector product, exact or positive semi-definite.  Written from the math; the reference has no
// counterpart.
//
//   membrane  rest record of a triangle (X0, X1, X2), 4 floats (B00, B01, B11, A): e1 = X1 - X0, e2 = X2 - X0, a = |e1|, t1 = e1 / a,
//             b = e2 . t1, c = |e2 - b t1|; B = [[1 / a, -b / (a c)], [0, 1 / c]] is the inverse of the upper-triangular rest edge matrix,
//             A = a c / 2 the rest area.  a = 0, c = 0 or an entry beyond the float range: an all-zero record (ELASTIC_DEGENERATE).
//             At positions x:  F = [x1 - x0, x2 - x0] B (3 x 2),  E = (F^T F - I) / 2,  S = 2 mu E + lam tr(E) I,
//                 energy    A (mu |E|_F^2 + lam / 2 tr(E)^2);  mu, lam are per-area stiffnesses (the caller multiplies in the thickness)
//                 gradient  G = A (F S) B^T,  g1 = G[:, 0], g2 = G[:, 1], g0 = -(g1 + g2)
//                 product   with z: dF = [z1 - z0, z2 - z0] B, dE = sym(F^T dF), dS = 2 mu dE + lam tr(dE) I, dP = dF S + F dS, mapped to
//                           the corners like F S.
//             StVK has no singularity: a triangle collapsed to a point or inverted is an ordinary input.
//   psd       S in dF S is replaced by its projection S+ onto the positive semi-definite 2 x 2 matrices, in closed form:
//             m = (S00 + S11) / 2, r = sqrt(((S00 - S11) / 2)^2 + S01^2); S+ = S if m - r >= 0, 0 if m + r <= 0, else
//             (m + r) / (2 r) (S - (m - r) I).  The F dS part contributes 2 mu |dE|^2 + lam tr(dE)^2 >= 0 for mu, lam >= 0 and dF S+ is
//             positive semi-definite by construction, so H+ majorises H and equals it, bit for bit, where the triangle is not compressed.
//             No iteration and no per-thread matrix: the indefinite part is discarded analytically, as for the barrier.
//   bending   hinge (x0, x1, x2, x3): x0 < x1 the edge, x2 and x3 the opposite vertices.  Rest cotangents c01, c02 of the angles at x0 in
//             (x0, x1, x2) and (x0, x1, x3), c03, c04 of those at x1; K = (c03 + c04, c01 + c02, -c01 - c03, -c02 - c04); record, 4 floats:
//             k = sqrt(3 / (A0 + A1)) K, A0, A1 the rest areas.  A rest triangle of zero area or an entry beyond the float range: an
//             all-zero record (ELASTIC_DEGENERATE).  With w = sum_i k_i x_i:
//                 energy kb / 2 |w|^2,  gradient kb k_i w,  product kb k_i (sum_j k_j z_j): the gradient's formula at z.
//             Positive semi-definite as it stands: psd changes nothing.  DOMAIN: the energy is zero at rest only where the rest shape is
//             flat across the hinge (cloth); on a curved rest shape it penalises the rest curvature too.
//   overflow  an energy or a term beyond the float range: the element contributes exactly zero (energy and every term) and the function
//             returns ELASTIC_OVERFLOW for the caller to count.  No NaN comes from finite inputs.  An all-zero record contributes exactly
//             zero and is ELASTIC_IDLE.
// Float32 throughout.  The evaluation has only + - * / and sqrt; translation units that use this are built with -ffp-contract=off, so a
// float32 chain in numpy reproduces it bit for bit.  Sums of three products are formed left to right.
#pragma once
#include <cfloat>
#include <cmath>

#include <hip/hip_runtime.h>

namespace zsr {

enum { ELASTIC_IDLE = 0, ELASTIC_ACTIVE = 1, ELASTIC_OVERFLOW = 2, ELASTIC_DEGENERATE = 3 };
enum { ELASTIC_OP_ENERGY, ELASTIC_OP_GRADIENT, ELASTIC_OP_PRODUCT, ELASTIC_OP_PRODUCT_PSD };

__host__ __device__ __forceinline__ float elastic_dot(const float (&a)[3], const float (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__host__ __device__ __forceinline__ void elastic_cross(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ __forceinline__ bool elastic_finite(float x) { return fabsf(x) <= FLT_MAX; }

// the rest record (B00, B01, B11, A) of a triangle; ELASTIC_ACTIVE, or ELASTIC_DEGENERATE with an all-zero record
__host__ __device__ __forceinline__ int elastic_tri_rest(const float (&X0)[3], const float (&X1)[3], const float (&X2)[3], float (&rec)[4]) {
  rec[0] = rec[1] = rec[2] = rec[3] = 0.f;
  const float e1[3] = {X1[0] - X0[0], X1[1] - X0[1], X1[2] - X0[2]}, e2[3] = {X2[0] - X0[0], X2[1] - X0[1], X2[2] - X0[2]};
  const float a = sqrtf(elastic_dot(e1, e1));
  if (!(a > 0.f && a <= FLT_MAX)) return ELASTIC_DEGENERATE;
  const float t1[3] = {e1[0] / a, e1[1] / a, e1[2] / a};
  const float b = elastic_dot(e2, t1);
  const float p[3] = {e2[0] - b * t1[0], e2[1] - b * t1[1], e2[2] - b * t1[2]};
  const float c = sqrtf(elastic_dot(p, p));
  if (!(c > 0.f && c <= FLT_MAX)) return ELASTIC_DEGENERATE;
  const float ac = a * c;
  if (!(ac > 0.f)) return ELASTIC_DEGENERATE;
  const float B00 = 1.f / a, B01 = -b / ac, B11 = 1.f / c, A = 0.5f * ac;
  if (!(elastic_finite(B00) && elastic_finite(B01) && elastic_finite(B11) && elastic_finite(A) && A > 0.f)) return ELASTIC_DEGENERATE;
  rec[0] = B00, rec[1] = B01, rec[2] = B11, rec[3] = A;
  return ELASTIC_ACTIVE;
}

// the rest record k[4] of a hinge; ELASTIC_ACTIVE, or ELASTIC_DEGENERATE with an all-zero record
__host__ __device__ __forceinline__ int elastic_hinge_rest(const float (&X0)[3], const float (&X1)[3], const float (&X2)[3], const float (&X3)[3],
                                                           float (&rec)[4]) {
  rec[0] = rec[1] = rec[2] = rec[3] = 0.f;
  float e[3], a2[3], a3[3], b2[3], b3[3], n0[3], n1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e[d] = X1[d] - X0[d];
    a2[d] = X2[d] - X0[d];
    a3[d] = X3[d] - X0[d];
    b2[d] = X1[d] - X2[d];
    b3[d] = X1[d] - X3[d];
  }
  elastic_cross(e, a2, n0);
  elastic_cross(e, a3, n1);
  const float s0 = sqrtf(elastic_dot(n0, n0)), s1 = sqrtf(elastic_dot(n1, n1));  // twice the rest areas
  if (!(s0 > 0.f && s0 <= FLT_MAX && s1 > 0.f && s1 <= FLT_MAX)) return ELASTIC_DEGENERATE;
  const float c01 = elastic_dot(e, a2) / s0, c02 = elastic_dot(e, a3) / s1, c03 = elastic_dot(e, b2) / s0, c04 = elastic_dot(e, b3) / s1;
  const float q = sqrtf(3.f / (0.5f * s0 + 0.5f * s1));
  const float k[4] = {q * (c03 + c04), q * (c01 + c02), q * (-c01 - c03), q * (-c02 - c04)};
  if (!(elastic_finite(k[0]) && elastic_finite(k[1]) && elastic_finite(k[2]) && elastic_finite(k[3]))) return ELASTIC_DEGENERATE;
  rec[0] = k[0], rec[1] = k[1], rec[2] = k[2], rec[3] = k[3];
  return ELASTIC_ACTIVE;
}

// what the membrane operations share: the two columns of F and the entries of E and S
struct ElasticStrain {
  float F0[3], F1[3], E00, E01, E11, tr, S00, S01, S11;
};
// the two columns of [y1 - y0, y2 - y0] B
__host__ __device__ __forceinline__ void elastic_columns(const float (&rec)[4], const float (&y)[3][3], float (&c0)[3], float (&c1)[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float d1 = y[1][d] - y[0][d], d2 = y[2][d] - y[0][d];
    c0[d] = rec[0] * d1;
    c1[d] = rec[1] * d1 + rec[2] * d2;
  }
}
__host__ __device__ __forceinline__ ElasticStrain elastic_strain(const float (&rec)[4], const float (&x)[3][3], float mu, float lam) {
  ElasticStrain s;
  elastic_columns(rec, x, s.F0, s.F1);
  s.E00 = 0.5f * (elastic_dot(s.F0, s.F0) - 1.f);
  s.E11 = 0.5f * (elastic_dot(s.F1, s.F1) - 1.f);
  s.E01 = 0.5f * elastic_dot(s.F0, s.F1);
  s.tr = s.E00 + s.E11;
  const float mu2 = 2.f * mu, lt = lam * s.tr;
  s.S00 = mu2 * s.E00 + lt;
  s.S11 = mu2 * s.E11 + lt;
  s.S01 = mu2 * s.E01;
  return s;
}
__host__ __device__ __forceinline__ float elastic_tri_energy_of(const float (&rec)[4], const ElasticStrain &s, float mu, float lam) {
  return rec[3] * (mu * ((s.E00 * s.E00 + s.E11 * s.E11) + 2.f * (s.E01 * s.E01)) + (0.5f * lam) * (s.tr * s.tr));
}
// A (P B^T) on the corners from the columns P0, P1 of a 3 x 2 matrix: t[1] = A (P0 B00 + P1 B01), t[2] = A (P1 B11), t[0] = -(t[1] + t[2])
__host__ __device__ __forceinline__ bool elastic_corners(const float (&rec)[4], const float (&P0)[3], const float (&P1)[3], float (&t)[3][3]) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    t[1][d] = rec[3] * (P0[d] * rec[0] + P1[d] * rec[1]);
    t[2][d] = rec[3] * (P1[d] * rec[2]);
    t[0][d] = -(t[1][d] + t[2][d]);
    ok = ok && elastic_finite(t[0][d]) && elastic_finite(t[1][d]) && elastic_finite(t[2][d]);
  }
  return ok;
}
__host__ __device__ __forceinline__ void elastic_zero3(float (&t)[3][3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k][0] = t[k][1] = t[k][2] = 0.f;
}

// energy of a triangle at x; returns ELASTIC_*
__host__ __device__ __forceinline__ int elastic_tri_energy(const float (&rec)[4], const float (&x)[3][3], float mu, float lam, float &energy) {
  energy = 0.f;
  if (rec[3] == 0.f) return ELASTIC_IDLE;
  const ElasticStrain s = elastic_strain(rec, x, mu, lam);
  const float e = elastic_tri_energy_of(rec, s, mu, lam);
  if (!elastic_finite(e)) return ELASTIC_OVERFLOW;
  energy = e;
  return ELASTIC_ACTIVE;
}

// energy and gradient g[3][3] of a triangle at x; returns ELASTIC_* (OVERFLOW: energy and gradient 0)
__host__ __device__ __forceinline__ int elastic_tri_gradient(const float (&rec)[4], const float (&x)[3][3], float mu, float lam, float &energy,
                                                             float (&g)[3][3]) {
  energy = 0.f;
  elastic_zero3(g);
  if (rec[3] == 0.f) return ELASTIC_IDLE;
  const ElasticStrain s = elastic_strain(rec, x, mu, lam);
  const float e = elastic_tri_energy_of(rec, s, mu, lam);
  float P0[3], P1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    P0[d] = s.S00 * s.F0[d] + s.S01 * s.F1[d];
    P1[d] = s.S01 * s.F0[d] + s.S11 * s.F1[d];
  }
  if (elastic_corners(rec, P0, P1, g) && elastic_finite(e)) {
    energy = e;
    return ELASTIC_ACTIVE;
  }
  elastic_zero3(g);
  return ELASTIC_OVERFLOW;
}

// h[3][3] = (H z) on the corners of a triangle at x; PSD: the H+ of the header; returns ELASTIC_* (OVERFLOW: h = 0)
template <bool PSD>
__host__ __device__ __forceinline__ int elastic_tri_product(const float (&rec)[4], const float (&x)[3][3], const float (&z)[3][3], float mu, float lam,
                                                            float (&h)[3][3]) {
  elastic_zero3(h);
  if (rec[3] == 0.f) return ELASTIC_IDLE;
  const ElasticStrain s = elastic_strain(rec, x, mu, lam);
  float T00 = s.S00, T01 = s.S01, T11 = s.S11;
  if constexpr (PSD) {
    const float m = 0.5f * (s.S00 + s.S11), hd = 0.5f * (s.S00 - s.S11);
    const float r = sqrtf(hd * hd + s.S01 * s.S01);
    if (!(m - r >= 0.f)) {
      if (m + r <= 0.f) {
        T00 = T01 = T11 = 0.f;
      } else {
        const float q = (m + r) / (2.f * r), lo = m - r;
        T00 = q * (s.S00 - lo);
        T11 = q * (s.S11 - lo);
        T01 = q * s.S01;
      }
    }
  }
  float dF0[3], dF1[3];
  elastic_columns(rec, z, dF0, dF1);
  const float dE00 = elastic_dot(s.F0, dF0), dE11 = elastic_dot(s.F1, dF1);
  const float dE01 = 0.5f * (elastic_dot(s.F0, dF1) + elastic_dot(s.F1, dF0));
  const float mu2 = 2.f * mu, lt = lam * (dE00 + dE11);
  const float dS00 = mu2 * dE00 + lt, dS11 = mu2 * dE11 + lt, dS01 = mu2 * dE01;
  float P0[3], P1[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    P0[d] = (T00 * dF0[d] + T01 * dF1[d]) + (dS00 * s.F0[d] + dS01 * s.F1[d]);
    P1[d] = (T01 * dF0[d] + T11 * dF1[d]) + (dS01 * s.F0[d] + dS11 * s.F1[d]);
  }
  if (elastic_corners(rec, P0, P1, h)) return ELASTIC_ACTIVE;
  elastic_zero3(h);
  return ELASTIC_OVERFLOW;
}

// w = sum_i k_i y_i of a hinge
__host__ __device__ __forceinline__ void elastic_hinge_w(const float (&k)[4], const float (&y)[4][3], float (&w)[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) w[d] = ((k[0] * y[0][d] + k[1] * y[1][d]) + k[2] * y[2][d]) + k[3] * y[3][d];
}
__host__ __device__ __forceinline__ void elastic_zero4(float (&t)[4][3]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k][0] = t[k][1] = t[k][2] = 0.f;
}
__host__ __device__ __forceinline__ bool elastic_idle4(const float (&k)[4]) { return k[0] == 0.f && k[1] == 0.f && k[2] == 0.f && k[3] == 0.f; }

// t[i] = (kb k_i) w on the four corners; false: a term beyond the float range
__host__ __device__ __forceinline__ bool elastic_hinge_terms(const float (&k)[4], float kb, const float (&w)[3], float (&t)[4][3]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      t[i][d] = (kb * k[i]) * w[d];
      ok = ok && elastic_finite(t[i][d]);
    }
  return ok;
}

// energy kb / 2 |w|^2 of a hinge at x; returns ELASTIC_*
__host__ __device__ __forceinline__ int elastic_hinge_energy(const float (&k)[4], const float (&x)[4][3], float kb, float &energy) {
  energy = 0.f;
  if (elastic_idle4(k)) return ELASTIC_IDLE;
  float w[3];
  elastic_hinge_w(k, x, w);
  const float e = (0.5f * kb) * elastic_dot(w, w);
  if (!elastic_finite(e)) return ELASTIC_OVERFLOW;
  energy = e;
  return ELASTIC_ACTIVE;
}

// energy and gradient g[4][3] of a hinge at x; returns ELASTIC_* (OVERFLOW: energy and gradient 0)
__host__ __device__ __forceinline__ int elastic_hinge_gradient(const float (&k)[4], const float (&x)[4][3], float kb, float &energy, float (&g)[4][3]) {
  energy = 0.f;
  elastic_zero4(g);
  if (elastic_idle4(k)) return ELASTIC_IDLE;
  float w[3];
  elastic_hinge_w(k, x, w);
  const float e = (0.5f * kb) * elastic_dot(w, w);
  if (elastic_hinge_terms(k, kb, w, g) && elastic_finite(e)) {
    energy = e;
    return ELASTIC_ACTIVE;
  }
  elastic_zero4(g);
  return ELASTIC_OVERFLOW;
}

// h[4][3] = (H z) on the four corners of a hinge: the gradient's formula at z (H does not depend on the positions)
__host__ __device__ __forceinline__ int elastic_hinge_product(const float (&k)[4], const float (&z)[4][3], float kb, float (&h)[4][3]) {
  elastic_zero4(h);
  if (elastic_idle4(k)) return ELASTIC_IDLE;
  float w[3];
  elastic_hinge_w(k, z, w);
  if (elastic_hinge_terms(k, kb, w, h)) return ELASTIC_ACTIVE;
  elastic_zero4(h);
  return ELASTIC_OVERFLOW;
}

}  // namespace zsr
