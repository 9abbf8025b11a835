// ccd_device.hpp -- ccd_pt / ccd_ee: a conservative bound on the step t in [0, tMax] along a direction p for which a point-triangle or an
// edge-edge pair at x + t p stays free of contact, by additive CCD (Li et al. 2021, "Codimensional Incremental Potential Contact", 4.3):
// conservative advancement on the unsigned distance of tri_closest / ee_closest (distance_device.hpp).  No root finding: the reference's
// vertexFaceCCD / edgeEdgeCCD (geometry/Geometry.hpp) answer yes or no over rational arithmetic and give no step length.  Written from the
// geometry:
//   relative motion   the distance does not change when all four corners move by the same vector, so the mean m of the four rows of p is
//                     subtracted first, q_k = p_k - m (four equal rows give q = 0 exactly: (a + a) + (a + a) and the product with 1/4 are
//                     exact).  Over a step t a point of the triangle (of an edge) moves by at most t max |q_k| of its corners, so the
//                     distance falls by at most t l_p,
//                         PT: l_p = |q_0| + max(|q_1|, |q_2|, |q_3|)        EE: l_p = max(|q_0|, |q_1|) + max(|q_2|, |q_3|).
//                     ANY common vector may be subtracted, so the rounding of m costs nothing; what is rounded is q (1 rounding, u = 2^-24),
//                     the squares and their sum (3 u on a sum of positive terms), the root (1/2 of that + 1) and the sum of two norms (1):
//                     4.5 u relative.  l_p is multiplied by 1 + 8 u (CCD_LP_UP), so it is never below the exact value for the same float32
//                     rows, in particular never below the float64 value.  Squares of components under 1e-19 leave the normal range; with
//                     the largest |q_kd| under 1e-10 (CCD_LP_TINY) the bound is 4 max |q_kd| instead (>= 2 sqrt(3) max |q_kd| >= l_p), above
//                     it the underflow is at most 2e-19 per norm, 4e-9 of l_p.  l_p == 0: nothing moves relatively, t = tMax.
//   start             d0 = the distance at t = 0; d0 == 0: t = 0, status CCD_ZERO.  g = slack d0 is the gap the step keeps.  The first
//                     increment t_l = (1 - slack) d0 / l_p cannot bring the distance under g; t_l >= tMax ends the pair at tMax without
//                     another distance evaluation (the early out: most pairs of a candidate list).
//   loop              the distance d at x + t' p, t' = min(t + t_l, tMax) -- one product, one sum, from the original x: the expression a
//                     float32 caller applies the step with, never accumulated positions.  t > 0 and d < g: stop, the answer is t.
//                     Otherwise t = t' (t == tMax: the answer) and t_l = 0.9 d / l_p.  The evaluation is clamped to tMax, not the answer
//                     after it: an increment that overshoots tMax proves no contact up to tMax, but the gap AT tMax is known only where
//                     the distance was taken (two edges that pass each other at 1.03 tMax are closer than g at tMax and further at
//                     1.03 tMax), and every answer is to keep the gap.  After maxIter evaluations the current t is returned with
//                     status CCD_CAPPED: every t the loop reaches is a valid bound, a slowly closing pair at a tiny distance just gets
//                     there in many steps.
//   NaN, Inf          a NaN or Inf in x or p, an l_p or d0 beyond the float range: t = 0 (status CCD_OK, nothing is counted).  Inside the
//                     loop every test is written so that a NaN distance stops at the t reached so far; no path with a NaN leads to tMax.
// The state between two evaluations is CcdState; ccd_start and ccd_step are the two phases the kernel (zpc_amd/csrc/mesh_ccd.hip) runs in
// different lanes, and ccd_pair is their composition, so a pair's answer does not depend on who computes it.
//
// Float32 limits.  The distance carries the error beta = K u (S + M) of tests/ref64_proximity.py (K = 32 PT, 64 EE; S = distance plus the
// edge lengths, M the largest coordinate), and the positions x + t p another 2 u M per corner.  Every t > 0 the loop accepts had a
// float32 distance >= g, so the true distance there is at least slack d0 - 3 beta (tests/ref64_ccd.py derives the 3); a stop means the
// true distance at t is at most 10 slack d0 + (22 + 16 slack) beta.  A pair with slack d0 <= 2 beta is below that resolution: the same
// code runs, the result is a number in [0, tMax] that stops short of the contact as float32 sees it, but its gap is not guaranteed --
// callers that start this close (coordinates of size 1: d0 under 4e-5 at slack 0.1) should raise slack or treat the pair as touching.
// The step 0.9 d / l_p is safe in exact arithmetic for any factor <= 1; with the error of d it is safe while the true distance stays above
// 9 beta, which slack d0 >= 10 beta guarantees outright and the bound's own slack (K counts worst cases one after the other) in between.
// Translation units that use this are built with -ffp-contract=off, as everything behind tri_closest / ee_closest.
#pragma once
#include <cfloat>
#include <cmath>

#include "distance_device.hpp"

namespace zsr {

enum { CCD_OK = 0, CCD_ZERO = 1, CCD_CAPPED = 2 };
constexpr float CCD_LP_UP = 1.f + 0x1p-21f;  // 1 + 8 u
constexpr float CCD_LP_TINY = 1e-10f;
constexpr float CCD_ADVANCE = 0.9f;

struct CcdState {
  float t, tl, lp, g;  // the step reached, the next increment, the bound on the relative speed, the gap to keep
  int evals;           // distance evaluations of the loop so far
};

template <bool EE>
__host__ __device__ __forceinline__ float ccd_distance(const float (&x)[4][3]) {
  if constexpr (EE)
    return sqrtf(ee_closest(x[0], x[1], x[2], x[3]).dist2);
  else
    return sqrtf(tri_closest(x[0], x[1], x[2], x[3]).dist2);
}

__host__ __device__ __forceinline__ float ccd_max(float a, float b) { return a > b ? a : b; }

// l_p of the header comment; NaN for a NaN or Inf in p
template <bool EE>
__host__ __device__ __forceinline__ float ccd_speed_bound(const float (&p)[4][3]) {
  float n[4], amax = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) n[k] = 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float m = ((p[0][d] + p[1][d]) + (p[2][d] + p[3][d])) * 0.25f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float q = p[k][d] - m;
      n[k] = d == 0 ? q * q : n[k] + q * q;
      amax = ccd_max(amax, fabsf(q));
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) n[k] = sqrtf(n[k]);
  const float lp = EE ? ccd_max(n[0], n[1]) + ccd_max(n[2], n[3]) : n[0] + ccd_max(n[1], ccd_max(n[2], n[3]));
  return amax < CCD_LP_TINY ? 4.f * amax : lp * CCD_LP_UP;
}

// steps 1 and 2: true = the pair is finished with s.t and status; false = s holds the state in front of the first evaluation of the loop
template <bool EE>
__host__ __device__ __forceinline__ bool ccd_start(const float (&x)[4][3], const float (&p)[4][3], float slack, float tMax, CcdState &s,
                                                   int &status) {
  status = CCD_OK;
  s.t = 0.f, s.tl = 0.f, s.lp = 0.f, s.g = 0.f, s.evals = 0;
  float finite = 0.f;  // 0 x anything finite = +-0; a NaN or Inf makes it NaN
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) finite += x[k][d] * 0.f + p[k][d] * 0.f;
  if (!(finite == 0.f)) return true;
  s.lp = ccd_speed_bound<EE>(p);
  if (!(s.lp <= FLT_MAX)) return true;
  if (s.lp == 0.f) {
    s.t = tMax;
    return true;
  }
  const float d0 = ccd_distance<EE>(x);
  if (!(d0 <= FLT_MAX)) return true;
  if (d0 == 0.f) {
    status = CCD_ZERO;
    return true;
  }
  s.g = slack * d0;
  s.tl = ((1.f - slack) * d0) / s.lp;
  if (s.tl >= tMax) {
    s.t = tMax;
    return true;
  }
  return false;
}

// one evaluation of the loop: true = finished with s.t and status
template <bool EE>
__host__ __device__ __forceinline__ bool ccd_step(const float (&x)[4][3], const float (&p)[4][3], float tMax, int maxIter, CcdState &s,
                                                  int &status) {
  float tt = s.t + s.tl;
  if (tt >= tMax) tt = tMax;
  float y[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) y[k][d] = x[k][d] + tt * p[k][d];
  const float d = ccd_distance<EE>(y);
  ++s.evals;
  if (!(d >= s.g) && (s.t > 0.f || d != d)) return true;
  s.t = tt;
  if (s.t >= tMax) return true;
  s.tl = (CCD_ADVANCE * d) / s.lp;
  if (s.evals >= maxIter) {
    status = CCD_CAPPED;
    return true;
  }
  return false;
}

template <bool EE>
__host__ __device__ __forceinline__ float ccd_pair(const float (&x)[4][3], const float (&p)[4][3], float slack, float tMax, int maxIter,
                                                   int &status, int *evals = nullptr) {
  CcdState s;
  if (!ccd_start<EE>(x, p, slack, tMax, s, status))
    while (!ccd_step<EE>(x, p, tMax, maxIter, s, status)) {}
  if (evals) *evals = s.evals;
  return s.t;
}

// x: the point, then the triangle's a, b, c
__host__ __device__ __forceinline__ float ccd_pt(const float (&x)[4][3], const float (&p)[4][3], float slack, float tMax, int maxIter, int &status,
                                                 int *evals = nullptr) {
  return ccd_pair<false>(x, p, slack, tMax, maxIter, status, evals);
}

// x: a0, a1, b0, b1
__host__ __device__ __forceinline__ float ccd_ee(const float (&x)[4][3], const float (&p)[4][3], float slack, float tMax, int maxIter, int &status,
                                                 int *evals = nullptr) {
  return ccd_pair<true>(x, p, slack, tMax, maxIter, status, evals);
}

}  // namespace zsr
