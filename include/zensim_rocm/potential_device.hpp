// potential_device.hpp -- the arithmetic of the mesh incremental potential (zpc_amd/csrc/mesh_potential.hip) behind its element kernels:
//
//     E(x) = 1/2 (x - xt)^T M (x - xt) + scale (Psi_elastic(x) + B(x) + D(x - start))
//
// the inertia term and the gradient epilogue per vertex, the trial positions of a backtracking line search, the composition of the energy
// from its four float64 totals and the line search's decisions.  Host and device, only + - * and comparisons, float32 unless a double is
// written out, so a numpy chain (tests/ref64_potential.py) reproduces it bit for bit; translation units that use this are built with
// -ffp-contract=off.
//
//   inertia    at a free vertex d = x - xt, e = (0.5f mass) ((d0 d0 + d1 d1) + d2 d2); a fixed vertex has d = 0 and e = 0.
//   gradient   g = mass d + scale acc per component, acc the float32 sum over the runs of the vertex (the caller's gather); a fixed vertex
//              has the zero row.
//   energy     E = parts[0] + (double) scale ((parts[1] + parts[2]) + parts[3]) in float64; parts = inertia, elastic, barrier, friction,
//              each the float64 fixed-order total of its float32 per-element energies.
//   trial      t_0 = tMax, t_{k+1} = shrink t_k; x_k = x + t_k p per component, x_k = x at a fixed vertex; u_k = x_k - start.
//   decision   in float64.  Before the first trial: E_0, slope or tMax not finite, or tMax <= 0 -> not_finite; else slope not < 0 ->
//              not_descent.  Trial k is accepted iff E_k is finite and E_k <= E_0 + ((double) c1 (double) t_k) slope (so the barrier's +inf
//              at zero distance rejects); else trials == maxTrials -> max_trials; else the next trial runs at shrink t_k.
//   fixed      a vertex is fixed where its byte is set or its mass is not finite and positive (solve_device.hpp).
#pragma once
#include <cfloat>
#include <cmath>

#include "solve_device.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZSR_POTENTIAL_HD __host__ __device__ inline
#else
#define ZSR_POTENTIAL_HD inline
#endif

namespace zsr {

enum { POTENTIAL_RUNNING = 0, POTENTIAL_ACCEPTED = 1, POTENTIAL_MAX_TRIALS = 2, POTENTIAL_NOT_DESCENT = 3, POTENTIAL_NOT_FINITE = 4 };

// what a line search leaves on the device: the caller's record.  history [maxTrials + 1] doubles follow (E_0, then one entry per trial)
struct PotentialRecord {
  int trials, flag;
  float t;      // the accepted step; 0 while none is
  float tNext;  // the step of the next trial
  double energy, slope;
};

ZSR_POTENTIAL_HD bool potential_finite(double x) { return fabs(x) <= DBL_MAX; }

ZSR_POTENTIAL_HD bool potential_fixed(const float *mass, const unsigned char *fixed, size_t v) {
  return (fixed && fixed[v]) || !solve_mass_ok(mass[v]);
}

// d = x - xt and the inertia energy of a free vertex
ZSR_POTENTIAL_HD float potential_inertia(const float (&x)[3], const float (&xt)[3], float mass, float (&d)[3]) {
  d[0] = x[0] - xt[0], d[1] = x[1] - xt[1], d[2] = x[2] - xt[2];
  return (0.5f * mass) * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

ZSR_POTENTIAL_HD void potential_gradient(float mass, const float (&d)[3], float scale, const float (&acc)[3], float (&g)[3]) {
  g[0] = mass * d[0] + scale * acc[0];
  g[1] = mass * d[1] + scale * acc[1];
  g[2] = mass * d[2] + scale * acc[2];
}

ZSR_POTENTIAL_HD double potential_energy(const double (&parts)[4], float scale) {
  return parts[0] + (double)scale * ((parts[1] + parts[2]) + parts[3]);
}

ZSR_POTENTIAL_HD void potential_trial(const float (&x)[3], const float (&p)[3], float t, bool fixed, float (&xk)[3]) {
  for (int k = 0; k < 3; ++k) xk[k] = fixed ? x[k] : x[k] + t * p[k];
}

ZSR_POTENTIAL_HD void potential_displacement(const float (&xk)[3], const float (&start)[3], float (&u)[3]) {
  for (int k = 0; k < 3; ++k) u[k] = xk[k] - start[k];
}

// the start of a line search: E_0 and the slope into the record and the history, the first trial's step, the flag
ZSR_POTENTIAL_HD void potential_begin(PotentialRecord &r, double *history, double e0, double slope, float tMax) {
  r.trials = 0, r.t = 0.f, r.tNext = tMax, r.energy = e0, r.slope = slope;
  history[0] = e0;
  if (!potential_finite(e0) || !potential_finite(slope) || !(fabsf(tMax) <= FLT_MAX) || !(tMax > 0.f)) r.flag = POTENTIAL_NOT_FINITE;
  else if (!(slope < 0.0)) r.flag = POTENTIAL_NOT_DESCENT;
  else r.flag = POTENTIAL_RUNNING;
}

ZSR_POTENTIAL_HD bool potential_armijo(double ek, double e0, float c1, float tk, double slope) {
  return potential_finite(ek) && ek <= e0 + ((double)c1 * (double)tk) * slope;
}

// trial r.trials ran at r.tNext and gave ek
ZSR_POTENTIAL_HD void potential_decide(PotentialRecord &r, double *history, double ek, float c1, float shrink, int maxTrials) {
  const float tk = r.tNext;
  const int k = r.trials + 1;
  r.trials = k;
  history[k] = ek;
  if (potential_armijo(ek, history[0], c1, tk, r.slope)) {
    r.t = tk, r.energy = ek, r.flag = POTENTIAL_ACCEPTED;
  } else if (k == maxTrials) {
    r.flag = POTENTIAL_MAX_TRIALS;
  } else {
    r.tNext = shrink * tk;
  }
}

}  // namespace zsr
