// solve_device.hpp -- the per-vertex 3 x 3 block of the block-Jacobi preconditioner of the mesh Newton system (zpc_amd/csrc/mesh_solve.hip):
// how the blocks of the terms are combined with the mass, and the inverse of the combined block.  Host and device, float32 throughout,
// only + - * / and comparisons, so a float32 chain in numpy (tests/ref64_solve.py) reproduces it bit for bit; translation units that use
// this are built with -ffp-contract=off.
//
// A symmetric block is six floats (xx, xy, xz, yy, yz, zz) = (a, b, c, d, e, f).
//
//   combine   D = scale ((D_elastic + D_barrier) + D_friction), in that order, every entry; then mass is added to xx, yy, zz.
//   inverse   the adjugate over the determinant, operation by operation:
//                 c00 = d f - e e     c01 = c e - b f     c02 = b e - c d
//                 c11 = a f - c c     c12 = b c - a e     c22 = a d - b b
//                 det = (a c00 + b c01) + c c02
//                 inverse = (c00, c01, c02, c11, c12, c22) / det      (six divisions)
//             used where det > 0, det is finite and all six quotients are finite.
//   fallback  everywhere else the scalar Jacobi: the diagonal (1 / a, 1 / d, 1 / f), each where the entry is positive and finite and its
//             reciprocal is finite, else 1 / mass; the off-diagonal entries are zero.  block_inverse returns 1 for the caller to count.
//   fixed     a fixed vertex gets the zero block (the caller's job: the function is not called for it).
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZSR_SOLVE_HD __host__ __device__ inline
#else
#define ZSR_SOLVE_HD inline
#endif

namespace zsr {

ZSR_SOLVE_HD bool solve_finite(float x) { return fabsf(x) <= FLT_MAX; }

// a mass that is not finite and positive marks a fixed vertex
ZSR_SOLVE_HD bool solve_mass_ok(float mass) { return mass > 0.f && mass <= FLT_MAX; }

ZSR_SOLVE_HD void block_combine(const float (&el)[6], const float (&ba)[6], const float (&fr)[6], float scale, float mass, float (&D)[6]) {
  for (int k = 0; k < 6; ++k) D[k] = scale * ((el[k] + ba[k]) + fr[k]);
  D[0] = D[0] + mass;
  D[3] = D[3] + mass;
  D[5] = D[5] + mass;
}

// inv = D^-1 (returns 0) or the scalar Jacobi fallback (returns 1)
ZSR_SOLVE_HD int block_inverse(const float (&D)[6], float mass, float (&inv)[6]) {
  const float a = D[0], b = D[1], c = D[2], d = D[3], e = D[4], f = D[5];
  const float c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const float c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
  const float det = (a * c00 + b * c01) + c * c02;
  if (det > 0.f && solve_finite(det)) {
    inv[0] = c00 / det, inv[1] = c01 / det, inv[2] = c02 / det, inv[3] = c11 / det, inv[4] = c12 / det, inv[5] = c22 / det;
    bool ok = true;
    for (int k = 0; k < 6; ++k) ok = ok && solve_finite(inv[k]);
    if (ok) return 0;
  }
  const float rm = 1.f / mass;
  const float diag[3] = {a, d, f};
  float r[3];
  for (int k = 0; k < 3; ++k) {
    const float q = 1.f / diag[k];
    r[k] = (diag[k] > 0.f && solve_finite(diag[k]) && solve_finite(q)) ? q : rm;
  }
  inv[0] = r[0], inv[1] = 0.f, inv[2] = 0.f, inv[3] = r[1], inv[4] = 0.f, inv[5] = r[2];
  return 1;
}

// z = B r for a symmetric block B: each row left to right
ZSR_SOLVE_HD void block_apply(const float (&B)[6], const float (&r)[3], float (&z)[3]) {
  z[0] = (B[0] * r[0] + B[1] * r[1]) + B[2] * r[2];
  z[1] = (B[1] * r[0] + B[3] * r[1]) + B[4] * r[2];
  z[2] = (B[2] * r[0] + B[4] * r[1]) + B[5] * r[2];
}

}  // namespace zsr
