#pragma once
// mpm_math.hpp -- per-particle scalar code of the MPM kernels: 3x3 SVD (quaternion Jacobi, per-lane VALU: not a dense contraction,
// so no MFMA), polar decomposition, the packed symmetric stress, Material and the five constitutive models.  Replaces
//   compute_stress_fixedcorotated / _sand ...   cuda/physics/ConstitutiveModel.hpp:10-326, math::svd cuda/math/matrix/svd.cuh
#include "common.hpp"

namespace zsr {

// ======================================================================================= small math
__device__ __forceinline__ float rsq(float x) { return __frsqrt_rn(x); }

#define SVD_GAMMA 5.8284273147583007813f
#define SVD_CSTAR 0.9238795325112867f
#define SVD_SSTAR 0.3826834323650898f

// one Jacobi conjugation in the (X,Y) plane of the symmetric matrix S, accumulated into quaternion q=(w,v)
template <int X, int Y, int Z> __device__ __forceinline__ void jacobi_conj(float (&S)[3][3], float (&q)[4]) {
  float sh = S[X][Y] * 0.5f;
  float ch = S[X][X] - S[Y][Y];
  const bool ok = sh * sh >= 1.e-20f;
  sh = ok ? sh : 0.f;
  ch = ok ? ch : 1.f;
  float sh2 = sh * sh, ch2 = ch * ch;
  const float w = rsq(sh2 + ch2);
  sh *= w;
  ch *= w;
  const bool fix = ch2 <= SVD_GAMMA * sh2;  // angle too large for the approximation: use pi/8
  sh = fix ? SVD_SSTAR : sh;
  ch = fix ? SVD_CSTAR : ch;
  sh2 = sh * sh;
  ch2 = ch * ch;
  const float c = ch2 - sh2, s = 2.f * sh * ch;
  const float sxx = S[X][X], sxy = S[X][Y], syy = S[Y][Y], sxz = S[X][Z], syz = S[Y][Z];
  const float t1 = c * sxx + s * sxy, t2 = c * sxy + s * syy;
  const float t3 = -s * sxx + c * sxy, t4 = -s * sxy + c * syy;
  S[X][X] = c * t1 + s * t2;
  S[X][Y] = S[Y][X] = c * t3 + s * t4;
  S[Y][Y] = -s * t3 + c * t4;
  S[X][Z] = S[Z][X] = c * sxz + s * syz;
  S[Y][Z] = S[Z][Y] = -s * sxz + c * syz;
  const float qw = q[0], qx = q[1 + X], qy = q[1 + Y], qz = q[1 + Z];
  q[0] = qw * ch - qz * sh;
  q[1 + X] = qx * ch + qy * sh;
  q[1 + Y] = qy * ch - qx * sh;
  q[1 + Z] = qz * ch + qw * sh;
}

template <int A, int B, bool SWAPV> __device__ __forceinline__ void cond_swap_cols(float (&rho)[3], float (&Bm)[3][3], float (&Vm)[3][3]) {
  const bool sw = rho[A] < rho[B];
  const float ra = rho[A], rb = rho[B];
  rho[A] = sw ? rb : ra;
  rho[B] = sw ? ra : rb;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float ba = Bm[r][A], bb = Bm[r][B];
    Bm[r][A] = sw ? bb : ba;
    Bm[r][B] = sw ? -ba : bb;
    if constexpr (SWAPV) {
      const float va = Vm[r][A], vb = Vm[r][B];
      Vm[r][A] = sw ? vb : va;
      Vm[r][B] = sw ? -va : vb;
    }
  }
}

template <int P, int R> __device__ __forceinline__ void qr_step(float (&Bm)[3][3], float (&Um)[3][3]) {
  const float a1 = Bm[P][P], a2 = Bm[R][P];
  const float rho2 = a1 * a1 + a2 * a2;
  const bool ok = rho2 > 1.e-24f;
  const float ir = rsq(ok ? rho2 : 1.f);
  const float c = ok ? a1 * ir : 1.f, s = ok ? a2 * ir : 0.f;
#pragma unroll
  for (int col = 0; col < 3; ++col) {
    const float bp = Bm[P][col], br = Bm[R][col];
    Bm[P][col] = c * bp + s * br;
    Bm[R][col] = -s * bp + c * br;
  }
#pragma unroll
  for (int row = 0; row < 3; ++row) {
    const float up = Um[row][P], ur = Um[row][R];
    Um[row][P] = c * up + s * ur;
    Um[row][R] = -s * up + c * ur;
  }
}

// A = U diag(S) V^T; U, V rotations, |S0| >= |S1| >= |S2| (math::svd convention).  Outputs as [row][col] arrays:
// Um, Sg, and -- only when asked for -- Vm (sorted) and Bs = A V (sorted, before the QR), which lets the caller form
// P F^T = U diag(Phat) (F V)^T without ever building P or re-multiplying by F.
template <bool NEED_V, bool NEED_B>
__device__ __forceinline__ void svd3_core(const float (&A)[9], float (&Um)[3][3], float (&Sg)[3], float (&Vm)[3][3], float (&Bs)[3][3]) {
  float S[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S[i][j] = A[3 * i] * A[3 * j] + A[1 + 3 * i] * A[1 + 3 * j] + A[2 + 3 * i] * A[2 + 3 * j];
  float q[4] = {1.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int sweep = 0; sweep < 4; ++sweep) {
    jacobi_conj<0, 1, 2>(S, q);
    jacobi_conj<1, 2, 0>(S, q);
    jacobi_conj<2, 0, 1>(S, q);
  }
  const float n = rsq(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float w = q[0] * n, x = q[1] * n, y = q[2] * n, z = q[3] * n;
  Vm[0][0] = 1 - 2 * (y * y + z * z); Vm[0][1] = 2 * (x * y - w * z);     Vm[0][2] = 2 * (x * z + w * y);
  Vm[1][0] = 2 * (x * y + w * z);     Vm[1][1] = 1 - 2 * (x * x + z * z); Vm[1][2] = 2 * (y * z - w * x);
  Vm[2][0] = 2 * (x * z - w * y);     Vm[2][1] = 2 * (y * z + w * x);     Vm[2][2] = 1 - 2 * (x * x + y * y);
  float Bm[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Bm[r][c] = A[r] * Vm[0][c] + A[r + 3] * Vm[1][c] + A[r + 6] * Vm[2][c];
  float rho[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) rho[c] = Bm[0][c] * Bm[0][c] + Bm[1][c] * Bm[1][c] + Bm[2][c] * Bm[2][c];
  cond_swap_cols<0, 1, NEED_V>(rho, Bm, Vm);
  cond_swap_cols<0, 2, NEED_V>(rho, Bm, Vm);
  cond_swap_cols<1, 2, NEED_V>(rho, Bm, Vm);
  if constexpr (NEED_B) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Bs[r][c] = Bm[r][c];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Um[r][c] = r == c ? 1.f : 0.f;
  qr_step<0, 1>(Bm, Um);
  qr_step<0, 2>(Bm, Um);
  qr_step<1, 2>(Bm, Um);
  Sg[0] = Bm[0][0]; Sg[1] = Bm[1][1]; Sg[2] = Bm[2][2];
}

// column-major 9-vector interface (diagnostic entry point zs_rocm_svd3)
__device__ __forceinline__ void svd3(const float (&A)[9], float (&U)[9], float (&Sg)[3], float (&V)[9]) {
  float Um[3][3], Vm[3][3], Bs[3][3];
  svd3_core<true, false>(A, Um, Sg, Vm, Bs);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      U[r + 3 * c] = Um[r][c];
      V[r + 3 * c] = Vm[r][c];
    }
}

// out = M1 diag(d) M2^T (math/matrix/MatrixUtils.h:26-47)
__device__ __forceinline__ void mat_diag_matT(float (&out)[9], const float (&m1)[9], const float (&d)[3], const float (&m2)[9]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r + 3 * c] = m1[r] * d[0] * m2[c] + m1[r + 3] * d[1] * m2[c + 3] + m1[r + 6] * d[2] * m2[c + 6];
}
__device__ __forceinline__ void pft_vol(const float (&P)[9], const float (&F)[9], float volume, float (&PF)[9]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) PF[r + 3 * c] = (P[r] * F[c] + P[r + 3] * F[c + 3] + P[r + 6] * F[c + 6]) * volume;
}

// The cached stress attribute (`particles.stress`, written by the tail of G2P / update_stress, read by P2G): P F^T vol is the Kirchhoff
// stress times the volume, symmetric for every isotropic model of P2G.hpp:82-101 (and for the fluid: -p I + viscosity (C + C^T)), so it
// is stored as its 6 distinct components {xx, xy, xz, yy, yz, zz} -- 24 instead of 36 bytes per particle on both the G2P write and the
// P2G read (88 instead of 100 B of particle state per P2G particle).  The symmetric part is taken: the off-diagonal pairs of the
// computed product differ by rounding only.
constexpr int STRESS_N = 6;
__device__ __forceinline__ void stress_pack(const float (&PF)[9], float (&S)[STRESS_N]) {
  S[0] = PF[0];
  S[1] = 0.5f * (PF[1] + PF[3]);
  S[2] = 0.5f * (PF[2] + PF[6]);
  S[3] = PF[4];
  S[4] = 0.5f * (PF[5] + PF[7]);
  S[5] = PF[8];
}
__device__ __forceinline__ void stress_unpack(const float (&S)[STRESS_N], float (&PF)[9]) {
  PF[0] = S[0]; PF[1] = S[1]; PF[2] = S[2];
  PF[3] = S[1]; PF[4] = S[3]; PF[5] = S[4];
  PF[6] = S[2]; PF[7] = S[4]; PF[8] = S[5];
}

struct Material {
  float volume, mu, lam, cohesion, beta, yieldSurface;
  int volCorrection;
  float yieldStress;           // von Mises
  float bm, xi, Msqr;          // NACC: bulk modulus NACCConfig::bulk(), hardening factor, M^2
  int hardeningOn;
  float bulk, viscosity;       // EquationOfState
  // derived on the host once (make_dev) so that the kernels find them in SGPRs: computed per wave they are loop invariants the compiler
  // hoists into VGPRs, and in the 128-register fused kernels every such register is a spill (r05: scratch reloads behind the record
  // prefetch = a full memory latency per chunk)
  float smu;                   // 2 mu
  float dpCoef;                // DruckerPrager: (3 lam + 2 mu) / (2 mu)
  float expCohesion;           // DruckerPrager: exp(cohesion)
};

// compute_stress_fixedcorotated (cuda/physics/ConstitutiveModel.hpp:10-47).  The reference forms P = U diag(Phat) V^T and
// then P F^T; since (F V) is already available from the SVD, P F^T = U diag(Phat) (F V)^T is formed directly.
__device__ __forceinline__ void stress_fixedcorotated(const Material &m, const float (&F)[9], float (&PF)[9]) {
  float U[3][3], S[3], V[3][3], B[3][3];
  svd3_core<false, true>(F, U, S, V, B);
  const float J = S[0] * S[1] * S[2];
  const float smu = 2.f * m.mu, slam = m.lam * (J - 1.f);
  float Ph[3];
  Ph[0] = (smu * (S[0] - 1.f) + slam * (S[1] * S[2])) * m.volume;
  Ph[1] = (smu * (S[1] - 1.f) + slam * (S[0] * S[2])) * m.volume;
  Ph[2] = (smu * (S[2] - 1.f) + slam * (S[0] * S[1])) * m.volume;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float u0 = U[r][0] * Ph[0], u1 = U[r][1] * Ph[1], u2 = U[r][2] * Ph[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) PF[r + 3 * c] = u0 * B[c][0] + u1 * B[c][1] + u2 * B[c][2];
  }
}

// compute_stress_sand (cuda/physics/ConstitutiveModel.hpp:246-326): Drucker-Prager return mapping in log-strain.
// logJp is updated.  The reference overwrites F with the projected F_e = U diag(New_S) V^T and then forms
// P F_e^T * vol with P = U diag(Phat) V^T; with V^T V = I that product is U diag(Phat_i New_S_i) U^T * vol -- the
// Kirchhoff stress -- so neither P nor V is needed for the force.  WRITE_F: also return the projected F (test entry).
template <bool WRITE_F>
__device__ __forceinline__ void stress_sand(const Material &m, float &logJp, float (&F)[9], float (&PF)[9]) {
  float U[3][3], S[3], V[3][3], B[3][3];
  svd3_core<WRITE_F, false>(F, U, S, V, B);
  const float smu = m.smu;
  float eps[3], NS[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float a = fabsf(S[i]);
    a = a > 1e-4f ? a : 1e-4f;
    eps[i] = logf(a) - m.cohesion;
  }
  const float sum_eps = eps[0] + eps[1] + eps[2];
  const float tr = sum_eps + logJp;
  float eh[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) eh[i] = eps[i] - (tr * (1.f / 3.f));
  const float ehn = sqrtf(eh[0] * eh[0] + eh[1] * eh[1] + eh[2] * eh[2]);
  bool newF = false;
  float Hs[3] = {0.f, 0.f, 0.f};  // log of the projected singular values
  if (tr >= 0.f) {  // case II: cone tip
    NS[0] = NS[1] = NS[2] = m.expCohesion;
    Hs[0] = Hs[1] = Hs[2] = m.cohesion;
    newF = true;
    if (m.volCorrection) logJp = m.beta * sum_eps + logJp;
  } else if (m.mu != 0.f) {
    logJp = 0.f;
    const float dg = ehn + m.dpCoef * tr * m.yieldSurface;
    float H[3];
    if (dg <= 0.f) {  // case I: inside the cone
#pragma unroll
      for (int i = 0; i < 3; ++i) H[i] = eps[i] + m.cohesion;
    } else {  // case III: onto the cone surface
      const float sc = dg * __frcp_rn(ehn);
#pragma unroll
      for (int i = 0; i < 3; ++i) H[i] = eps[i] - sc * eh[i] + m.cohesion;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if constexpr (WRITE_F) NS[i] = expf(H[i]);
      else NS[i] = 1.f;  // only its positivity matters below
      Hs[i] = H[i];
    }
    newF = true;
  }
  // New_S_log = log(New_S) (ConstitutiveModel.hpp:309): New_S = exp(H), so log(New_S) == H up to one rounding; the
  // mu == 0 && trace < 0 corner keeps the reference's log(0) = -inf
  float tau[3];
  {
    float lg[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) lg[i] = NS[i] > 0.f ? Hs[i] : -INFINITY;
    const float trl = lg[0] + lg[1] + lg[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) tau[i] = (smu * lg[i] + m.lam * trl) * m.volume;  // Phat_i * New_S_i * vol
  }
  if (newF) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float u0 = U[r][0] * tau[0], u1 = U[r][1] * tau[1], u2 = U[r][2] * tau[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) PF[r + 3 * c] = u0 * U[c][0] + u1 * U[c][1] + u2 * U[c][2];
    }
    if constexpr (WRITE_F) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float u0 = U[r][0] * NS[0], u1 = U[r][1] * NS[1], u2 = U[r][2] * NS[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) F[r + 3 * c] = u0 * V[c][0] + u1 * V[c][1] + u2 * V[c][2];
      }
    }
  } else {
    // mu == 0 && trace < 0: F is not projected and New_S = 0 (reference corner case): P = U diag(-inf/0) V^T -> NaN/inf;
    // reproduce "non-finite" without caring about the exact pattern
#pragma unroll
    for (int d = 0; d < 9; ++d) PF[d] = tau[0];
  }
}

// compute_stress_vonmisesfixedcorotated (cuda/physics/ConstitutiveModel.hpp:47-116): von Mises return mapping of the
// Kirchhoff stress in principal space, F projected in place (the caller decides whether it is stored), then the
// fixed-corotated P F^T vol of the projected state.
__device__ __forceinline__ void stress_vonmises(const Material &m, float (&F)[9], float (&PF)[9]) {
  float U[9], S[3], V[9];
  svd3(F, U, S, V);
  float Sc[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) Sc[d] = 1e-4f > S[d] ? 1e-4f : S[d];
  float J = Sc[0] * Sc[1] * Sc[2];
  float tau[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) tau[d] = 2 * m.mu * (Sc[d] - 1) * Sc[d] + m.lam * (J - 1) * J;
  const float tr = tau[0] + tau[1] + tau[2];
  float st[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) st[d] = tau[d] - (tr / 3.f);
  const float s_norm = sqrtf(st[0] * st[0] + st[1] * st[1] + st[2] * st[2]);
  const float scaled_tauy = sqrtf(2.f / (6.f - 3.f)) * m.yieldStress;
  if (s_norm - scaled_tauy > 0) {
    const float alpha = scaled_tauy / s_norm;
    J = 1.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float tau_new = alpha * st[d] + (tr / 3.f);
      const float b2m4ac = m.mu * m.mu - 2 * m.mu * (m.lam * (J - 1) * J - tau_new);
      S[d] = (m.mu + sqrtf(b2m4ac)) / (2 * m.mu);
    }
    mat_diag_matT(F, U, S, V);
  }
  J = S[0] * S[1] * S[2];
  const float smu = 2.f * m.mu, slam = m.lam * (J - 1.f);
  float Ph[3], P[9];
  Ph[0] = smu * (S[0] - 1.f) + slam * (S[1] * S[2]);
  Ph[1] = smu * (S[1] - 1.f) + slam * (S[0] * S[2]);
  Ph[2] = smu * (S[2] - 1.f) + slam * (S[0] * S[1]);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) P[r + 3 * c] = Ph[0] * U[r] * V[c] + Ph[1] * U[r + 3] * V[c + 3] + Ph[2] * U[r + 6] * V[c + 6];
  pft_vol(P, F, m.volume, PF);
}

// compute_stress_nacc (cuda/physics/ConstitutiveModel.hpp:118-243): non-associated Cam-Clay, three projection cases +
// hardening through logJp; F projected in place; neo-Hookean-type P F^T vol of the projected state.
__device__ __forceinline__ void stress_nacc(const Material &m, float &logJp, float (&F)[9], float (&PF)[9]) {
  float U[9], S[3], V[9];
  svd3(F, U, S, V);
  const float bm = m.bm, beta = m.beta, Msqr = m.Msqr, mu = m.mu;
  const float p0 = bm * (0.00001f + sinhf(m.xi * (-logJp > 0 ? -logJp : 0)));
  const float p_min = -beta * p0;
  const float Je_trial = S[0] * S[1] * S[2];
  const float Bh[3] = {S[0] * S[0], S[1] * S[1], S[2] * S[2]};
  const float trB = (Bh[0] + Bh[1] + Bh[2]) / 3.f;
  const float Jm = mu * powf(Je_trial, -2.f / 3.f);
  const float sh[3] = {Jm * (Bh[0] - trB), Jm * (Bh[1] - trB), Jm * (Bh[2] - trB)};
  const float psi = bm * 0.5f * (Je_trial - 1.f / Je_trial);
  const float p_trial = -psi * Je_trial;
  const float ys = 3.f / 2.f * (1 + 2.f * beta);
  const float yp = (Msqr * (p_trial - p_min) * (p_trial - p0));
  const float sn = sh[0] * sh[0] + sh[1] * sh[1] + sh[2] * sh[2];
  const float y = (ys * sn) + yp;
  if (p_trial > p0) {  // case 1: max tip
    const float Je_new = sqrtf(-2.f * p0 / bm + 1.f);
    S[0] = S[1] = S[2] = powf(Je_new, 1.f / 3.f);
    mat_diag_matT(F, U, S, V);
    if (m.hardeningOn) logJp += logf(Je_trial / Je_new);
  } else if (p_trial < p_min) {  // case 2: min tip
    const float Je_new = sqrtf(-2.f * p_min / bm + 1.f);
    S[0] = S[1] = S[2] = powf(Je_new, 1.f / 3.f);
    mat_diag_matT(F, U, S, V);
    if (m.hardeningOn) logJp += logf(Je_trial / Je_new);
  } else if (y >= 1e-4) {  // case 3: onto the yield surface + hardening
    const float Bs = powf(Je_trial, 2.f / 3.f) / mu * sqrtf(-yp / ys) / sqrtf(sn);
#pragma unroll
    for (int i = 0; i < 3; ++i) S[i] = sqrtf(sh[i] * Bs + trB);
    mat_diag_matT(F, U, S, V);
    if (m.hardeningOn && p0 > 1e-4 && p_trial < p0 - 1e-4 && p_trial > 1e-4 + p_min) {
      const float pc = (1.f - beta) * p0 / 2;
      const float q_trial = sqrtf(3.f / 2.f * sn);
      float dir[2] = {pc - p_trial, -q_trial};
      const float dn = sqrtf(dir[0] * dir[0] + dir[1] * dir[1]);
      dir[0] /= dn;
      dir[1] /= dn;
      const float Cq = Msqr * (pc - p_min) * (pc - p0);
      const float Bq = Msqr * dir[0] * (2 * pc - p0 - p_min);
      const float Aq = Msqr * dir[0] * dir[0] + (1 + 2 * beta) * dir[1] * dir[1];
      const float l1 = (-Bq + sqrtf(Bq * Bq - 4 * Aq * Cq)) / (2 * Aq);
      const float l2 = (-Bq - sqrtf(Bq * Bq - 4 * Aq * Cq)) / (2 * Aq);
      const float p1 = pc + l1 * dir[0], p2 = pc + l2 * dir[0];
      const float pf = (p_trial - pc) * (p1 - pc) > 0 ? p1 : p2;
      const float tJ = (-2 * pf / bm + 1);
      const float Jf = sqrtf(tJ > 0 ? tJ : -tJ);
      if (Jf > 1e-4) logJp += logf(Je_trial / Jf);
    }
  }
  const float J = S[0] * S[1] * S[2];
  float b[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) b[r + 3 * c] = F[r] * F[c] + F[r + 3] * F[c + 3] + F[r + 6] * F[c + 6];  // F F^T
  const float trb = (b[0] + b[4] + b[8]) / 3.f;
  b[0] -= trb; b[4] -= trb; b[8] -= trb;
  const float dc = mu * powf(J, -2.f / 3.f), ic = bm * .5f * (J * J - 1.f);
#pragma unroll
  for (int d = 0; d < 9; ++d) PF[d] = (dc * b[d] + ((d & 3) ? 0.f : ic)) * m.volume;
}

// EquationOfState branch of P2GTransfer (simulation/transfer/P2G.hpp:60-81): J = particles.J, C = particles.C
__device__ __forceinline__ void stress_eos(const Material &m, float J, const float (&C)[9], float (&PF)[9]) {
  const float vol = m.volume * J;
  float pressure = m.bulk;
  {
    const float J2 = J * J, J4 = J2 * J2;
    pressure = pressure * (1 / (J * J2 * J4) - 1);
  }
  PF[0] = ((C[0] + C[0]) * m.viscosity - pressure) * vol;
  PF[1] = (C[1] + C[3]) * m.viscosity * vol;
  PF[2] = (C[2] + C[6]) * m.viscosity * vol;
  PF[3] = (C[3] + C[1]) * m.viscosity * vol;
  PF[4] = ((C[4] + C[4]) * m.viscosity - pressure) * vol;
  PF[5] = (C[5] + C[7]) * m.viscosity * vol;
  PF[6] = (C[6] + C[2]) * m.viscosity * vol;
  PF[7] = (C[7] + C[5]) * m.viscosity * vol;
  PF[8] = ((C[8] + C[8]) * m.viscosity - pressure) * vol;
}
// the fluid model keeps J where the solids keep F (component 0 of the `F` attribute); -2 = fluid without a constitutive
// update in G2P (the G2P kernels' "no model" value for solids is -1)
constexpr int MPM_FLUID_NO_STRESS = -2;
__host__ __device__ constexpr bool model_is_fluid(int model) { return model == ZS_MPM_EQUATION_OF_STATE || model == MPM_FLUID_NO_STRESS; }
// which models carry the scalar plastic state logJp (P2G.hpp:88-101)
__host__ __device__ constexpr bool model_uses_logjp(int model) { return model == ZS_MPM_DRUCKER_PRAGER || model == ZS_MPM_NACC; }
// one entry point for the four constitutive models of P2G.hpp:82-101.  F is the local copy: the plastic models project it
// in place, P2G / G2P never store it back (only logJp), the test entry zs_rocm_mpm_stress does (WRITE_F).
template <int MODEL, bool WRITE_F = false>
__device__ __forceinline__ void model_stress(const Material &m, float &logJp, float (&F)[9], float (&PF)[9], const float (&C)[9]) {
  if constexpr (MODEL == ZS_MPM_EQUATION_OF_STATE) stress_eos(m, F[0], C, PF);
  else if constexpr (MODEL == ZS_MPM_FIXED_COROTATED) stress_fixedcorotated(m, F, PF);
  else if constexpr (MODEL == ZS_MPM_DRUCKER_PRAGER) stress_sand<WRITE_F>(m, logJp, F, PF);
  else if constexpr (MODEL == ZS_MPM_VONMISES_FIXED_COROTATED) stress_vonmises(m, F, PF);
  else stress_nacc(m, logJp, F, PF);
}

}  // namespace zsr
