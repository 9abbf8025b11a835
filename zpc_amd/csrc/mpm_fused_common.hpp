#pragma once
// mpm_fused_common.hpp -- what the fused G2P2G steps on compact storage (mpm_fused_kernels.hpp) and on slotted storage (mpm_slot.hpp)
// share: the particle record of a fused step, the consumers' channel sets, the staged Q-form record and its accumulation, the
// accumulators' way into an LDS arena (acc_to_arena), the per-lane stencil-node terms of the list scatters (StencilNodeLane), and the
// arguments of the compact step's launcher.  No kernel lives here.
#include "mpm_arena.hpp"

namespace zsr {

template <int LW, bool DP, bool FLUID = false> struct RecG {  // fused-step inputs: m, x, F or J (, logJp)
  float pos[3], F[9], m, logJp;
  // `delta`: element offset from the (output) attribute arrays of `ps` to the input arrays -- 0 in place; in the re-ordering
  // step the inputs are read from the other buffer of the same layout at the particle's OLD index
  __device__ __forceinline__ void load(const ParticlesDev &ps, size_t i, long long delta = 0) {
    const POff<LW> o = particle_offset<LW>(ps.pos.chns, i);
    Port<float> pp = ps.pos, pf = ps.F, pm = ps.mass, pl = ps.logJp;
    pp.base += delta; pf.base += delta; pm.base += delta;
    // m and logJp FIRST: they are used after the constitutive update, and the wait counter is in order -- as the last loads of the
    // record their wait (s_waitcnt vmcnt(0) behind the SVD) also waited for every store issued in front of the SVD
    m = pload1<LW>(pm, o);
    if constexpr (DP) {
      pl.base += delta;
      logJp = pload1<LW>(pl, o);
    }
    pload<LW, 3>(pp, o, pos);
    pload_state<LW, FLUID>(pf, o, F);
  }
};

template <int CS> struct ConsumerSet {  // CS 0: m + mv_x, 1: mv_y + mv_z, 2: f_x + f_y, 3: f_z
  static constexpr bool STRESS = CS >= 2;
  static constexpr bool MASS = CS == 0;
  static constexpr int NV = CS == 1 || CS == 2 ? 2 : 1;        // vector-valued channels (a direction d each)
  static constexpr int NA = NV + (MASS ? 1 : 0);               // accumulators per node
  static constexpr int D0 = CS == 0 ? 0 : (CS == 1 ? 1 : (CS == 2 ? 0 : 2));  // first direction; the second is D0 + 1
  static constexpr int CH0 = CS == 0 ? 0 : (CS == 1 ? 2 : (CS == 2 ? 4 : 6));  // first grid channel of the set
};
// Staged record of the role-split kernels (r05, "Q form"): what a particle adds to node (a, b, c) of its stencil in vector channel j is
//   W_abc (alpha_j + (a - 1) bx_j + (b - 1) by_j + (c - 1) bz_j),
// alpha = the channel's value at the CENTRE node of the stencil, b. = its change per node step -- momentum d (P2G.hpp:112-119):
// alpha = m (v_d + C[d, :] . (dx - lp)), b_k = m C[d + 3 k] dx; force d (:104-110): alpha = kscale (P F^T)[d, :] . (dx - lp),
// b_k = kscale (P F^T)[d + 3 k] dx.  The producer (lane = particle, every lane busy) forms the 24 coefficients once; the four
// consumers (lane = cell, a third of the lanes idle, everything repeated per channel set) no longer rebuild the offsets x_i - x_p and
// the products C . (x_i - x_p) per node: 766 -> 585 VALU instructions per consumed round.
//   [0] m, [1..3] d0 = x'/dx - base node (local position in cells, [0.5, 1.5)), [4 + 4 j + {0, 1, 2, 3}] = alpha, bx, by, bz of
//   channel j = mv_x, mv_y, mv_z, f_x, f_y, f_z
constexpr int G2P2G_QF = 28;
__device__ __forceinline__ void stage_qform(const MpmDev &mp, float *st, float pm, const float (&lpn)[3], const float (&vel)[3], const float (&C)[9],
                                            const float (&PF)[9]) {
  const float dxi = mp.dxi;
  const float kscale = mp.fscale;
  float lc[3];  // centre node - particle
#pragma unroll
  for (int k = 0; k < 3; ++k) lc[k] = fmaf(-lpn[k], mp.dx, mp.dx);
  st[0] = pm;
#pragma unroll
  for (int d = 0; d < 3; ++d) st[(1 + d) * 64] = lpn[d];
  const float pmdx = pm * mp.dx, ksdx = mp.fscaleDx;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    float *q = st + (4 + 4 * d) * 64;
    q[0] = pm * (vel[d] + (C[d] * lc[0] + C[3 + d] * lc[1] + C[6 + d] * lc[2]));
    q[64] = pmdx * C[d];
    q[128] = pmdx * C[3 + d];
    q[192] = pmdx * C[6 + d];
    float *g = st + (16 + 4 * d) * 64;
    g[0] = kscale * (PF[d] * lc[0] + PF[3 + d] * lc[1] + PF[6 + d] * lc[2]);
    g[64] = ksdx * PF[d];
    g[128] = ksdx * PF[3 + d];
    g[192] = ksdx * PF[6 + d];
  }
}
template <int CS>
__device__ __forceinline__ void g2p2g_consume_set(const MpmDev &mp, const float *st, int lane, float (&acc)[27][ConsumerSet<CS>::NA]) {
  using S = ConsumerSet<CS>;
  auto f = [&](int k) { return st[k * 64 + lane]; };
  // every staged value of the set first (LDS reads in one go), then the arithmetic: one LDS latency per particle
  float d0s[3], al[S::NV], bx[S::NV], by[S::NV], bz[S::NV];
#pragma unroll
  for (int d = 0; d < 3; ++d) d0s[d] = f(1 + d);
  float pm = 0.f;
  if constexpr (S::MASS) pm = f(0);
#pragma unroll
  for (int j = 0; j < S::NV; ++j) {
    const int q = 4 + 4 * ((S::STRESS ? 3 : 0) + S::D0 + j);
    al[j] = f(q);
    bx[j] = f(q + 1);
    by[j] = f(q + 2);
    bz[j] = f(q + 3);
  }
  asm volatile("" ::: "memory");  // (keeps the compiler from sinking the reads back between the fmas)
  float w[3][3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float d0 = d0s[d];
    w[d][0] = 0.5f * (1.5f - d0) * (1.5f - d0);
    const float d1 = d0 - 1.0f;
    w[d][1] = 0.75f - d1 * d1;
    const float zz = 0.5f + d1;
    w[d][2] = 0.5f * zz * zz;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float qa[S::NV];
#pragma unroll
    for (int j = 0; j < S::NV; ++j) qa[j] = a == 0 ? al[j] - bx[j] : (a == 1 ? al[j] : al[j] + bx[j]);
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      const float wxy = w[0][a] * w[1][bb];
      const float W0 = wxy * w[2][0], W1 = wxy * w[2][1], W2 = wxy * w[2][2];
      auto &A0 = acc[(a * 3 + bb) * 3], &A1 = acc[(a * 3 + bb) * 3 + 1], &A2 = acc[(a * 3 + bb) * 3 + 2];
      if constexpr (S::MASS) {
        A0[0] = fmaf(W0, pm, A0[0]);
        A1[0] = fmaf(W1, pm, A1[0]);
        A2[0] = fmaf(W2, pm, A2[0]);
      }
#pragma unroll
      for (int j = 0; j < S::NV; ++j) {
        const float qab = bb == 0 ? qa[j] - by[j] : (bb == 1 ? qa[j] : qa[j] + by[j]);
        constexpr int o = S::MASS ? 1 : 0;
        A0[o + j] = fmaf(W0, qab - bz[j], A0[o + j]);
        A1[o + j] = fmaf(W1, qab, A1[o + j]);
        A2[o + j] = fmaf(W2, qab + bz[j], A2[o + j]);
      }
    }
  }
}

// The 27 register planes of a consumer lane (lane = cell, acc[k] = its stencil node k) -> the lane's channels of an LDS arena of layout AL;
// a0 = the cell's stencil node 0 in the first of the NA channels.  The channels belong to this wave alone.  In phase k the 64 lanes of the
// wave add to 64 distinct nodes; the next phase touches nodes other lanes wrote in this one, so the phases must stay ordered -- but only
// inside the wave: LDS operations of one wave execute in order, so a wavefront-scope fence (no instruction, it only keeps the compiler from
// hoisting the next phase's reads over this phase's writes) replaces 27 workgroup barriers.  ZERO: the planes are cleared for the next bin.
template <class AL, bool ZERO = false, int NA>
__device__ __forceinline__ void acc_to_arena(float *a0, float (&acc)[27][NA]) {
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    float *g = a0 + AL::at(k / 9, (k / 3) % 3, k % 3);
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      g[q * AL::CH] += acc[k][q];
      if constexpr (ZERO) acc[k][q] = 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
}

// One stencil node (0..26) of a staged record (stage_qform), as the lanes of the list scatters see it (lane = node): only the node's
// weight formula (alpha + beta (s d0 + t)^2 per axis) and its offset from the centre node are per-lane constants; the channels are a
// compile-time loop.
struct StencilNodeLane {
  int sel[3];
  float ws[3], wt[3], wa[3], wb[3], oc[3];
  __device__ __forceinline__ explicit StencilNodeLane(int node) : sel{node / 9, (node / 3) % 3, node % 3} {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ws[q] = sel[q] == 0 ? -1.f : 1.f;
      wt[q] = sel[q] == 0 ? 1.5f : (sel[q] == 1 ? -1.f : -0.5f);
      wa[q] = sel[q] == 1 ? 0.75f : 0.f;
      wb[q] = sel[q] == 1 ? -1.f : 0.5f;
      oc[q] = (float)(sel[q] - 1);
    }
  }
  // axis q's factor of the node's weight; d0 = staged local position of that axis
  __device__ __forceinline__ float weight(int q, float d0) const {
    const float u = fmaf(ws[q], d0 - floorf(d0 - 0.5f), wt[q]);  // the reference's second base_node (see `edge` in slot_produce_entry)
    return fmaf(wb[q], u * u, wa[q]);
  }
  // what the record at `st` adds to this node in accumulator q of channel set CS; Wt = the node's weight
  template <int CS> __device__ __forceinline__ float value(const float *st, float Wt, int q) const {
    using S = ConsumerSet<CS>;
    if (S::MASS && q == 0) return Wt * st[0];  // mass
    const float *c = st + (4 + 4 * ((S::STRESS ? 3 : 0) + S::D0 + q - (S::MASS ? 1 : 0))) * 64;
    return Wt * fmaf(c[192], oc[2], fmaf(c[128], oc[1], fmaf(c[64], oc[0], c[0])));
  }
  // what the record adds to this node in ALL seven grid channels (v[0] mass, v[1 + j] staged channel j: the sets' accumulators in grid
  // order, each the expression of value<CS>); every staged value is read before the first is used
  __device__ __forceinline__ void values(const float *st, float Wt, float (&v)[7]) const {
    float c[6][4];
    const float m = st[0];
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) c[j][k] = st[(4 + 4 * j + k) * 64];
    v[0] = Wt * m;
#pragma unroll
    for (int j = 0; j < 6; ++j) v[1 + j] = Wt * fmaf(c[j][3], oc[2], fmaf(c[j][2], oc[1], fmaf(c[j][1], oc[0], c[j][0])));
  }
};

// fused G2P2G launch for one block side: defined in mpm_fused_impl.hpp, instantiated in mpm_fused4.hip / mpm_fused8.hip (the
// 30 instantiations per side of the largest kernel compile in parallel)
struct FusedArgs {
  const float *gridA;
  float *gridB;
  const int *binStart;
  const unsigned *cellCount;
  const int *nbr;
  int *staleG, *staleP, *counts, *driftFlag;
  unsigned nbins;
  int binBase, writeAll, lw, model;
  const int *order;   // re-ordering step: input slot of output slot i (nullptr: in place)
  long long inDelta;  // element offset from the output attribute arrays to the input ones
};
template <int S> void g2p2g_launch_side(Launch &L, const MpmDev &mp, const ParticlesDev &pd, const BhtDev &t, const FusedArgs &a);

}  // namespace zsr
