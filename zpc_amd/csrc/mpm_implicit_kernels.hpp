#pragma once
// mpm_implicit_kernels.hpp -- the implicit-MPM force operator (G2P2GTransfer, simulation/transfer/G2P2G.hpp:14-150): particle order,
// one workgroup per grid block, exact path; included by mpm_implicit.hip only.
//
// Per particle: C from a dof vector of trial node velocities on the stencil of the UNCHANGED position, F_trial = (I + dt C) F (fluid:
// J_trial = (1 + dt tr C) J), the constitutive model on the trial state, contrib = (P F^T vol) D_inv, and W contrib xixp added into a
// second dof vector.  No particle attribute is written (logJp included: the model runs on a local copy, G2P2G.hpp:115).
// Dof vectors are AoS: entry 3 (block side^3 + cell) + d (G2P2G.hpp:71,135-139).
//
// Binned kernel (implicit_block_kernel): the position does not change inside the operator, so gather and scatter share one arena and
// the same weights, and there are no movers to re-slot.  A workgroup owns a grid block, a wave owns one bin of it at a time:
//   * the block's trial velocities (10^3 nodes, side 4: 6^3) are staged in LDS once from the AoS dof vector;
//   * lane = particle over 64 consecutive particles of the bin: sum-factorised gather of B only, constitutive update with every lane
//     busy, then the particle's Q-form record {cell, d0[3], (alpha, bx, by, bz) x 3 force channels} goes to the wave's LDS buffer;
//   * lane = cell: the round-robin order of a bin gives every cell's particles their indices from ballots on the cell counts
//     (RoundWalk), so lane c reads the records of ITS cell from the buffer and accumulates 27 x 3 node sums in registers;
//   * once per bin the register stencils go into the block's force arena in 27 conflict-free phases of ds_read + add + ds_write, the
//     waves of the workgroup taking turns (no LDS float atomics: 193 against 11 cycles per wave-instruction, profiles/);
//   * the force arena reaches fOut once per node by global_atomic_add_f32, apron nodes through `nbr`.
// A particle that is not stored under its cell (it moved since the last re-bin) or whose base node lies outside the block's cells is
// queued and takes the exact particle-order code afterwards: results do not depend on how fresh the bins are.
#include "mpm_arena.hpp"

namespace zsr {

constexpr int IMPL_TRIAL_N = 27;  // floats per particle of the test hook: C_trial, F_trial (fluid: J_trial in slot 0), P F^T vol

// trial state -> P F^T vol (before D_inv); F is F_trial on entry (fluid: J_trial in F[0])
template <int MODEL>
__device__ __forceinline__ void implicit_stress(const MpmDev &mp, const float (&oldF)[9], float logJp, const float (&C)[9], float (&F)[9],
                                                float (&PF)[9]) {
  advance_state<model_is_fluid(MODEL)>(oldF, C, mp.dt, F);
  float Fl[9];
#pragma unroll
  for (int d = 0; d < 9; ++d) Fl[d] = F[d];  // the plastic models project their local copy only
  float lj = logJp;
  model_stress<MODEL>(mp.mat, lj, Fl, PF, C);
}
__device__ __forceinline__ void implicit_store_trial(float *trial, size_t i, const float (&C)[9], const float (&F)[9], const float (&PF)[9]) {
  float *t = trial + i * IMPL_TRIAL_N;
#pragma unroll
  for (int d = 0; d < 9; ++d) {
    t[d] = C[d];
    t[9 + d] = F[d];
    t[18 + d] = PF[d];
  }
}

// the particle's own 3^3 stencil as an "arena" of g2p_gather_lds (register-resident after unrolling)
struct StencilArena {
  static constexpr int CH = 27;
  __device__ static constexpr int at(int x, int y, int z) { return x * 9 + y * 3 + z; }
};

// ---- particle-order path: the reference's algorithm (hash query + global float atomics per node), the 27 queries folded into the
//      <= 8 distinct blocks a stencil can touch and shared by the gather and the scatter.  The gather's SUMS are formed as the binned
//      kernel forms them (see below), so that a particle gets the same trial state on either path
template <int SIDE, int MODEL>
__device__ __forceinline__ void implicit_particle_global(const MpmDev &mp, const ParticlesDev &ps, size_t i, const BhtDev &t, const float *vIn,
                                                         float *fOut, float *trial) {
  constexpr int NC = SIDE * SIDE * SIDE;
  const float D_inv = mp.D_inv;
  float pos[3];
  load_attr<3>(ps.pos, i, pos);
  Arena ar;
  make_arena(mp.dx, mp.dxi, pos, ar);
  int loc[3], key[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    loc[d] = ar.corner[d] & (SIDE - 1);
    key[d] = (ar.corner[d] - loc[d]) / SIDE * mp.kscale;
  }
  int blk[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const bool need = (!(o & 4) || loc[0] + 2 >= SIDE) && (!(o & 2) || loc[1] + 2 >= SIDE) && (!(o & 1) || loc[2] + 2 >= SIDE);
    int k[3] = {key[0] + (o >> 2) * mp.kscale, key[1] + ((o >> 1) & 1) * mp.kscale, key[2] + (o & 1) * mp.kscale};
    blk[o] = need ? bht_query<3>(t, k) : -1;
  }
  auto node_of = [&](int a, int b, int c) -> long long {  // dof node of stencil node (a, b, c), -1: its block is not in the partition
    const int x = loc[0] + a, y = loc[1] + b, z = loc[2] + c;
    const int o = ((x >= SIDE) << 2) | ((y >= SIDE) << 1) | (z >= SIDE);
    int bn = blk[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) bn = (o == q) ? blk[q] : bn;
    if (bn < 0) return -1;
    return (long long)bn * NC + ((x & (SIDE - 1)) * SIDE + (y & (SIDE - 1))) * SIDE + (z & (SIDE - 1));
  };
  // the 27 node velocities by hash query, then the SAME sum-factorised arithmetic as the binned kernel (g2p_gather_lds on a private
  // 3^3 arena): both paths form C_trial, hence F_trial and the stress, from identical operations in identical order.  The
  // constitutive model turns an ulp of F into ~100 u of P F^T vol, so two associations of this sum would give the paths forces that
  // differ by more than the scatter's own rounding.
  float nv[3 * StencilArena::CH];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long node = node_of(a, b, c);
        const float *g = vIn + 3 * (size_t)(node < 0 ? 0 : node);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) nv[ch * StencilArena::CH + StencilArena::at(a, b, c)] = node >= 0 ? g[ch] : 0.f;
      }
  float vel[3], C[9];
  g2p_gather_lds<StencilArena>(mp, ar, nv, D_inv, vel, C);
  float oldF[9], F[9], PF[9];
  load_state<model_is_fluid(MODEL)>(ps.F, i, oldF);
  float lj = 0.f;
  if constexpr (model_uses_logjp(MODEL)) lj = ps.logJp.base[ps.logJp.off(i)];
  implicit_stress<MODEL>(mp, oldF, lj, C, F, PF);
  if (trial) implicit_store_trial(trial, i, C, F, PF);
  float contrib[9];
#pragma unroll
  for (int d = 0; d < 9; ++d) contrib[d] = PF[d] * D_inv;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long node = node_of(a, b, c);
        if (node < 0) continue;  // the reference does not check (G2P2G.hpp:130); a valid partition never gets here
        const float xi0 = (float)a * mp.dx - ar.lp[0], xi1 = (float)b * mp.dx - ar.lp[1], xi2 = (float)c * mp.dx - ar.lp[2];
        float W = ar.w[0][a];
        W *= ar.w[1][b];
        W *= ar.w[2][c];
        float *g = fOut + 3 * (size_t)node;
#pragma unroll
        for (int d = 0; d < 3; ++d) unsafeAtomicAdd(g + d, W * (contrib[d] * xi0 + contrib[3 + d] * xi1 + contrib[6 + d] * xi2));
      }
}

template <int SIDE, int MODEL>
static __global__ __launch_bounds__(256) void implicit_global_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, const float *vIn, float *fOut,
                                                                     float *trial) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ps.n) return;
  implicit_particle_global<SIDE, MODEL>(mp, ps, i, t, vIn, fOut, trial);
}

template <int SIDE, int MODEL>
static __global__ __launch_bounds__(256) void implicit_stale_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, const float *vIn, float *fOut,
                                                                    float *trial, const int *stale, const int *staleCount) {
  const int n = *staleCount;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    implicit_particle_global<SIDE, MODEL>(mp, ps, (size_t)stale[j], t, vIn, fOut, trial);
}

// ---- binned path
constexpr int IMPL_REC_N = 16;  // rows of a Q-form record: cell code, d0[3], then per force channel alpha, bx, by, bz

// one record -> the lane's 27 x 3 node sums: W_abc (alpha + (a - 1) bx + (b - 1) by + (c - 1) bz), the weights rebuilt from d0 with
// make_arena's own expressions (same bits as the gather's)
__device__ __forceinline__ void implicit_accumulate(const float *rec, float (&acc)[27][3]) {
  float w[3][3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float d0 = rec[(1 + d) * 64];
    w[d][0] = 0.5f * (1.5f - d0) * (1.5f - d0);
    const float d1 = d0 - 1.0f;
    w[d][1] = 0.75f - d1 * d1;
    const float zz = 0.5f + d1;
    w[d][2] = 0.5f * zz * zz;
  }
  float al[3], bx[3], by[3], bz[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    al[j] = rec[(4 + 4 * j) * 64];
    bx[j] = rec[(5 + 4 * j) * 64];
    by[j] = rec[(6 + 4 * j) * 64];
    bz[j] = rec[(7 + 4 * j) * 64];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float qa[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) qa[j] = a == 0 ? al[j] - bx[j] : (a == 1 ? al[j] : al[j] + bx[j]);
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      const float wxy = w[0][a] * w[1][bb];
      const float W0 = wxy * w[2][0], W1 = wxy * w[2][1], W2 = wxy * w[2][2];
      float(&A0)[3] = acc[(a * 3 + bb) * 3], (&A1)[3] = acc[(a * 3 + bb) * 3 + 1], (&A2)[3] = acc[(a * 3 + bb) * 3 + 2];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float qab = bb == 0 ? qa[j] - by[j] : (bb == 1 ? qa[j] : qa[j] + by[j]);
        A0[j] = fmaf(W0, qab - bz[j], A0[j]);
        A1[j] = fmaf(W1, qab, A1[j]);
        A2[j] = fmaf(W2, qab + bz[j], A2[j]);
      }
    }
  }
}

// LDS arena of a block's nodes + apron: dense 10^3 for side 8, the bin arena for side 4 (block == bin)
template <int SIDE> struct ImplicitArena { using type = ArenaBlk; };
template <> struct ImplicitArena<4> { using type = ArenaLds; };

template <int SIDE, int MODEL, int LW>
static __global__ __launch_bounds__(SIDE == 8 ? 256 : 64) void implicit_block_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, const float *vIn,
                                                                                  float *fOut, float *trial, const int *binStart,
                                                                                  const unsigned *cellCount, const int *nbr, int *stale,
                                                                                  int *staleCount) {
  using AL = typename ImplicitArena<SIDE>::type;
  constexpr int NC = SIDE * SIDE * SIDE, W = SIDE + 2, NT = SIDE == 8 ? 256 : 64, NW = NT / 64, BPB = bins_per_block<SIDE>();
  __shared__ float varena[3 * AL::CH];            // trial velocities of the block's nodes + apron
  __shared__ float farena[3 * AL::CH];            // forces of the same nodes
  __shared__ float recs[NW][IMPL_REC_N * 64];     // a wave's 64 Q-form records, row-major by field
  const int blk = (int)blockIdx.x;
  if (binStart[blk * BPB] == binStart[blk * BPB + BPB]) return;  // no particle in this block (workgroup-uniform)
  const int w = NW == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  int borg[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) borg[d] = t.activeKeys[3 * (size_t)blk + d] * (SIDE / mp.kscale);
  for (int node = threadIdx.x; node < W * W * W; node += NT) {
    const int x = node / (W * W), y = (node / W) % W, z = node % W;
    const int slot = ((x >= SIDE) << 2) | ((y >= SIDE) << 1) | (z >= SIDE);
    const int cell = ((x & (SIDE - 1)) * SIDE + (y & (SIDE - 1))) * SIDE + (z & (SIDE - 1));
    const int bn = nbr[(size_t)blk * 8 + slot];
    const float *g = vIn + 3 * ((size_t)(bn < 0 ? 0 : bn) * NC + cell);
    const int a = AL::at(x, y, z);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      varena[a + ch * AL::CH] = bn >= 0 ? g[ch] : 0.f;
      farena[a + ch * AL::CH] = 0.f;
    }
  }
  __syncthreads();
  const float D_inv = mp.D_inv;
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  float *rec = recs[w];
#pragma unroll 1
  for (int pass = 0; pass < BPB / NW; ++pass) {
    const int sub = pass * NW + w, bin = blk * BPB + sub;
    const BinGeom<SIDE> geo(bin);  // (origin of the bin inside the block; org is not used)
    const int start = binStart[bin], end = binStart[bin + 1];
    const int myCode = ((geo.o[0] + cx) * SIDE + geo.o[1] + cy) * SIDE + geo.o[2] + cz;  // this lane's cell of the block
    float acc[27][3];
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[k][j] = 0.f;
    if (start != end) {  // (wave-uniform)
      const unsigned cnt = cellCount[(size_t)bin * 64 + lane];
      RoundWalk walk(cnt, start);
      int pi = 0, rEnd = start;  // this lane's particle of the current round, and where that round ends (wave-uniform)
      bool has = false, done = true;
#pragma unroll 1
      for (int cs = start; cs < end; cs += 64) {
        const int ce = cs + 64 < end ? cs + 64 : end;
        {  // ---- lane = particle: gather, constitutive update, record
          const int i = cs + lane;
          float code = -1.f;
          if (i < ce) {
            RecB<MODEL == ZS_MPM_EQUATION_OF_STATE ? MPM_FLUID_NO_STRESS : MODEL, LW> cur;
            cur.load(ps, (size_t)i);
            Arena ar;
            make_arena(mp.dx, mp.dxi, cur.pos, ar);
            const int ocx = ar.corner[0] - borg[0], ocy = ar.corner[1] - borg[1], ocz = ar.corner[2] - borg[2];
            if ((unsigned)ocx < (unsigned)SIDE && (unsigned)ocy < (unsigned)SIDE && (unsigned)ocz < (unsigned)SIDE) {
              float vel[3], C[9], F[9], PF[9];
              g2p_gather_lds<AL>(mp, ar, varena + AL::at(ocx, ocy, ocz), D_inv, vel, C);
              implicit_stress<MODEL>(mp, cur.F, model_uses_logjp(MODEL) ? cur.logJp : 0.f, C, F, PF);
              if (trial) implicit_store_trial(trial, (size_t)i, C, F, PF);
              code = (float)((ocx * SIDE + ocy) * SIDE + ocz);
              // d0 of make_arena from lp = lpn dx is not exact; recompute it from the position as make_arena does
#pragma unroll
              for (int d = 0; d < 3; ++d) {
                const float X = cur.pos[d] * mp.dxi;
                const float lpn = X - floorf(X - 0.5f);
                rec[(1 + d) * 64 + lane] = lpn - floorf(lpn - 0.5f);
              }
              const float lc[3] = {mp.dx - ar.lp[0], mp.dx - ar.lp[1], mp.dx - ar.lp[2]};  // centre node - particle
              const float sdx = D_inv * mp.dx;
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                rec[(4 + 4 * j) * 64 + lane] = D_inv * (PF[j] * lc[0] + PF[3 + j] * lc[1] + PF[6 + j] * lc[2]);
                rec[(5 + 4 * j) * 64 + lane] = sdx * PF[j];
                rec[(6 + 4 * j) * 64 + lane] = sdx * PF[3 + j];
                rec[(7 + 4 * j) * 64 + lane] = sdx * PF[6 + j];
              }
            } else {
              stale[atomicAdd(staleCount, 1)] = i;  // the base node lies outside the block's cells: exact path (hash queries)
              code = -2.f;
            }
          }
          rec[lane] = code;
        }
        __builtin_amdgcn_wave_barrier();  // (one wave: its LDS operations execute in order)
        // ---- lane = cell: the rounds (or parts of rounds) that lie inside [cs, ce)
        for (;;) {
          if (has && !done && pi < ce) {
            const int q = pi - cs;
            if ((unsigned)q < 64u) {
              const float code = rec[q];
              if (code == (float)myCode) implicit_accumulate(rec + q, acc);
              else if (code >= 0.f) stale[atomicAdd(staleCount, 1)] = pi;  // stored under another cell than its own: exact path
            }
            done = true;
          }
          if (rEnd > ce || rEnd >= end) break;  // the round goes on in the next chunk / the last round is complete
          bool any;
          has = walk.next(pi, any);
          done = false;
          rEnd = walk.base;
          if (!any) break;
        }
        __builtin_amdgcn_wave_barrier();  // the records are consumed before the next chunk overwrites them
      }
    }
    // the waves add their register stencils into the block's force arena one after the other: in phase (a, b, c) lane (cx, cy, cz)
    // owns node (cx + a, cy + b, cz + c) of its bin -- 64 distinct nodes
    float *a0 = farena + AL::at(geo.o[0] + cx, geo.o[1] + cy, geo.o[2] + cz);
#pragma unroll 1
    for (int turn = 0; turn < NW; ++turn) {
      if (turn == w && start != end) {
#pragma unroll
        for (int k = 0; k < 27; ++k) {
          float *g = a0 + AL::at(k / 9, (k / 3) % 3, k % 3);
#pragma unroll
          for (int j = 0; j < 3; ++j) g[j * AL::CH] += acc[k][j];
          __builtin_amdgcn_wave_barrier();
        }
      }
      __syncthreads();
    }
  }
  // flush: once per node of the block's arena
  for (int node = threadIdx.x; node < W * W * W; node += NT) {
    const int x = node / (W * W), y = (node / W) % W, z = node % W;
    const int slot = ((x >= SIDE) << 2) | ((y >= SIDE) << 1) | (z >= SIDE);
    const int cell = ((x & (SIDE - 1)) * SIDE + (y & (SIDE - 1))) * SIDE + (z & (SIDE - 1));
    const int bn = nbr[(size_t)blk * 8 + slot];
    if (bn < 0) continue;
    const int a = AL::at(x, y, z);
    float *g = fOut + 3 * ((size_t)bn * NC + cell);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v = farena[a + ch * AL::CH];
      if (v != 0.f) unsafeAtomicAdd(g + ch, v);
    }
  }
}

}  // namespace zsr
