#pragma once
// mpm_fused_kernels.hpp -- kernels of the fused G2P2G step on compact (binned) storage; included by mpm_fused_impl.hpp only
#include "mpm_arena.hpp"
#include "mpm_fused_common.hpp"

namespace zsr {

// ======================================================================================= G2P2G (fused)
// G2P of step n and P2G of step n+1 in ONE pass over the particles (the reference has the same idea as G2P2GTransfer,
// simulation/transfer/G2P2G.hpp): a particle is read once (m, x, F, logJp: 56 B), gathered from grid A, advected, its F and
// constitutive model updated, and scattered straight into grid B; only x, F, logJp go back to HBM (52 B).  v, C and
// P F^T vol never leave the chip (WRITE_ALL stores them for callers that want the full state).  Unfused, the same work
// moves 296.5 B per particle and step.
//
// g2p2g_reorder_kernel, the kernel of the re-ordering step (the in-place step runs the role-split g2p2g_rs_kernel further down):
// one workgroup of four waves owns a bin; lane = cell.  Per chunk of four rounds:
//   phase 1   wave w runs round 4c + w through G2P (node velocities read from the LDS arena) + F update + constitutive model
//             and stages {m, x', v', C', P F^T} of its 64 particles in LDS;
//   phase 2   waves 0/1 accumulate mass + momentum (4 channels, 108 register accumulators) of staged rounds {0,1} / {2,3},
//             waves 2/3 the three stress channels of the same rounds; two LDS arenas collect the two halves.
// The kernel is VALU-bound (SQ_INSTS_VALU x 4 cycles ~ 85 % of the SIMD cycles), so the design minimises instructions: the
// first version kept the 81 node velocities in registers and gave each of the four waves one channel role in
// phase 2 (each staged round consumed by 4 waves: 4x the arena / weight work) and took 5.0 ms per 67.1 M-particle step.
// Particles that are not in the cell they are stored under are exact as before: mis-binned at read -> queue G (global
// gather + global scatter afterwards); moved out of the cell by this step's advection -> queue P (state stored, global
// scatter afterwards).
constexpr int G2P2G_NF = 25;       // staged floats per particle: m, x(3), v(3), C(9), P F^T vol(9)
constexpr int G2P2G_MQ_CAP = 512;  // in-bin movers a workgroup can take through its LDS queue (a bin holds ~512 particles)

// phase-2 consumer of one staged record.  STRESS = false: mass + momentum (4 channels), true: rhs (3 channels)
template <bool STRESS>
__device__ __forceinline__ void g2p2g_consume(const MpmDev &mp, const float *st, int lane, float kscale, float (&acc)[27][STRESS ? 3 : 4]) {
  auto f = [&](int k) { return st[k * 64 + lane]; };
  const float pos[3] = {f(1), f(2), f(3)};
  Arena ar;
  make_arena(mp.dx, mp.dxi, pos, ar);
  float xo[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) xo[d][k] = (float)k * mp.dx - ar.lp[d];
  float Px[3][3], Py[3][3], Pz[3][3], wzs[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float c0 = STRESS ? f(16 + d) : f(7 + d), c1 = STRESS ? f(19 + d) : f(10 + d), c2 = STRESS ? f(22 + d) : f(13 + d);
    const float v = STRESS ? 0.f : f(4 + d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Px[k][d] = c0 * xo[0][k];
      Py[k][d] = c1 * xo[1][k];
      Pz[k][d] = STRESS ? c2 * xo[2][k] : fmaf(c2, xo[2][k], v);
    }
  }
  const float scale = STRESS ? kscale : f(0);
#pragma unroll
  for (int k = 0; k < 3; ++k) wzs[k] = ar.w[2][k] * scale;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      const float wxy = ar.w[0][a] * ar.w[1][bb];
      const float q0 = Px[a][0] + Py[bb][0], q1 = Px[a][1] + Py[bb][1], q2 = Px[a][2] + Py[bb][2];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float Ws = wxy * wzs[c];
        auto &A = acc[(a * 3 + bb) * 3 + c];
        if constexpr (!STRESS) {
          A[0] += Ws;
          A[1] = fmaf(Ws, q0 + Pz[c][0], A[1]);
          A[2] = fmaf(Ws, q1 + Pz[c][1], A[2]);
          A[3] = fmaf(Ws, q2 + Pz[c][2], A[3]);
        } else {
          A[0] = fmaf(Ws, q0 + Pz[c][0], A[0]);
          A[1] = fmaf(Ws, q1 + Pz[c][1], A[1]);
          A[2] = fmaf(Ws, q2 + Pz[c][2], A[2]);
        }
      }
    }
}

// W = wave index: phase 1 handles round 4c + W; phase 2 role: waves 0/1 take mass + momentum of staged rounds {0,1} / {2,3},
// waves 2/3 the stress channels of rounds {0,1} / {2,3}; waves 0,2 accumulate into arena 0, waves 1,3 into arena 1
template <int SIDE, int SMODEL, int LW, int W>
__device__ __forceinline__ void g2p2g_body(const MpmDev &mp, const ParticlesDev &ps, const BinGeom<SIDE> &geo, int start, unsigned cnt,
                                           int lane, const float *varena, float *parena, float *stage, unsigned long long *smask,
                                           int *staleG, int *staleGCount, int *staleP, int *stalePCount, int *mq, int *mqCount,
                                           const int *order, long long inDelta) {
  using AL = ArenaLds;
  constexpr bool DP = model_uses_logjp(SMODEL);
  constexpr bool STRESS = W >= 2;
  constexpr int NCH = STRESS ? 3 : 4;
  constexpr int R0 = (W & 1) * 2;  // first of this wave's two staged rounds in phase 2
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  const float dxi = mp.dxi;
  const float D_inv = mp.D_inv;
  const float kscale = mp.fscale;
  const float *v0 = varena + AL::at(cx, cy, cz);
  float acc[27][NCH];
#pragma unroll
  for (int k = 0; k < 27; ++k)
#pragma unroll
    for (int q = 0; q < NCH; ++q) acc[k][q] = 0.f;
  RoundWalk walk(cnt, start);
  auto next_chunk = [&](int &idx, bool &has, bool &any) {
    any = false;
    has = false;
    idx = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i;
      bool a;
      const bool h = walk.next(i, a);
      if (r == 0) any = a;
      if (r == W) {
        idx = i;
        has = h;
      }
    }
  };
  int i0, i1;
  bool has0, has1, any, any1;
  next_chunk(i0, has0, any);
  RecG<LW, DP, model_is_fluid(SMODEL)> cur, nxt;
  // slot i of the (new) binned order holds the particle stored at order[i] of the input buffer; everything this kernel stores goes
  // to slot i of the output buffer, so the physical re-bin costs no pass of its own
  if (has0) cur.load(ps, (size_t)order[i0], inDelta);
  int par = 0;  // stage / mask buffer of this chunk (double buffered: ONE barrier per chunk)
  while (any) {
    float *myStage = stage + (size_t)(par * 4 + W) * (G2P2G_NF * 64);
    next_chunk(i1, has1, any1);
    if (has1) nxt.load(ps, (size_t)order[i1], inDelta);  // in flight during this chunk
    // ---------------- phase 1: G2P + update of this wave's round
    bool valid = false;
    if (has0) {
      Arena ar;
      make_arena(mp.dx, mp.dxi, cur.pos, ar);
      // the particle's cell relative to the bin.  Anywhere inside the bin the node velocities are in the LDS arena, so a
      // particle that has wandered into a neighbouring cell of the same bin is still gathered here; only one that is outside
      // the bin altogether takes the exact path (hash queries into grid A)
      const int ocx = ar.corner[0] - geo.org[0], ocy = ar.corner[1] - geo.org[1], ocz = ar.corner[2] - geo.org[2];
      if ((unsigned)ocx >= 4u || (unsigned)ocy >= 4u || (unsigned)ocz >= 4u) {
        {  // the exact path works on slot i0 of the output buffer: give it the inputs
          const POff<LW> oo = particle_offset<LW>(ps.pos.chns, (size_t)i0);
          pstore<LW, 3>(ps.pos, oo, cur.pos);
          pstore_state<LW, model_is_fluid(SMODEL)>(ps.F, oo, cur.F);
          pstore1<LW>(ps.mass, oo, cur.m);
          if constexpr (DP) pstore1<LW>(ps.logJp, oo, cur.logJp);
        }
        staleG[atomicAdd(staleGCount, 1)] = i0;  // outside the bin: exact gather + scatter afterwards
        // drift guard of the split launch: the exact path of an interior block may only reach blocks within two of its own
        if ((unsigned)(ocx + 4) >= 12u || (unsigned)(ocy + 4) >= 12u || (unsigned)(ocz + 4) >= 12u) staleGCount[8] = 1;
      } else {
        float vel[3], C[9];
        g2p_gather_lds<AL>(mp, ar, varena + AL::at(ocx, ocy, ocz), D_inv, vel, C);
        const POff<LW> o = particle_offset<LW>(ps.pos.chns, (size_t)i0);
        float pos[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) pos[d] = cur.pos[d] + vel[d] * mp.dt;
        float F[9], PF[9];
        advance_state<model_is_fluid(SMODEL)>(cur.F, C, mp.dt, F);
        pstore_state<LW, model_is_fluid(SMODEL)>(ps.F, o, F);
        pstore<LW, 3>(ps.pos, o, pos);
        pstore1<LW>(ps.mass, o, cur.m);  // the mass moves with the particle
        {  // F has been stored above: the plastic models may project this local copy
          float lj = 0.f;
          if constexpr (DP) lj = cur.logJp;
          model_stress<SMODEL>(mp.mat, lj, F, PF, C);
          if constexpr (DP) pstore1<LW>(ps.logJp, o, lj);
        }
        // where is it now?  same cell as this lane: register accumulation (phase 2).  Another cell of the same bin: queued in
        // LDS and scattered into the bin's arena by the dense post-pass of the kernel.  Outside the bin: exact path.
        const int ncx = (int)floorf(pos[0] * dxi - 0.5f) - geo.org[0], ncy = (int)floorf(pos[1] * dxi - 0.5f) - geo.org[1],
                  ncz = (int)floorf(pos[2] * dxi - 0.5f) - geo.org[2];
        const bool moved = ncx != cx || ncy != cy || ncz != cz;
        if (moved) {
          pstore<LW, 3>(ps.vel, o, vel);
          pstore<LW, 9>(ps.C, o, C);
          {
            float S[STRESS_N];
            stress_pack(PF, S);
            pstore<LW, STRESS_N>(ps.stress, o, S);
          }
          bool queued = false;
          if ((unsigned)ncx < 4u && (unsigned)ncy < 4u && (unsigned)ncz < 4u) {
            const int slot = atomicAdd(mqCount, 1);
            if (slot < G2P2G_MQ_CAP) {
              mq[slot] = i0;
              queued = true;
            }
          }
          if (!queued) {
            staleP[atomicAdd(stalePCount, 1)] = i0;  // left the bin during this step: exact scatter afterwards
            if ((unsigned)(ncx + 4) >= 12u || (unsigned)(ncy + 4) >= 12u || (unsigned)(ncz + 4) >= 12u) staleGCount[8] = 1;
          }
        } else {
          valid = true;
          myStage[0 * 64 + lane] = cur.m;
#pragma unroll
          for (int d = 0; d < 3; ++d) myStage[(1 + d) * 64 + lane] = pos[d];
#pragma unroll
          for (int d = 0; d < 3; ++d) myStage[(4 + d) * 64 + lane] = vel[d];
#pragma unroll
          for (int d = 0; d < 9; ++d) myStage[(7 + d) * 64 + lane] = C[d];
#pragma unroll
          for (int d = 0; d < 9; ++d) myStage[(16 + d) * 64 + lane] = PF[d];
        }
      }
    }
    {
      const unsigned long long vm = __ballot(valid);
      if (lane == 0) smask[par * 4 + W] = vm;
    }
    __syncthreads();  // this chunk is staged; everybody has finished consuming the chunk before the previous one
    // ---------------- phase 2: two staged rounds per wave, 4 (mass + momentum) or 3 (stress) channels
#pragma unroll 1
    for (int rr = R0; rr < R0 + 2; ++rr) {
      const unsigned long long vm = smask[par * 4 + rr];
      if (vm == 0ull) continue;
      if ((vm >> lane) & 1ull) g2p2g_consume<STRESS>(mp, stage + (size_t)(par * 4 + rr) * (G2P2G_NF * 64), lane, kscale, acc);
    }
    par ^= 1;
    cur = nxt;
    has0 = has1;
    i0 = i1;
    any = any1;
  }
  // every wave owns its (arena, channel set): waves 0/2 write arena 0 (channels 0-3 / 4-6), waves 1/3 arena 1
  acc_to_arena<AL>(parena + (size_t)(W & 1) * (7 * AL::CH) + (STRESS ? 4 : 0) * AL::CH + AL::at(cx, cy, cz), acc);
  __syncthreads();  // the post-pass and the flush read both arenas
}

template <int SIDE, int SMODEL, int LW>
static __global__ __launch_bounds__(256) void g2p2g_reorder_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, const float *gridA, float *gridB,
                                                            const int *binStart, const unsigned *cellCount, const int *nbr, int *staleG,
                                                            int *staleGCount, int *staleP, int *stalePCount, int binBase,
                                                            const int *order, long long inDelta) {
  using AL = ArenaLds;
  constexpr int NC = SIDE * SIDE * SIDE;
  __shared__ float varena[3 * AL::CH];
  __shared__ float parena[2 * 7 * AL::CH];
  __shared__ float stage[2 * 4 * G2P2G_NF * 64];
  __shared__ unsigned long long smask[2 * 4];
  __shared__ int mq[G2P2G_MQ_CAP];
  __shared__ int mqCount;
  if (threadIdx.x == 0) mqCount = 0;
  const int bin = (int)blockIdx.x + binBase;  // a launch covers a range of blocks (boundary blocks first, see zs_rocm_mpm_g2p2g_range)
  const int start = binStart[bin], end = binStart[bin + 1];
  if (start == end) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const BinGeom<SIDE> geo(t, bin, mp.kscale);
  // (The gather below and the flush at the end are spelled out in the two compact kernels although mpm_arena.hpp has them as
  // arena_gather_velocities / arena_flush_to_grid for the slotted step, and so is the in-bin-mover pass, which has no shared form: as calls
  // of a common function each of the three changes these kernels' SGPR spill counts -- profiles/fused_dedupe.md.)
  if (tid < 216) {  // node decoded once for the 3 velocity channels
    const int x = tid / 36, y = (tid / 6) % 6, z = tid % 6;
    int slot, cell;
    arena_to_grid<SIDE>(geo.o, x, y, z, slot, cell);
    const int bn = nbr[(size_t)geo.block * 8 + slot];
    float *a = varena + AL::at(x, y, z);
    const float *g = gridA + ((size_t)(bn < 0 ? 0 : bn) * 7 + 1) * NC + cell;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) a[ch * AL::CH] = bn >= 0 ? g[ch * NC] : 0.f;
  }
  for (int k = tid; k < 2 * 7 * AL::CH; k += 256) parena[k] = 0.f;
  const unsigned cnt = cellCount[(size_t)bin * 64 + lane];
  __syncthreads();
  if (w == 0) g2p2g_body<SIDE, SMODEL, LW, 0>(mp, ps, geo, start, cnt, lane, varena, parena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, order, inDelta);
  else if (w == 1) g2p2g_body<SIDE, SMODEL, LW, 1>(mp, ps, geo, start, cnt, lane, varena, parena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, order, inDelta);
  else if (w == 2) g2p2g_body<SIDE, SMODEL, LW, 2>(mp, ps, geo, start, cnt, lane, varena, parena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, order, inDelta);
  else g2p2g_body<SIDE, SMODEL, LW, 3>(mp, ps, geo, start, cnt, lane, varena, parena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, order, inDelta);
  // dense post-pass over the particles that changed cell inside this bin: one thread per particle, contributions added to the
  // bin's arena with LDS atomics (the register stencils of the lanes are keyed to cells).  Their state was stored by other
  // lanes of this workgroup a moment ago: read it at agent scope so that a stale L1 line (x was loaded in phase 1) cannot serve it.
  // (Measured alternative: records parked in LDS and walked one by one with lane = node and plain read-add-write per wave-owned
  // channel -- no atomics, but a serial, latency-bound walk: 20 % slower on the 200-step free fall.)
  {
    // The queued particles' state was stored by OTHER waves of this workgroup during the loop, with plain stores; the reads below are
    // agent-scope loads.  A barrier orders instructions, not the arrival of stores at L2 (outside threadgroup-split mode a workgroup-scope
    // release does not wait for vmcnt), so every wave drains its stores and the workgroup meets once more before the post-pass reads.
    // (Added while hunting the rare deviation of the 24-step test; that turned out to be something else -- profiles/r03_compact_outliers.md --
    // but the ordering is not guaranteed without it.)
    if (mqCount > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    const int nm = mqCount < G2P2G_MQ_CAP ? mqCount : G2P2G_MQ_CAP;  // the body ended with a barrier
    const float dxi = mp.dxi;
    const float kscale = mp.fscale;
    for (int q = tid; q < nm; q += 256) {
      const size_t i = (size_t)mq[q];
      auto cload = [&](const Port<float> &p, int comp) {
        return __hip_atomic_load(p.base + p.off(i) + (size_t)comp * p.cstride(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      };
      const float m = ps.mass.base[ps.mass.off(i)];
      float pos[3], vel[3], C[9], PF[9];
#pragma unroll
      for (int d = 0; d < 3; ++d) { pos[d] = cload(ps.pos, d); vel[d] = cload(ps.vel, d); }
#pragma unroll
      for (int d = 0; d < 9; ++d) C[d] = cload(ps.C, d);
      {
        float S[STRESS_N];
#pragma unroll
        for (int d = 0; d < STRESS_N; ++d) S[d] = cload(ps.stress, d) * kscale;
        stress_unpack(S, PF);
      }
      Arena ar;
      make_arena(mp.dx, mp.dxi, pos, ar);
      const int kx = ar.corner[0] - geo.org[0], ky = ar.corner[1] - geo.org[1], kz = ar.corner[2] - geo.org[2];
      if ((unsigned)kx >= 4u || (unsigned)ky >= 4u || (unsigned)kz >= 4u) {
        // the queueing test rounds pos * (1/dx) - 0.5 in one step, make_arena in two: on an exact cell face they can disagree
        staleP[atomicAdd(stalePCount, 1)] = (int)i;
        continue;
      }
      float *a0 = parena + AL::at(kx, ky, kz);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float W = ar.w[0][a] * ar.w[1][b] * ar.w[2][c];
            const float x0 = (float)a * mp.dx - ar.lp[0], x1 = (float)b * mp.dx - ar.lp[1], x2 = (float)c * mp.dx - ar.lp[2];
            float *g = a0 + AL::at(a, b, c);
            atomicAdd(g, W * m);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              atomicAdd(g + (1 + d) * AL::CH, W * m * (vel[d] + (C[d] * x0 + C[3 + d] * x1 + C[6 + d] * x2)));
              atomicAdd(g + (4 + d) * AL::CH, (PF[d] * x0 + PF[3 + d] * x1 + PF[6 + d] * x2) * W);
            }
          }
    }
    __syncthreads();
  }
  if (tid < 216) {
    const int x = tid / 36, y = (tid / 6) % 6, z = tid % 6;
    int slot, cell;
    arena_to_grid<SIDE>(geo.o, x, y, z, slot, cell);
    const int bn = nbr[(size_t)geo.block * 8 + slot];
    const float *a = parena + AL::at(x, y, z);
    if (bn >= 0) {
      float *g = gridB + (size_t)bn * 7 * NC + cell;
#pragma unroll
      for (int ch = 0; ch < 7; ++ch) {
        const float v = a[ch * AL::CH] + a[(7 + ch) * AL::CH];
        if (v != 0.f) unsafeAtomicAdd(g + ch * NC, v);
      }
    }
    else if (a[0] + a[7 * AL::CH] != 0.f) {
      staleGCount[9] = 1;  // mass for a node whose block is not in the partition: the partition no longer covers the particles
    }
  }
}
// ---------------------------------------------------------------------------------------------------------------------------
// Role-split variant of the fused pass (the default; the four-wave g2p2g_reorder_kernel above stays for the re-ordering step).
// Measured on the four-wave kernel (64 Mi particles): the costs of its parts
// ADD UP instead of overlapping -- constitutive update 1.0 ms + phase-2 accumulation 0.9 + gather 0.5 + streaming skeleton 2.2
// + head/tail of a bin 0.45 = 5.0 ms -- because at 223 VGPRs / 74.5 KB LDS only two waves share a SIMD, each of them parked 37 %
// of its life (SQ_WAIT_ANY), and one wave alone issues a VALU instruction only every ~5 cycles.  The accumulators (27 nodes x 7
// channels per cell) are what costs the registers, so they move to waves of their own:
//   waves 0-3  PRODUCERS  round 4c + w of chunk c: G2P from the LDS velocity arena, advection, F update, constitutive model,
//                         stores, {m, x', v', C', P F^T} staged in LDS -- no accumulators: < 128 VGPRs
//   waves 4-7  CONSUMERS  of the chunk staged one iteration earlier: each owns a channel set {m, mv_x} {mv_y, mv_z} {f_x, f_y}
//                         {f_z} of ALL four staged rounds: 54 accumulators, < 128 VGPRs; each channel of the bin's single LDS
//                         arena belongs to one wave, so the final flush needs no barrier between its 27 phases
// One barrier per chunk (stage double-buffered), 512 threads, 66 KB LDS: two workgroups = 16 waves per CU = 4 per SIMD.  The
// per-record arena / weight set-up is repeated by four consumers instead of two (+190 VALU per 64 particles, +9 %).
template <int CS>
__device__ __forceinline__ void g2p2g_rs_consumer(const MpmDev &mp, int lane, int nchunks, const float *stage, const unsigned long long *smask,
                                                  float *parena) {
  using S = ConsumerSet<CS>;
  using AL = ArenaLds;
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  const float dxi = mp.dxi;
  const float kscale = mp.fscale;
  float acc[27][S::NA];
#pragma unroll
  for (int k = 0; k < 27; ++k)
#pragma unroll
    for (int q = 0; q < S::NA; ++q) acc[k][q] = 0.f;
  for (int k = (int)threadIdx.x - 256; k < 7 * AL::CH; k += 256) parena[k] = 0.f;  // the four consumer waves clear the bin's arena
  __syncthreads();  // (the producers fill the velocity arena meanwhile)
  for (int it = 0; it <= nchunks; ++it) {
    if (it > 0) {
      const int par = (it - 1) & 1;
#pragma unroll 1
      for (int rr = 0; rr < 4; ++rr) {
        const unsigned long long vm = smask[par * 4 + rr];
        if (vm == 0ull) continue;
        if ((vm >> lane) & 1ull) g2p2g_consume_set<CS>(mp, stage + (size_t)(par * 4 + rr) * (G2P2G_QF * 64), lane, acc);
      }
    }
    __syncthreads();
  }
  acc_to_arena<AL>(parena + (size_t)S::CH0 * AL::CH + AL::at(cx, cy, cz), acc);  // the set's channels of the bin's arena belong to this wave alone
}
// producer wave W (0..3): round 4c + W of every chunk c
template <int SIDE, int SMODEL, int LW, bool WRITE_ALL, int W>
__device__ __forceinline__ void g2p2g_rs_producer(const MpmDev &mp, const ParticlesDev &ps, const BinGeom<SIDE> &geo, int start, unsigned cnt,
                                                  int lane, int nchunks, float *varena, float *stage, unsigned long long *smask,
                                                  int *staleG, int *staleGCount, int *staleP, int *stalePCount, int *mq, int *mqCount,
                                                  const float *gridA, const int *nbr) {
  using AL = ArenaLds;
  constexpr bool DP = model_uses_logjp(SMODEL);
  constexpr bool FLUID = model_is_fluid(SMODEL);
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  const float dxi = mp.dxi;
  const float D_inv = mp.D_inv;
  RoundWalk walk(cnt, start);
  auto next_chunk = [&](int &idx, bool &has) {
    has = false;
    idx = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int i;
      bool a;
      const bool h = walk.next(i, a);
      if (r == W) {
        idx = i;
        has = h;
      }
    }
  };
  int i0 = 0, i1 = 0;
  bool has0 = false, has1 = false;
  RecG<LW, DP, FLUID> cur, nxt;
  // head of the bin: the first records are requested BEFORE the velocity arena is filled -- both need only what the bin number
  // gives (binStart / cellCount / block key / nbr row arrive together), so a bin starts after two memory round trips, not four
  // (requested into `nxt` and handed over at the top of the iteration that uses it: see g2p2g_slot_producer)
  if (nchunks > 0) {
    next_chunk(i1, has1);
    if (has1) nxt.load(ps, (size_t)i1);
  }
  {
    constexpr int NC = SIDE * SIDE * SIDE;
    const int tid = (int)threadIdx.x;  // the four producer waves are threads 0..255
    if (tid < 216) {  // node decoded once for the 3 velocity channels
      const int x = tid / 36, y = (tid / 6) % 6, z = tid % 6;
      int slot, cell;
      arena_to_grid<SIDE>(geo.o, x, y, z, slot, cell);
      const int bn = nbr[(size_t)geo.block * 8 + slot];
      float *a = varena + AL::at(x, y, z);
      const float *g = gridA + ((size_t)(bn < 0 ? 0 : bn) * 7 + 1) * NC + cell;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) a[ch * AL::CH] = bn >= 0 ? g[ch * NC] : 0.f;
    }
  }
  __syncthreads();
  for (int it = 0; it <= nchunks; ++it) {
    if (it < nchunks) {
      const int par = it & 1;
      float *myStage = stage + (size_t)(par * 4 + W) * (G2P2G_QF * 64);
      cur = nxt;
      has0 = has1;
      i0 = i1;
      has1 = false;
      if (it + 1 < nchunks) {
        next_chunk(i1, has1);
        if (has1) nxt.load(ps, (size_t)i1);  // in flight during this chunk
      }
      bool valid = false;
      if (has0) {
        Arena ar;
        make_arena(mp.dx, mp.dxi, cur.pos, ar);
        const int ocx = ar.corner[0] - geo.org[0], ocy = ar.corner[1] - geo.org[1], ocz = ar.corner[2] - geo.org[2];
        if ((unsigned)ocx >= 4u || (unsigned)ocy >= 4u || (unsigned)ocz >= 4u) {
          staleG[atomicAdd(staleGCount, 1)] = i0;  // outside the bin: exact gather + scatter afterwards
          if ((unsigned)(ocx + 4) >= 12u || (unsigned)(ocy + 4) >= 12u || (unsigned)(ocz + 4) >= 12u) staleGCount[8] = 1;
        } else {
          float vel[3], C[9];
          g2p_gather_lds<AL>(mp, ar, varena + AL::at(ocx, ocy, ocz), D_inv, vel, C);
          const POff<LW> o = particle_offset<LW>(ps.pos.chns, (size_t)i0);
          float pos[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) pos[d] = cur.pos[d] + vel[d] * mp.dt;
          float F[9], PF[9];
          advance_state<FLUID>(cur.F, C, mp.dt, F);
          pstore_state<LW, FLUID>(ps.F, o, F);
          pstore<LW, 3>(ps.pos, o, pos);
          {  // F has been stored above: the plastic models may project this local copy
            float lj = 0.f;
            if constexpr (DP) lj = cur.logJp;
            model_stress<SMODEL>(mp.mat, lj, F, PF, C);
            if constexpr (DP) pstore1<LW>(ps.logJp, o, lj);
          }
          // base node and normalised local position of the NEW position, exactly as make_arena derives them
          float lpn[3];
          int nc[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const float X = pos[d] * dxi;
            const float fl = floorf(X - 0.5f);
            nc[d] = (int)fl - geo.org[d];
            lpn[d] = X - fl;
          }
          const int ncx = nc[0], ncy = nc[1], ncz = nc[2];
          // The reference derives the weights from localPos - base_node(localPos) (InterpolationKernel.hpp:108) although localPos is already
          // relative to the base node (simulation/Utils.hpp:59-60).  The second base_node is 0 -- except when X - floor(X - 0.5) ROUNDS up to
          // 1.5, or X - 0.5 rounds up to an integer and leaves it just below 0.5 (only possible for |X| < 1, next to the coordinate origin):
          // then it is +-1 and the weights are those of d0 -+ 1 on the unchanged corner.  make_arena restates that; the consumers take the
          // staged lpn as d0 without the second floor, so such a particle goes the way of the in-bin movers (post-pass, make_arena) instead.
          // profiles/r03_compact_outliers.md
          const bool moved = ncx != cx || ncy != cy || ncz != cz ||
                             !(lpn[0] >= 0.5f && lpn[0] < 1.5f && lpn[1] >= 0.5f && lpn[1] < 1.5f && lpn[2] >= 0.5f && lpn[2] < 1.5f);
          if (WRITE_ALL || moved) {
            pstore<LW, 3>(ps.vel, o, vel);
            pstore<LW, 9>(ps.C, o, C);
            {
            float S[STRESS_N];
            stress_pack(PF, S);
            pstore<LW, STRESS_N>(ps.stress, o, S);
          }
          }
          if (moved) {
            bool queued = false;
            if ((unsigned)ncx < 4u && (unsigned)ncy < 4u && (unsigned)ncz < 4u) {
              const int slot = atomicAdd(mqCount, 1);
              if (slot < G2P2G_MQ_CAP) {
                mq[slot] = i0;
                queued = true;
              }
            }
            if (!queued) {
              staleP[atomicAdd(stalePCount, 1)] = i0;  // left the bin during this step: exact scatter afterwards
              if ((unsigned)(ncx + 4) >= 12u || (unsigned)(ncy + 4) >= 12u || (unsigned)(ncz + 4) >= 12u) staleGCount[8] = 1;
            }
          } else {
            valid = true;
            stage_qform(mp, myStage + lane, cur.m, lpn, vel, C, PF);
          }
        }
      }
      {
        const unsigned long long vm = __ballot(valid);
        if (lane == 0) smask[par * 4 + W] = vm;
      }
    }
    __syncthreads();
  }
}

template <int SIDE, int SMODEL, int LW, bool WRITE_ALL>
static __global__ __launch_bounds__(512, 4) void g2p2g_rs_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, const float *gridA, float *gridB,
                                                          const int *binStart, const unsigned *cellCount, const int *nbr, int *staleG,
                                                          int *staleGCount, int *staleP, int *stalePCount, int binBase) {
  using AL = ArenaLds;
  constexpr int NC = SIDE * SIDE * SIDE;
  __shared__ float varena[3 * AL::CH];
  __shared__ float parena[7 * AL::CH];
  __shared__ float stage[2 * 4 * G2P2G_QF * 64];
  __shared__ unsigned long long smask[2 * 4];
  __shared__ int mq[G2P2G_MQ_CAP];
  __shared__ int mqCount;
  if (threadIdx.x == 0) mqCount = 0;
  const int bin = (int)blockIdx.x + binBase;
  const int start = binStart[bin], end = binStart[bin + 1];
  if (start == end) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const BinGeom<SIDE> geo(t, bin, mp.kscale);
  const unsigned cnt = cellCount[(size_t)bin * 64 + lane];
  // rounds of this bin = the fullest cell; every wave needs the number of chunks (uniform loop with one barrier per chunk)
  unsigned mx = cnt;
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)mx, sft, 64);
    mx = o > mx ? o : mx;
  }
  const int nchunks = (int)((mx + 3u) >> 2);
  if (w == 0) g2p2g_rs_producer<SIDE, SMODEL, LW, WRITE_ALL, 0>(mp, ps, geo, start, cnt, lane, nchunks, varena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, gridA, nbr);
  else if (w == 1) g2p2g_rs_producer<SIDE, SMODEL, LW, WRITE_ALL, 1>(mp, ps, geo, start, cnt, lane, nchunks, varena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, gridA, nbr);
  else if (w == 2) g2p2g_rs_producer<SIDE, SMODEL, LW, WRITE_ALL, 2>(mp, ps, geo, start, cnt, lane, nchunks, varena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, gridA, nbr);
  else if (w == 3) g2p2g_rs_producer<SIDE, SMODEL, LW, WRITE_ALL, 3>(mp, ps, geo, start, cnt, lane, nchunks, varena, stage, smask, staleG, staleGCount, staleP, stalePCount, mq, &mqCount, gridA, nbr);
  else if (w == 4) g2p2g_rs_consumer<0>(mp, lane, nchunks, stage, smask, parena);
  else if (w == 5) g2p2g_rs_consumer<1>(mp, lane, nchunks, stage, smask, parena);
  else if (w == 6) g2p2g_rs_consumer<2>(mp, lane, nchunks, stage, smask, parena);
  else g2p2g_rs_consumer<3>(mp, lane, nchunks, stage, smask, parena);
  __syncthreads();  // all channel sets are in the arena
  // in-bin movers: dense post-pass with LDS atomics (see g2p2g_reorder_kernel)
  {
    // The queued particles' state was stored by OTHER waves of this workgroup during the loop, with plain stores; the reads below are
    // agent-scope loads.  A barrier orders instructions, not the arrival of stores at L2 (outside threadgroup-split mode a workgroup-scope
    // release does not wait for vmcnt), so every wave drains its stores and the workgroup meets once more before the post-pass reads.
    // (Added while hunting the rare deviation of the 24-step test; that turned out to be something else -- profiles/r03_compact_outliers.md --
    // but the ordering is not guaranteed without it.)
    if (mqCount > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    const int nm = mqCount < G2P2G_MQ_CAP ? mqCount : G2P2G_MQ_CAP;
    const float dxi = mp.dxi;
    const float kscale = mp.fscale;
    for (int q = tid; q < nm; q += 512) {
      const size_t i = (size_t)mq[q];
      auto cload = [&](const Port<float> &p, int comp) {
        return __hip_atomic_load(p.base + p.off(i) + (size_t)comp * p.cstride(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      };
      const float m = ps.mass.base[ps.mass.off(i)];
      float pos[3], vel[3], C[9], PF[9];
#pragma unroll
      for (int d = 0; d < 3; ++d) { pos[d] = cload(ps.pos, d); vel[d] = cload(ps.vel, d); }
#pragma unroll
      for (int d = 0; d < 9; ++d) C[d] = cload(ps.C, d);
      {
        float S[STRESS_N];
#pragma unroll
        for (int d = 0; d < STRESS_N; ++d) S[d] = cload(ps.stress, d) * kscale;
        stress_unpack(S, PF);
      }
      Arena ar;
      make_arena(mp.dx, mp.dxi, pos, ar);
      const int kx = ar.corner[0] - geo.org[0], ky = ar.corner[1] - geo.org[1], kz = ar.corner[2] - geo.org[2];
      if ((unsigned)kx >= 4u || (unsigned)ky >= 4u || (unsigned)kz >= 4u) {
        staleP[atomicAdd(stalePCount, 1)] = (int)i;
        continue;
      }
      float *a0 = parena + AL::at(kx, ky, kz);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float W = ar.w[0][a] * ar.w[1][b] * ar.w[2][c];
            const float x0 = (float)a * mp.dx - ar.lp[0], x1 = (float)b * mp.dx - ar.lp[1], x2 = (float)c * mp.dx - ar.lp[2];
            float *g = a0 + AL::at(a, b, c);
            atomicAdd(g, W * m);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              atomicAdd(g + (1 + d) * AL::CH, W * m * (vel[d] + (C[d] * x0 + C[3 + d] * x1 + C[6 + d] * x2)));
              atomicAdd(g + (4 + d) * AL::CH, (PF[d] * x0 + PF[3 + d] * x1 + PF[6 + d] * x2) * W);
            }
          }
    }
    __syncthreads();
  }
  if (tid < 216) {
    const int x = tid / 36, y = (tid / 6) % 6, z = tid % 6;
    int slot, cell;
    arena_to_grid<SIDE>(geo.o, x, y, z, slot, cell);
    const int bn = nbr[(size_t)geo.block * 8 + slot];
    const float *a = parena + AL::at(x, y, z);
    if (bn >= 0) {
      float *g = gridB + (size_t)bn * 7 * NC + cell;
#pragma unroll
      for (int ch = 0; ch < 7; ++ch) {
        const float v = a[ch * AL::CH];
        if (v != 0.f) unsafeAtomicAdd(g + ch * NC, v);
      }
    } else if (a[0] != 0.f) {
      staleGCount[9] = 1;  // mass for a node whose block is not in the partition
    }
  }
}
// queue G: gather from grid A with hash queries (stores the full state), then scatter to grid B; queue P: scatter only
template <int SIDE, int SMODEL>
static __global__ __launch_bounds__(256) void g2p2g_stale_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, const float *gridA, float *gridB,
                                                          const int *staleG, const int *staleGCount, const int *staleP,
                                                          const int *stalePCount, int *driftFlag) {
  const int ng = *staleGCount, np = *stalePCount;
  if (driftFlag && blockIdx.x == 0 && threadIdx.x == 0) {  // status words for the host: [0] drift flag, [1] exact-path particles
    if (staleGCount[8]) driftFlag[0] = 1;
    atomicAdd(&driftFlag[1], ng + np);
    if (staleGCount[9]) driftFlag[2] = 1;
  }
  const float dxi = mp.dxi;
  const float D_inv = mp.D_inv;
  // queue G only: exact gather + update; the scatter of both queues follows in stale_scatter_coop_kernel
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < ng; j += gridDim.x * blockDim.x)
    g2p_gather_global<SIDE, SMODEL>(mp, ps, (size_t)staleG[j], t, gridA, D_inv);
}

// Exact scatter of the queued particles, 32 lanes per particle: lane = stencil node (27 active).  The 8 candidate blocks are
// queried by lanes 0-7 at once, and the three z-neighbours of a node row sit in one 128-B line of the channel, so one atomic
// instruction of a half-wave touches 9 lines instead of the 27 (x 64 particles) of the thread-per-particle form.  Values and
// order of additions per node are those of p2g_scatter_global.
template <int SIDE>
static __global__ __launch_bounds__(256) void stale_scatter_coop_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, float *grid, const int *qa,
                                                                 const int *na, const int *qb, const int *nb, int *status) {
  constexpr int NC = SIDE * SIDE * SIDE;
  const int n0 = *na, n = n0 + *nb;
  const int sub = threadIdx.x & 31;
  const int ngrp = (int)((gridDim.x * blockDim.x) >> 5);
  const float dxi = mp.dxi;
  const float kscale = mp.fscale;
  const int a = sub / 9, b = (sub / 3) % 3, c = sub % 3;  // lanes 27-31 idle
  for (int j = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 5); j < n; j += ngrp) {
    const size_t i = (size_t)(j < n0 ? qa[j] : qb[j - n0]);
    float pos[3], vel[3], C[9], contrib[9];
    load_attr<3>(ps.pos, i, pos);
    load_attr<3>(ps.vel, i, vel);
    load_attr<9>(ps.C, i, C);
    {
      float S[STRESS_N];
      load_attr<STRESS_N>(ps.stress, i, S);
      stress_unpack(S, contrib);
    }
    const float mass = ps.mass.base[ps.mass.off(i)];
#pragma unroll
    for (int d = 0; d < 9; ++d) contrib[d] = contrib[d] * kscale;
    Arena ar;
    make_arena(mp.dx, mp.dxi, pos, ar);
    int loc[3], key[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      loc[d] = ar.corner[d] & (SIDE - 1);
      key[d] = (ar.corner[d] - loc[d]) / SIDE * mp.kscale;
    }
    int myblk = -1;
    if (sub < 8) {
      const bool need = (!(sub & 4) || loc[0] + 2 >= SIDE) && (!(sub & 2) || loc[1] + 2 >= SIDE) && (!(sub & 1) || loc[2] + 2 >= SIDE);
      int k[3] = {key[0] + (sub >> 2) * mp.kscale, key[1] + ((sub >> 1) & 1) * mp.kscale, key[2] + (sub & 1) * mp.kscale};
      if (need) myblk = bht_query<3>(t, k);
    }
    const int x = loc[0] + a, y = loc[1] + b, z = loc[2] + c;
    const int o = sub < 27 ? (((x >= SIDE) << 2) | ((y >= SIDE) << 1) | (z >= SIDE)) : 0;
    const int bn = __shfl(myblk, o, 32);
    if (sub < 27 && bn < 0 && status) status[2] = 1;  // a stencil node outside the partition: its contribution is lost
    if (sub < 27 && bn >= 0) {
      const int cell = ((x & (SIDE - 1)) * SIDE + (y & (SIDE - 1))) * SIDE + (z & (SIDE - 1));
      float *g = grid + (size_t)bn * 7 * NC + cell;
      const float xi0 = (float)a * mp.dx - ar.lp[0], xi1 = (float)b * mp.dx - ar.lp[1], xi2 = (float)c * mp.dx - ar.lp[2];
      float W = ar.w[0][a];
      W *= ar.w[1][b];
      W *= ar.w[2][c];
      unsafeAtomicAdd(g, mass * W);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        unsafeAtomicAdd(g + (1 + d) * NC, W * mass * (vel[d] + (C[d] * xi0 + C[3 + d] * xi1 + C[6 + d] * xi2)));
        unsafeAtomicAdd(g + (4 + d) * NC, (contrib[d] * xi0 + contrib[3 + d] * xi1 + contrib[6 + d] * xi2) * W);
      }
    }
  }
}

}  // namespace zsr
