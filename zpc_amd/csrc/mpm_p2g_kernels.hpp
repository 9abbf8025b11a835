#pragma once
// mpm_p2g_kernels.hpp -- the P2G kernels (particle order, binned, wide, tile-stream, exact path); included by mpm_p2g.hip only
#include "mpm_arena.hpp"

namespace zsr {

// ======================================================================================= P2G
// ---- particle-order path: the reference's algorithm (hash query + global float atomics per node), with the
//      27 queries folded into the <= 8 distinct blocks a stencil can touch.
template <int SIDE, int MODEL>
__device__ __forceinline__ void p2g_scatter_global(const MpmDev &mp, const ParticlesDev &ps, size_t i, const BhtDev &t, float *grid,
                                                   float D_inv) {
  constexpr int NC = SIDE * SIDE * SIDE;
  float pos[3], vel[3], C[9], contrib[9];
  load_attr<3>(ps.pos, i, pos);
  load_attr<3>(ps.vel, i, vel);
  load_attr<9>(ps.C, i, C);
  const float mass = ps.mass.base[ps.mass.off(i)];
  particle_contrib<MODEL>(mp, ps, i, D_inv, contrib);
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
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int x = loc[0] + a, y = loc[1] + b, z = loc[2] + c;
        const int o = ((x >= SIDE) << 2) | ((y >= SIDE) << 1) | (z >= SIDE);
        int bn = blk[0];
#pragma unroll
        for (int q = 1; q < 8; ++q) bn = (o == q) ? blk[q] : bn;
        if (bn < 0) continue;  // the reference does not check (P2G.hpp:109-110); a valid partition never gets here
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

template <int SIDE, int MODEL>
static __global__ __launch_bounds__(256) void p2g_global_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, float *grid) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ps.n) return;
  const float dxi = mp.dxi;
  p2g_scatter_global<SIDE, MODEL>(mp, ps, i, t, grid, 4.f * dxi * dxi);
}

template <int LW> struct RecA {  // sweep A inputs: x, v, C, m (16 floats)
  float pos[3], vel[3], C[9], mass;
  __device__ __forceinline__ void load(const ParticlesDev &ps, size_t i) {
    const POff<LW> o = particle_offset<LW>(ps.pos.chns, i);
    pload<LW, 3>(ps.pos, o, pos);
    pload<LW, 3>(ps.vel, o, vel);
    pload<LW, 9>(ps.C, o, C);
    mass = pload1<LW>(ps.mass, o);
  }
};
template <int SIDE, int MODEL, int LW>
static __global__ __launch_bounds__(64, 2) void p2g_binned_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, float *grid, const int *binStart,
                                                        const unsigned *cellCount, const int *nbr, int *stale, int *staleCount) {
  using AL = ArenaLds;
  constexpr int NC = SIDE * SIDE * SIDE;
  __shared__ float arena[7 * AL::CH];
  const int bin = (int)blockIdx.x;
  const int start = binStart[bin], end = binStart[bin + 1];
  if (start == end) return;  // empty bin (ghost block): uniform exit
  const int lane = threadIdx.x;
  for (int k = lane; k < 7 * AL::CH; k += 64) arena[k] = 0.f;
  const BinGeom<SIDE> geo(t, bin, mp.kscale);
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  const unsigned cnt = cellCount[(size_t)bin * 64 + lane];
  const float dxi = mp.dxi;
  const float D_inv = mp.D_inv;

  float *a0 = arena + AL::at(cx, cy, cz);
  __syncthreads();
  // Two sweeps over the bin's particles keep the register-resident stencil at 27 x 4 (mass, momentum) and
  // 27 x 3 (stress) accumulators instead of 27 x 7 = 189, which would cap occupancy at one wave per SIMD;
  // the price is reading x twice (+12 B/particle).
  {  // ---- sweep A: m, m v + m C (xi - xp)
    float acc[27][4];
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) acc[k][ch] = 0.f;
    RoundWalk walk(cnt, start);
    int i0, i1;
    bool any, any1;
    bool has0 = walk.next(i0, any);
    RecA<LW> cur, nxt;
    if (has0) cur.load(ps, (size_t)i0);
    while (any) {
      const bool has1 = walk.next(i1, any1);
      if (has1) nxt.load(ps, (size_t)i1);  // in flight while the current round is computed
      if (has0) {
        Arena ar;
        make_arena(mp.dx, mp.dxi, cur.pos, ar);
        if (ar.corner[0] - geo.org[0] != cx || ar.corner[1] - geo.org[1] != cy || ar.corner[2] - geo.org[2] != cz) {
          stale[atomicAdd(staleCount, 1)] = i0;  // left its cell since the last re-binning: exact path afterwards
        } else {
          // W m (v + C (xi - xp)) is affine in the node offset: evaluate it as (Px[a] + Py[b]) + Pz[c] with the
          // per-axis products hoisted -> 8 VALU ops per node instead of ~20 (rounding differs from the
          // reference's association by O(1 ulp), inside the stated tolerance)
          float Px[3][3], Py[3][3], Pz[3][3], wzm[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float x0 = (float)k * mp.dx - ar.lp[0], x1 = (float)k * mp.dx - ar.lp[1], x2 = (float)k * mp.dx - ar.lp[2];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              Px[k][d] = cur.C[d] * x0;
              Py[k][d] = cur.C[3 + d] * x1;
              Pz[k][d] = fmaf(cur.C[6 + d], x2, cur.vel[d]);
            }
            wzm[k] = ar.w[2][k] * cur.mass;
          }
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int bb = 0; bb < 3; ++bb) {
              const float wxy = ar.w[0][a] * ar.w[1][bb];
              const float q0 = Px[a][0] + Py[bb][0], q1 = Px[a][1] + Py[bb][1], q2 = Px[a][2] + Py[bb][2];
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const float Wm = wxy * wzm[c];
                float(&A)[4] = acc[(a * 3 + bb) * 3 + c];
                A[0] += Wm;
                A[1] = fmaf(Wm, q0 + Pz[c][0], A[1]);
                A[2] = fmaf(Wm, q1 + Pz[c][1], A[2]);
                A[3] = fmaf(Wm, q2 + Pz[c][2], A[3]);
              }
            }
        }
      }
      cur = nxt;
      has0 = has1;
      i0 = i1;
      any = any1;
    }
    // 27 phases: in phase (a,b,c) lane (cx,cy,cz) owns node (cx+a, cy+b, cz+c) -- all 64 nodes distinct
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      float *g = a0 + AL::at(k / 9, (k / 3) % 3, k % 3);
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) g[ch * AL::CH] += acc[k][ch];
      __syncthreads();
    }
  }
  {  // ---- sweep B: rhs = -dt D_inv (P F^T vol) (xi - xp) W
    float acc[27][3];
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[k][ch] = 0.f;
    RoundWalk walk(cnt, start);
    int i0, i1;
    bool any, any1;
    bool has0 = walk.next(i0, any);
    RecB<MODEL, LW> cur, nxt;
    if (has0) cur.load(ps, (size_t)i0);
    while (any) {
      const bool has1 = walk.next(i1, any1);
      if (has1) nxt.load(ps, (size_t)i1);
      if (has0) {
        Arena ar;
        make_arena(mp.dx, mp.dxi, cur.pos, ar);
        if (ar.corner[0] - geo.org[0] == cx && ar.corner[1] - geo.org[1] == cy && ar.corner[2] - geo.org[2] == cz) {
          float contrib[9];
          if constexpr (MODEL == MPM_CACHED_STRESS) {
#pragma unroll
            for (int d = 0; d < 9; ++d) contrib[d] = cur.F[d];
          } else {
            float lj = model_uses_logjp(MODEL) ? cur.logJp : 0.f;
            float Cp[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if constexpr (model_is_fluid(MODEL)) {
#pragma unroll
              for (int d = 0; d < 9; ++d) Cp[d] = cur.C[d];
            }
            model_stress<MODEL>(mp.mat, lj, cur.F, contrib, Cp);
            if constexpr (model_uses_logjp(MODEL))
              pstore1<LW>(ps.logJp, particle_offset<LW>(ps.pos.chns, (size_t)i0), lj);  // P2G.hpp:101 (projected F not written back)
          }
#pragma unroll
          for (int d = 0; d < 9; ++d) contrib[d] = contrib[d] * -mp.dt * D_inv;
          float Qx[3][3], Qy[3][3], Qz[3][3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float x0 = (float)k * mp.dx - ar.lp[0], x1 = (float)k * mp.dx - ar.lp[1], x2 = (float)k * mp.dx - ar.lp[2];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              Qx[k][d] = contrib[d] * x0;
              Qy[k][d] = contrib[3 + d] * x1;
              Qz[k][d] = contrib[6 + d] * x2;
            }
          }
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int bb = 0; bb < 3; ++bb) {
              const float wxy = ar.w[0][a] * ar.w[1][bb];
              const float q0 = Qx[a][0] + Qy[bb][0], q1 = Qx[a][1] + Qy[bb][1], q2 = Qx[a][2] + Qy[bb][2];
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const float Wt = wxy * ar.w[2][c];
                float(&A)[3] = acc[(a * 3 + bb) * 3 + c];
                A[0] = fmaf(Wt, q0 + Qz[c][0], A[0]);
                A[1] = fmaf(Wt, q1 + Qz[c][1], A[1]);
                A[2] = fmaf(Wt, q2 + Qz[c][2], A[2]);
              }
            }
        }
      }
      cur = nxt;
      has0 = has1;
      i0 = i1;
      any = any1;
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      float *g = a0 + AL::at(k / 9, (k / 3) % 3, k % 3) + 4 * AL::CH;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) g[ch * AL::CH] += acc[k][ch];
      __syncthreads();
    }
  }
  // flush: consecutive lanes -> consecutive z of one (channel, x, y) row
  int nb[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) nb[o] = nbr[(size_t)geo.block * 8 + o];
  for (int k = lane; k < 7 * 216; k += 64) {
    const int ch = k / 216, node = k % 216;
    const int x = node / 36, y = (node / 6) % 6, z = node % 6;
    const float v = arena[ch * AL::CH + AL::at(x, y, z)];
    if (v == 0.f) continue;
    int slot, cell;
    arena_to_grid<SIDE>(geo.o, x, y, z, slot, cell);
    int bn = nb[0];
#pragma unroll
    for (int q = 1; q < 8; ++q) bn = (slot == q) ? nb[q] : bn;
    if (bn < 0) continue;
    unsafeAtomicAdd(grid + ((size_t)bn * 7 + ch) * NC + cell, v);
  }
}


// ---- "wide" cached-stress P2G: ONE wave per bin carries all 7 channels (27 x 7 = 189 register accumulators).
// The four-wave split above repeats the arena / weight / address work in every wave (PMC: 1113 VALU instructions per
// 64-particle round, SQ_INSTS_VALU x 4 cycles = 96 % of the SIMD cycles: that kernel is VALU-bound).  Here the per-particle
// work is done once (~600 VALU per round).  The price is 2 waves per SIMD; the latency the occupancy no longer hides is
// covered by asynchronous global -> LDS loads (global_load_lds_dword: no staging VGPRs) issued one round ahead into a
// double-buffered record area of the LDS.
constexpr int P2GW_NF = 16 + STRESS_N;  // rows of a record: m, x, v, C, symmetric stress
constexpr int P2GW_MQ_CAP = 256;  // in-bin movers the wide P2G takes through its LDS queue  // m, x(3), v(3), C(9), P F^T vol(9)

// `tileBase`: wave-uniform element offset of a tile at or before the bin's first particle.  The per-lane part of every address
// is then a 32-bit byte offset from a scalar base (global_load_lds_dword v_off, s[base:base+1] offset:imm): ONE address VGPR
// per round instead of a 64-bit pointer per attribute.
template <int LW>
__device__ __forceinline__ void p2gw_issue(const ParticlesDev &ps, size_t i, bool has, float *buf, size_t tileBase) {
  // every lane of the wave executes the 25 instructions (LDS destination = wave-uniform row + lane * 4); lanes without a
  // particle in this round are masked off by exec
  if (has) {
    const POff<LW> o = particle_offset<LW>(ps.pos.chns, i);
    const unsigned voff = LW != 0 ? (unsigned)((o.o - tileBase) * sizeof(float)) : 0u;
    auto ptr = [&](const Port<float> &p, int comp) -> const float * {
      if constexpr (LW != 0)
        return reinterpret_cast<const float *>(reinterpret_cast<const char *>(p.base + tileBase) + (size_t)voff) + (size_t)comp * LW;
      else
        return p.base + p.off(o.o) + (size_t)comp * p.cstride();
    };
    __builtin_amdgcn_global_load_lds(ptr(ps.mass, 0), (__attribute__((address_space(3))) void *)(buf + 0 * 64), 4, 0, 0);
#pragma unroll
    for (int d = 0; d < 3; ++d) __builtin_amdgcn_global_load_lds(ptr(ps.pos, d), (__attribute__((address_space(3))) void *)(buf + (1 + d) * 64), 4, 0, 0);
#pragma unroll
    for (int d = 0; d < 3; ++d) __builtin_amdgcn_global_load_lds(ptr(ps.vel, d), (__attribute__((address_space(3))) void *)(buf + (4 + d) * 64), 4, 0, 0);
#pragma unroll
    for (int d = 0; d < 9; ++d) __builtin_amdgcn_global_load_lds(ptr(ps.C, d), (__attribute__((address_space(3))) void *)(buf + (7 + d) * 64), 4, 0, 0);
#pragma unroll
    for (int d = 0; d < STRESS_N; ++d) __builtin_amdgcn_global_load_lds(ptr(ps.stress, d), (__attribute__((address_space(3))) void *)(buf + (16 + d) * 64), 4, 0, 0);
  }
}
template <int LW> __device__ __forceinline__ size_t p2gw_tile_base(const ParticlesDev &ps, int start) {
  if constexpr (LW != 0) return ((size_t)start / LW) * (size_t)ps.pos.chns * LW;
  else return 0;
}

// one particle record (LDS row layout of p2gw_issue) -> the lane's 27 x 7 register stencil.
// r05, "Q form" (see stage_qform): per vector channel the value at the stencil's centre node and its change per node step,
//   momentum d: alpha = m (v_d + C[d, :] . (dx - lp)), b_k = m dx C[d + 3 k];  force d: alpha = kscale S[d, :] . (dx - lp), b_k = kscale dx S[d, k]
// (S = the symmetric P F^T vol), then per node W_abc (alpha + (a - 1) bx + (b - 1) by + (c - 1) bz): the offsets x_i - x_p and the products
// C (x_i - x_p) are no longer rebuilt per node, and ONE weight product W_abc serves all seven channels.
__device__ __forceinline__ void p2gw_accumulate(const MpmDev &mp, const Arena &ar, const float *rec, float kscale, float (&acc)[27][7]) {
  const float m = rec[0];
  float lc[3];  // centre node - particle
#pragma unroll
  for (int k = 0; k < 3; ++k) lc[k] = mp.dx - ar.lp[k];
  float al[6], bx[6], by[6], bz[6];
  {
    const float mdx = m * mp.dx, ksdx = kscale * mp.dx;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = rec[(4 + d) * 64], c0 = rec[(7 + d) * 64], c1 = rec[(10 + d) * 64], c2 = rec[(13 + d) * 64];
      al[d] = m * (v + (c0 * lc[0] + c1 * lc[1] + c2 * lc[2]));
      bx[d] = mdx * c0;
      by[d] = mdx * c1;
      bz[d] = mdx * c2;
      // row d of the symmetric P F^T vol {xx, xy, xz, yy, yz, zz} (rows 16..21 of the record)
      const float s0 = rec[(16 + d) * 64], s1 = rec[(16 + (d == 0 ? 1 : d == 1 ? 3 : 4)) * 64], s2 = rec[(16 + (d == 0 ? 2 : d == 1 ? 4 : 5)) * 64];
      al[3 + d] = kscale * (s0 * lc[0] + s1 * lc[1] + s2 * lc[2]);
      bx[3 + d] = ksdx * s0;
      by[3 + d] = ksdx * s1;
      bz[3 + d] = ksdx * s2;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float qa[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) qa[j] = a == 0 ? al[j] - bx[j] : (a == 1 ? al[j] : al[j] + bx[j]);
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      const float wxy = ar.w[0][a] * ar.w[1][bb];
      const float W0 = wxy * ar.w[2][0], W1 = wxy * ar.w[2][1], W2 = wxy * ar.w[2][2];
      float(&A0)[7] = acc[(a * 3 + bb) * 3], (&A1)[7] = acc[(a * 3 + bb) * 3 + 1], (&A2)[7] = acc[(a * 3 + bb) * 3 + 2];
      A0[0] = fmaf(W0, m, A0[0]);
      A1[0] = fmaf(W1, m, A1[0]);
      A2[0] = fmaf(W2, m, A2[0]);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float qab = bb == 0 ? qa[j] - by[j] : (bb == 1 ? qa[j] : qa[j] + by[j]);
        A0[1 + j] = fmaf(W0, qab - bz[j], A0[1 + j]);
        A1[1 + j] = fmaf(W1, qab, A1[1 + j]);
        A2[1 + j] = fmaf(W2, qab + bz[j], A2[1 + j]);
      }
    }
  }
}

// LDS arena shared by the G bins of one workgroup of p2g_wide_kernel: G = 1 one bin (6^3 nodes, ArenaLds), G = 2 the two bins of a
// block that are neighbours in z (4 x 4 x 8 cells, 6 x 6 x 10 nodes).  Strides from a search over (SY, SX): for a fixed stencil offset
// the 64 cells of a bin land on 32 distinct banks per half wave.
template <int G> struct ArenaLdsG;
template <> struct ArenaLdsG<1> {
  static constexpr int WX = 6, WY = 6, WZ = 6, SY = ArenaLds::SY, SX = ArenaLds::SX, CH = WX * SX;
  __device__ static constexpr int at(int x, int y, int z) { return x * SX + y * SY + z; }
};
template <> struct ArenaLdsG<2> {
  static constexpr int WX = 6, WY = 6, WZ = 10, SY = 12, SX = 80, CH = WX * SX;
  __device__ static constexpr int at(int x, int y, int z) { return x * SX + y * SY + z; }
};

// tail shared by the wide P2G kernels: the queued in-bin movers go into the arena by LDS atomics (same values as the exact path), then
// the arena goes to the grid -- origin of the workgroup's arena inside its block = the origin of its first bin
template <int SIDE, int G>
__device__ __forceinline__ void p2gw_movers_and_flush(const MpmDev &mp, const ParticlesDev &ps, const BinGeom<SIDE> &geo, float *arena, const int *mqw,
                                                      int mqCountW, int lane, int az, const int *nbr, float *grid) {
  using AL = ArenaLdsG<G>;
  constexpr int NC = SIDE * SIDE * SIDE;
  const float kscale = mp.fscale;
  {  // post-pass: the queued in-bin particles, one lane each, added to the arena with LDS atomics (same values as the exact path)
    const int nm = mqCountW < P2GW_MQ_CAP ? mqCountW : P2GW_MQ_CAP;
    for (int q = lane; q < nm; q += 64) {
      const size_t i = (size_t)mqw[q];
      float pos[3], vel[3], C[9], PF[9];
      load_attr<3>(ps.pos, i, pos);
      load_attr<3>(ps.vel, i, vel);
      load_attr<9>(ps.C, i, C);
      {
        float S[STRESS_N];
        load_attr<STRESS_N>(ps.stress, i, S);
        stress_unpack(S, PF);
      }
      const float m = ps.mass.base[ps.mass.off(i)];
#pragma unroll
      for (int d = 0; d < 9; ++d) PF[d] *= kscale;
      Arena ar;
      make_arena(mp.dx, mp.dxi, pos, ar);
      float *b0 = arena + AL::at(ar.corner[0] - geo.org[0], ar.corner[1] - geo.org[1], ar.corner[2] - geo.org[2] + az);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float W = ar.w[0][a] * ar.w[1][b] * ar.w[2][c];
            const float x0 = (float)a * mp.dx - ar.lp[0], x1 = (float)b * mp.dx - ar.lp[1], x2 = (float)c * mp.dx - ar.lp[2];
            float *g = b0 + AL::at(a, b, c);
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
  // flush: origin of the workgroup's arena inside its block = the origin of its first bin
  const int o0[3] = {geo.o[0], geo.o[1], geo.o[2] - az};
  for (int node = threadIdx.x; node < AL::WX * AL::WY * AL::WZ; node += 64 * G) {
    const int x = node / (AL::WY * AL::WZ), y = (node / AL::WZ) % AL::WY, z = node % AL::WZ;
    int slot2, cell;
    arena_to_grid<SIDE>(o0, x, y, z, slot2, cell);
    const int bn = nbr[(size_t)geo.block * 8 + slot2];
    if (bn >= 0) {
      const float *a = arena + AL::at(x, y, z);
      float *g = grid + (size_t)bn * 7 * NC + cell;
#pragma unroll
      for (int ch = 0; ch < 7; ++ch) {
        const float v = a[ch * AL::CH];
        if (v != 0.f) unsafeAtomicAdd(g + ch * NC, v);
      }
    }
  }
}

// DEPTH = rounds of records in flight ahead of the one being computed (DEPTH + 1 LDS buffers of P2GW_NF x 256 B per wave).
// G = bins (= waves) per workgroup.  Every wave streams its own bin exactly as a one-wave workgroup would (nothing is shared while the
// records flow); what the G waves share is the flush: their register stencils go into ONE arena and the workgroup issues one set of
// global float atomics for it.  The atomics are what the kernel writes (every atomic instruction writes the 32-byte sectors it touches
// through to memory, whatever the launch order: profiles/r04_launch_order.md), and neighbouring bins' aprons overlap: per 8^3 block
// 8 x 7 x 36 rows x 1.5 sectors = 3024 sector writes with G = 1, 2016 with G = 2 (a row of 10 z-nodes = the block's own 32-byte row + 8
// bytes of the next block's), 1680 with G = 4.
template <int SIDE, int LW, int DEPTH, int G>
static __global__ __launch_bounds__(64 * G, 2) void p2g_wide_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, float *grid, const int *binStart,
                                                           const unsigned *cellCount, const int *nbr, int *stale, int *staleCount) {
  static_assert(G == 1 || (SIDE == 8 && G == 2), "G bins of one block");
  using AL = ArenaLdsG<G>;
  constexpr int NC = SIDE * SIDE * SIDE;
  constexpr int NB = DEPTH + 1;
  constexpr int WBUF = NB * P2GW_NF * 64;  // floats of record buffers per wave
  // the record buffers and the flush arena are never live at the same time: one LDS region serves both
  constexpr int LDSF = G * WBUF > 7 * AL::CH ? G * WBUF : 7 * AL::CH;
  __shared__ float lds[LDSF];
  __shared__ int mq[G][P2GW_MQ_CAP];  // particles that sit in another cell of their bin (moved since the last re-bin)
  __shared__ int mqCount[G];
  const int w = G == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // (w in an SGPR)
  const int bin0 = (int)blockIdx.x * G, bin = bin0 + w;
  if (binStart[bin0] == binStart[bin0 + G]) return;  // none of the G bins holds a particle (workgroup-uniform)
  float *arena = lds;
  float(*pbuf)[P2GW_NF * 64] = reinterpret_cast<float(*)[P2GW_NF * 64]>(lds + w * WBUF);
  const int start = binStart[bin], end = binStart[bin + 1];
  if (lane == 0) mqCount[w] = 0;
  __syncthreads();
  const BinGeom<SIDE> geo(t, bin, mp.kscale);
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  const unsigned cnt = start == end ? 0u : cellCount[(size_t)bin * 64 + lane];
  const float dxi = mp.dxi;
  const float kscale = mp.fscale;  // contrib = -dt D_inv (P F^T vol)
  float acc[27][7];
#pragma unroll
  for (int k = 0; k < 27; ++k)
#pragma unroll
    for (int ch = 0; ch < 7; ++ch) acc[k][ch] = 0.f;
  // two walks over the same counts: `lead` runs DEPTH rounds ahead and issues the loads, `walk` consumes
  const size_t tileBase = p2gw_tile_base<LW>(ps, start);
  RoundWalk lead(cnt, start), walk(cnt, start);
  int li;
  bool lany = true;
  int issued = 0;  // rounds issued and not yet consumed (wave-uniform)
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {
    if (lany) {
      const bool lh = lead.next(li, lany);
      if (lany) {
        p2gw_issue<LW>(ps, (size_t)li, lh, pbuf[d % NB], tileBase);
        ++issued;
      }
    }
  }
  int slot = 0, lslot = DEPTH % NB;
  int i0;
  bool any;
  bool has0 = walk.next(i0, any);
  while (any) {
    if (lany) {
      const bool lh = lead.next(li, lany);
      if (lany) {
        p2gw_issue<LW>(ps, (size_t)li, lh, pbuf[lslot], tileBase);
        lslot = lslot + 1 == NB ? 0 : lslot + 1;
        ++issued;
      }
    }
    // wait until only the records issued AFTER the current one are still in flight
    // (a record is P2GW_NF loads; vmcnt holds 6 bits: two records in flight is the most that can be told apart)
    static_assert(2 * P2GW_NF <= 63, "vmcnt range");
    if (issued >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P2GW_NF) : "memory");
    else if (issued == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P2GW_NF) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (has0) {
      const float *rec = pbuf[slot] + lane;
      const float pos[3] = {rec[1 * 64], rec[2 * 64], rec[3 * 64]};
      Arena ar;
      make_arena(mp.dx, mp.dxi, pos, ar);
      const int ocx = ar.corner[0] - geo.org[0], ocy = ar.corner[1] - geo.org[1], ocz = ar.corner[2] - geo.org[2];
      if (ocx == cx && ocy == cy && ocz == cz) {
        p2gw_accumulate(mp, ar, rec, kscale, acc);
      } else {
        // another cell of the same bin: queued for the post-pass into the arena; outside the bin: exact path afterwards
        bool queued = false;
        if ((unsigned)ocx < 4u && (unsigned)ocy < 4u && (unsigned)ocz < 4u) {
          const int q = atomicAdd(&mqCount[w], 1);
          if (q < P2GW_MQ_CAP) {
            mq[w][q] = i0;
            queued = true;
          }
        }
        if (!queued) stale[atomicAdd(staleCount, 1)] = i0;
      }
    }
    --issued;
    slot = slot + 1 == NB ? 0 : slot + 1;
    has0 = walk.next(i0, any);
  }
  __syncthreads();  // every record of every wave has been consumed: the region becomes the arena
  for (int k = threadIdx.x; k < 7 * AL::CH; k += 64 * G) arena[k] = 0.f;
  __syncthreads();
  // this bin's corner inside the workgroup's arena: the G = 2 bins differ in z
  const int az = G == 1 ? 0 : (w & 1) * 4;
  float *a0 = arena + AL::at(cx, cy, cz + az);
#pragma unroll
  for (int k = 0; k < 27; ++k) {  // 27 conflict-free phases: in a phase the 64 G lanes of the workgroup own 64 G distinct nodes
    float *g = a0 + AL::at(k / 9, (k / 3) % 3, k % 3);
#pragma unroll
    for (int ch = 0; ch < 7; ++ch) g[ch * AL::CH] += acc[k][ch];
    if constexpr (G == 1) __builtin_amdgcn_wave_barrier();  // one wave: its LDS operations execute in order
    else __syncthreads();
  }
  __syncthreads();
  p2gw_movers_and_flush<SIDE, G>(mp, ps, geo, arena, mq[w], mqCount[w], lane, az, nbr, grid);
}

// The lane's 27 x 7 node sums of p2g_tile_kernel with the six vector channels as three register PAIRS per node, {mv_x, mv_y},
// {mv_z, f_x}, {f_y, f_z}: the Q-form accumulation then issues one v_pk_add_f32 / v_pk_fma_f32 where p2gw_accumulate issues two scalar
// instructions (the node's weight is broadcast from the low half of its pair: op_sel_hi:[0,1,1]).  A wave issues one instruction every
// ~5 cycles whatever it is (profiles/r02_valu_opcode_rates.md) and this kernel has two waves per SIMD, so its record stream is bound by
// the NUMBER of instructions a wave issues, not by the VALU rate (where a packed instruction costs 1.7 scalar ones: r03, fused kernels).
// Each half is the same IEEE operation as the scalar form; the products are formed in the same order as in p2gw_accumulate.
typedef float p2g_f2 __attribute__((ext_vector_type(2)));
struct P2GAccPk {
  float m[27];
  p2g_f2 q[27][3];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      m[k] = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j) q[k][j] = p2g_f2{0.f, 0.f};
    }
  }
  __device__ __forceinline__ float get(int k, int ch) const { return ch == 0 ? m[k] : (((ch - 1) & 1) ? q[k][(ch - 1) >> 1].y : q[k][(ch - 1) >> 1].x); }
};
// `own` false: the lane adds zeros (its record and its weights are replaced by zeros first: they may be anything, NaN included) -- the
// accumulation is NOT a divergent region, whose join would copy every register pair.
__device__ __forceinline__ void p2gw_accumulate_pk(const MpmDev &mp, const Arena &ar0, const float *rec0, float kscale, bool own, P2GAccPk &A) {
  Arena ar;
  float recv[P2GW_NF];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ar.lp[d] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) ar.w[d][k] = 0.f;
  }
#pragma unroll
  for (int r = 0; r < P2GW_NF; ++r) recv[r] = 0.f;
  if (own) {  // ONE divergent region: the record's reads and the copies of the weights
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      ar.lp[d] = ar0.lp[d];
#pragma unroll
      for (int k = 0; k < 3; ++k) ar.w[d][k] = ar0.w[d][k];
    }
    recv[0] = rec0[0];
#pragma unroll
    for (int r = 4; r < P2GW_NF; ++r) recv[r] = rec0[r * 64];
  }
  struct { const float *v; __device__ __forceinline__ float operator[](int i) const { return v[i / 64]; } } rec{recv};
  const float m = rec[0];
  float lc[3];  // centre node - particle
#pragma unroll
  for (int k = 0; k < 3; ++k) lc[k] = mp.dx - ar.lp[k];
  float al[6], bx[6], by[6], bz[6];
  {
    const float mdx = m * mp.dx, ksdx = kscale * mp.dx;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = rec[(4 + d) * 64], c0 = rec[(7 + d) * 64], c1 = rec[(10 + d) * 64], c2 = rec[(13 + d) * 64];
      al[d] = m * (v + (c0 * lc[0] + c1 * lc[1] + c2 * lc[2]));
      bx[d] = mdx * c0;
      by[d] = mdx * c1;
      bz[d] = mdx * c2;
      const float s0 = rec[(16 + d) * 64], s1 = rec[(16 + (d == 0 ? 1 : d == 1 ? 3 : 4)) * 64], s2 = rec[(16 + (d == 0 ? 2 : d == 1 ? 4 : 5)) * 64];
      al[3 + d] = kscale * (s0 * lc[0] + s1 * lc[1] + s2 * lc[2]);
      bx[3 + d] = ksdx * s0;
      by[3 + d] = ksdx * s1;
      bz[3 + d] = ksdx * s2;
    }
  }
  p2g_f2 alp[3], bxp[3], byp[3], bzp[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    alp[j] = p2g_f2{al[2 * j], al[2 * j + 1]};
    bxp[j] = p2g_f2{bx[2 * j], bx[2 * j + 1]};
    byp[j] = p2g_f2{by[2 * j], by[2 * j + 1]};
    bzp[j] = p2g_f2{bz[2 * j], bz[2 * j + 1]};
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p2g_f2 qa[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) qa[j] = a == 0 ? alp[j] - bxp[j] : (a == 1 ? alp[j] : alp[j] + bxp[j]);
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      const float wxy = ar.w[0][a] * ar.w[1][bb];
      const float W0 = wxy * ar.w[2][0], W1 = wxy * ar.w[2][1], W2 = wxy * ar.w[2][2];
      const int k0 = (a * 3 + bb) * 3;
      A.m[k0] = fmaf(W0, m, A.m[k0]);
      A.m[k0 + 1] = fmaf(W1, m, A.m[k0 + 1]);
      A.m[k0 + 2] = fmaf(W2, m, A.m[k0 + 2]);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const p2g_f2 qab = bb == 0 ? qa[j] - byp[j] : (bb == 1 ? qa[j] : qa[j] + byp[j]);
        A.q[k0][j] = __builtin_elementwise_fma((p2g_f2)(W0), qab - bzp[j], A.q[k0][j]);
        A.q[k0 + 1][j] = __builtin_elementwise_fma((p2g_f2)(W1), qab, A.q[k0 + 1][j]);
        A.q[k0 + 2][j] = __builtin_elementwise_fma((p2g_f2)(W2), qab + bzp[j], A.q[k0 + 2][j]);
      }
    }
  }
}

// private flush arena of one wave of p2g_tile_kernel: 6^3 nodes, one float4 per node and plane (plane 0: m, mv; plane 1: f), strides in
// nodes z + 12 y + 72 x: a 16-byte access of the wave is served in four passes of 16 lanes = the 4 x 4 (y, z) cells of one x, and
// 12 y + z (+ a phase offset) takes 16 distinct values mod 16 there -- no bank conflict in any of the 27 phases.
struct ArenaPriv {
  static constexpr int SY = 12, SX = 72, PLANE = 6 * SX;
  __device__ static constexpr int at(int x, int y, int z) { return x * SX + y * SY + z; }
};

// ---- tile-stream variant of the wide P2G (LW = 64 only): the record loads are decoupled from the rounds.
// A bin's particles are the contiguous range [start, end) of the compact order, i.e. the tiles start / 64 .. (end - 1) / 64 of the AoSoA
// container.  The wave requests WHOLE TILES (22 rows x 256 B by 6 - 8 `global_load_lds_dwordx4` of 1 KiB each instead of 22 dword
// requests per round of ~42 particles: an LDS-direct load costs the wave tens of cycles of issue whatever its width) into a ring of NB tile buffers as soon as
// the bin's range is known -- before its cell counts arrive, so the head of a wave is ONE memory round trip instead of two -- and a
// round's lane reads its particle at ring position (index mod 64) of tile (index / 64).  A tile buffer is re-requested when the walk has
// passed the tile's last particle: NB - 1 tiles (1.5 - 3 rounds) stay in flight ahead of the round being accumulated.
// One request = one `global_load_lds_dwordx4`: lane l moves 16 bytes from (row base + 16 l) to (LDS base + 16 l), i.e. FOUR consecutive
// 256-byte channel rows of the tile per wave-instruction (1 KiB), and the instruction offset advances both addresses.  MERGED: the host
// found m, x, v, C in 16 adjacent channels (the layout of zpc_amd.mpm and of the reference's particles TileVector {m, x, v, C, ...}):
// 4 + 2 requests per tile; otherwise one base per attribute, 8 requests (the last of an attribute with the lanes of its remaining rows).
// The requests are inline assembly on purpose: for the builtin the compiler puts `s_waitcnt vmcnt(0)` in front of every LDS read that
// follows an LDS-direct load it cannot tell apart (SIInsertWaitcnts: any DS read may alias a pending LDS-DMA write), i.e. in front of
// the first record read of EVERY round -- the ring would never hold a tile in flight.  The kernel orders reads behind arrivals itself
// (the vmcnt switch in front of a round), so the compiler must not know these are loads into LDS.  M0 = LDS base of the request.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void p2gt_dma4(unsigned long long sbase, unsigned voff, unsigned ldsAddr) {  // one dword per lane
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(ldsAddr) : "memory", "m0");
}
template <int OFF0, int CNT> __device__ __forceinline__ void p2gt_dma16_run(unsigned long long sbase, unsigned voff, unsigned ldsAddr) {
  // CNT requests 1 KiB apart (global and LDS address advance together through the instruction offset), one M0 write
  static_assert(CNT >= 1 && CNT <= 4, "instruction offsets up to 3072");
  if constexpr (CNT == 1)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3" ::"v"(voff), "s"(sbase), "s"(ldsAddr), "n"(OFF0) : "memory", "m0");
  else if constexpr (CNT == 2)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3\n\tglobal_load_lds_dwordx4 %0, %1 offset:%4" ::"v"(voff), "s"(sbase), "s"(ldsAddr),
                 "n"(OFF0), "n"(OFF0 + 1024) : "memory", "m0");
  else if constexpr (CNT == 3)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3\n\tglobal_load_lds_dwordx4 %0, %1 offset:%4\n\tglobal_load_lds_dwordx4 %0, %1 offset:%5" ::"v"(voff),
                 "s"(sbase), "s"(ldsAddr), "n"(OFF0), "n"(OFF0 + 1024), "n"(OFF0 + 2048) : "memory", "m0");
  else
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 offset:%3\n\tglobal_load_lds_dwordx4 %0, %1 offset:%4\n\tglobal_load_lds_dwordx4 %0, %1 offset:%5\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:%6" ::"v"(voff), "s"(sbase), "s"(ldsAddr), "n"(OFF0), "n"(OFF0 + 1024), "n"(OFF0 + 2048), "n"(OFF0 + 3072) : "memory", "m0");
}
#pragma clang diagnostic pop
template <int ROW0, int N>
__device__ __forceinline__ void p2gt_issue_attr(const Port<float> &p, size_t tb, int lane, float *buf) {
  // wave-uniform row base in an SGPR pair + one 32-bit lane offset
  const unsigned long long ub = (unsigned long long)(p.base + tb);
  const unsigned long long sb = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(ub >> 32)) << 32) |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ub);
  const unsigned voff = (unsigned)lane * 16u;
  const unsigned l = (unsigned)(size_t)(__attribute__((address_space(3))) float *)(buf + ROW0 * 64);
  constexpr int FULL = N / 4, REST = N % 4;
  static_assert(FULL <= 4, "up to 16 + 3 rows per base");
  if constexpr (FULL > 0) p2gt_dma16_run<0, FULL>(sb, voff, l);
  if constexpr (REST > 0)
    if (lane < REST * 16) p2gt_dma16_run<FULL * 1024, 1>(sb, voff, l);
}
template <bool MERGED> constexpr int p2gt_requests() { return MERGED ? 4 + (STRESS_N + 3) / 4 : 1 + 1 + 1 + 3 + (STRESS_N + 3) / 4; }
// [lo, hi): the particles of the tile that belong to this bin (0, 64 for an inner tile).  A lane moves the 4 particles 4 (lane mod 16) ...
// + 3 of a row; lanes whose four lie outside the range stay out of ALL the tile's requests, so that a 128-byte line of a boundary tile that
// only the neighbouring bin needs is not fetched here as well (the whole-tile form read 4 % more than the records: profiles/r06_pmc_p2g.md).
template <bool MERGED>
__device__ __forceinline__ void p2gt_issue(const ParticlesDev &ps, int tile, int lo, int hi, int lane, float *buf) {
  // element offset of the tile (wave-uniform); the stress attribute may live in a TileVector of its own (another channel count: the
  // reference-order P2G keeps it in a temporary, see zs_rocm_mpm_p2g)
  const size_t tb = (size_t)tile * (size_t)ps.pos.chns * 64, tbs = (size_t)tile * (size_t)ps.stress.chns * 64;
  const int pl = (lane & 15) * 4;
  if (pl + 3 >= lo && pl < hi) {
    if constexpr (MERGED) {
      p2gt_issue_attr<0, 16>(ps.mass, tb, lane, buf);
    } else {
      p2gt_issue_attr<0, 1>(ps.mass, tb, lane, buf);
      p2gt_issue_attr<1, 3>(ps.pos, tb, lane, buf);
      p2gt_issue_attr<4, 3>(ps.vel, tb, lane, buf);
      p2gt_issue_attr<7, 9>(ps.C, tb, lane, buf);
    }
    p2gt_issue_attr<16, STRESS_N>(ps.stress, tbs, lane, buf);
  }
}

template <int SIDE, int NB, int G, bool MERGED>
static __global__ __launch_bounds__(64 * G, 2) void p2g_tile_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, float *grid, const int *binStart,
                                                           const unsigned *cellCount, const int *nbr, int *stale, int *staleCount) {
  static_assert(G == 1 || (SIDE == 8 && G == 2), "G bins of one block");
  constexpr int NL = p2gt_requests<MERGED>();  // load instructions per tile
  static_assert((NB - 1) * NL <= 63, "vmcnt range");
  using AL = ArenaLdsG<G>;
  constexpr int NC = SIDE * SIDE * SIDE;
  constexpr int TILEF = P2GW_NF * 64;     // floats of one tile buffer
  constexpr int WBUF = NB * TILEF;        // ... of a wave's ring
  constexpr int LDSF = G * WBUF > 7 * AL::CH ? G * WBUF : 7 * AL::CH;  // ring and flush arena are never live at the same time
  __shared__ float lds[LDSF];
  __shared__ int mq[G][P2GW_MQ_CAP];
  __shared__ int mqCount[G];
  __shared__ unsigned cntLds[G][64];
  const int w = G == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int bin0 = (int)blockIdx.x * G, bin = bin0 + w;
  // the G + 1 range words of the workgroup's bins and this wave's cell counts are requested together
  int bs[G + 1];
#pragma unroll
  for (int k = 0; k <= G; ++k) bs[k] = binStart[bin0 + k];
  int start = bs[0], end = bs[1];
#pragma unroll
  for (int k = 1; k < G; ++k)
    if (w == k) start = bs[k], end = bs[k + 1];
  // the wave's cell counts (all zero for an empty bin) come through LDS like the tiles, requested in front of them: a load into a
  // register that the compiler tracks would get its `s_waitcnt vmcnt(n)` computed without the tile requests behind it (i.e. wait for
  // every tile requested so far), and one it does not track could be copied before it has landed
  {
    const unsigned long long cb = (unsigned long long)(cellCount + (size_t)bin * 64);
    const unsigned long long scb = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(cb >> 32)) << 32) |
                                   (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)cb);
    p2gt_dma4(scb, (unsigned)lane * 4u, (unsigned)(size_t)(__attribute__((address_space(3))) unsigned *)cntLds[w]);
  }
  float *arena = lds;
  float *ring = lds + w * WBUF;
  const int tile0 = start >> 6, tileEnd = (end + 63) >> 6;  // the bin's tiles (none if start == end)
  int tIssue = tile0;  // next tile to request; its buffer is ring[(tIssue - tile0) % NB] = islot
  int islot = 0;
  auto request = [&]() {
    const int lo = tIssue == tile0 ? (start & 63) : 0, hi = tIssue == tileEnd - 1 ? end - (tIssue << 6) : 64;
    p2gt_issue<MERGED>(ps, tIssue, lo, hi, lane, ring + islot * TILEF);
    ++tIssue;
    islot = islot + 1 == NB ? 0 : islot + 1;
  };
  if (start != end) {
#pragma unroll 1
    for (int k = 0; k < NB; ++k)
      if (tIssue < tileEnd) request();
  }
  if (bs[0] == bs[G]) return;  // none of the G bins holds a particle (workgroup-uniform)
  if (lane == 0) mqCount[w] = 0;  // (only this wave touches mq[w] / mqCount[w]: its LDS operations execute in order)
  BinGeom<SIDE> geo(bin);
  {  // the block's key by scalar loads (constant address space + uniform address)
    const auto *ak = reinterpret_cast<const __attribute__((address_space(4))) int *>(reinterpret_cast<unsigned long long>(t.activeKeys));
#pragma unroll
    for (int d = 0; d < 3; ++d) geo.org[d] = ak[3 * (size_t)geo.block + d] * (SIDE / mp.kscale) + geo.o[d];
  }
  // the block's 8 neighbour numbers {+0, +1}^3 for the flush: wave-uniform, requested now (scalar loads) instead of one dependent
  // vector load per flushed node at the end of the wave's life
  int nbs[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)  // (constant address space + uniform address = s_load: vmcnt stays the record requests' own)
    nbs[k] = reinterpret_cast<const __attribute__((address_space(4))) int *>(reinterpret_cast<unsigned long long>(nbr))[(size_t)geo.block * 8 + k];
  const float kscale = mp.fscale;  // contrib = -dt D_inv (P F^T vol)
  P2GAccPk acc;
  acc.clear();
  int base = start;      // first particle of the round (wave-uniform)
  int tDone = tile0;     // tiles below have arrived
  int cslot = 0;         // ring slot of tile base / 64
  unsigned r = 0;
  {  // the cell counts were requested before the first tiles: they have arrived once at most the tiles' requests are outstanding
    const int req = tIssue - tile0;
    if (req >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB >= 3 ? 3 * NL : 0) : "memory");
    else if (req == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NL) : "memory");
    else if (req == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  const unsigned cnt = cntLds[w][lane];
  bool has = cnt > r;
  unsigned long long m = __ballot(has);
  while (m != 0ull) {
    const int nr = __popcll(m);
    const int p = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    const int tb = base >> 6, tLast = (base + nr - 1) >> 6;
    // a tile buffer is free once the walk has passed the tile: tile tIssue - NB was left when base reached (tIssue - NB + 1) * 64
    if (tIssue < tileEnd && tb > tIssue - NB) request();
    if (tLast >= tDone) {
      const int ahead = tIssue - 1 - tLast;  // requested tiles the round does not need yet
      if (NB >= 4 && ahead >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB >= 4 ? 3 * NL : 0) : "memory");
      else if (NB >= 3 && ahead == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NL) : "memory");
      else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      tDone = tLast + 1;
    }
    {
      // every lane reads "its" record (a lane without a particle in this round reads some record of the ring: never used) so that the
      // round has ONE divergent region, the accumulation; movers are rare and sit behind a wave-uniform branch
      const int nslot = cslot + 1 == NB ? 0 : cslot + 1;
      const float *rec = ring + ((p >> 6) == tb ? cslot : nslot) * TILEF + (p & 63);
      const float pos[3] = {rec[1 * 64], rec[2 * 64], rec[3 * 64]};
      Arena ar;
      make_arena(mp.dx, mp.dxi, pos, ar);
      const int ocx = ar.corner[0] - geo.org[0], ocy = ar.corner[1] - geo.org[1], ocz = ar.corner[2] - geo.org[2];
      const bool inBin = (unsigned)(ocx | ocy | ocz) < 4u;  // all three in 0..3
      const bool own = has && inBin && ((ocx << 4) | (ocy << 2) | ocz) == lane;  // lane = cell: (x, y, z) = (lane >> 4, (lane >> 2) & 3, lane & 3)
      p2gw_accumulate_pk(mp, ar, rec, kscale, own, acc);
      if (__ballot(has && !own) != 0ull) {  // some particle has left the cell it is stored under (wave-uniform, rare)
        if (has && !own) {
          bool queued = false;
          if (inBin) {  // another cell of the same bin: queued for the post-pass into the arena; outside the bin: exact path afterwards
            const int q = atomicAdd(&mqCount[w], 1);
            if (q < P2GW_MQ_CAP) {
              mq[w][q] = p;
              queued = true;
            }
          }
          if (!queued) stale[atomicAdd(staleCount, 1)] = p;
        }
      }
    }
    base += nr;
    if ((base >> 6) != tb) cslot = cslot + 1 == NB ? 0 : cslot + 1;
    ++r;
    has = cnt > r;
    m = __ballot(has);
  }
  // ---- tail.  Every tile the wave requested has been consumed, so its ring is free: it becomes the wave's PRIVATE 6^3 arena, two
  // planes of one float4 per node ({m, mv} and {f, -}: ArenaPriv).  No other wave touches it until the group's barrier below, and a
  // wave's LDS operations execute in order, so the 27 read-add-write phases need no barrier and no wait for a write: the 16-byte read
  // of (phase k + 1, plane p) is issued right behind the write of (phase k, plane p).
  using AP = ArenaPriv;
  static_assert(2 * AP::PLANE * 4 <= WBUF && WBUF % 4 == 0, "private arena inside the wave's ring, 16-byte accesses");
  float4 *priv = reinterpret_cast<float4 *>(ring);
  for (int k = lane; k < 2 * AP::PLANE; k += 64) priv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
#define P2GT_LDS_ORDER()                                   \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)
  P2GT_LDS_ORDER();
  {
    float4 *a0 = priv + AP::at(lane >> 4, (lane >> 2) & 3, lane & 3);
    float4 va = a0[0], vb = a0[AP::PLANE];
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      float4 *g = a0 + AP::at(k / 9, (k / 3) % 3, k % 3);
      float4 *gn = a0 + AP::at((k + 1) / 9, ((k + 1) / 3) % 3, (k + 1) % 3);
      g[0] = make_float4(va.x + acc.get(k, 0), va.y + acc.get(k, 1), va.z + acc.get(k, 2), va.w + acc.get(k, 3));
      P2GT_LDS_ORDER();
      if (k + 1 < 27) va = gn[0];
      g[AP::PLANE] = make_float4(vb.x + acc.get(k, 4), vb.y + acc.get(k, 5), vb.z + acc.get(k, 6), 0.f);
      P2GT_LDS_ORDER();
      if (k + 1 < 27) vb = gn[AP::PLANE];
    }
  }
  {  // the queued in-bin movers, one lane each, by LDS atomics into the private arena (same values as the exact path)
    const int nm = mqCount[w] < P2GW_MQ_CAP ? mqCount[w] : P2GW_MQ_CAP;
    for (int q = lane; q < nm; q += 64) {
      const size_t i = (size_t)mq[w][q];
      float pos[3], vel[3], C[9], PF[9];
      load_attr<3>(ps.pos, i, pos);
      load_attr<3>(ps.vel, i, vel);
      load_attr<9>(ps.C, i, C);
      {
        float S[STRESS_N];
        load_attr<STRESS_N>(ps.stress, i, S);
        stress_unpack(S, PF);
      }
      const float pm = ps.mass.base[ps.mass.off(i)];
#pragma unroll
      for (int d = 0; d < 9; ++d) PF[d] *= kscale;
      Arena ar;
      make_arena(mp.dx, mp.dxi, pos, ar);
      float *b0 = reinterpret_cast<float *>(priv + AP::at(ar.corner[0] - geo.org[0], ar.corner[1] - geo.org[1], ar.corner[2] - geo.org[2]));
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float W = ar.w[0][a] * ar.w[1][b] * ar.w[2][c];
            const float x0 = (float)a * mp.dx - ar.lp[0], x1 = (float)b * mp.dx - ar.lp[1], x2 = (float)c * mp.dx - ar.lp[2];
            float *g = b0 + 4 * AP::at(a, b, c);
            atomicAdd(g, W * pm);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
              atomicAdd(g + 1 + d, W * pm * (vel[d] + (C[d] * x0 + C[3 + d] * x1 + C[6 + d] * x2)));
              atomicAdd(g + 4 * AP::PLANE + d, (PF[d] * x0 + PF[3 + d] * x1 + PF[6 + d] * x2) * W);
            }
          }
    }
  }
  if constexpr (G == 1) P2GT_LDS_ORDER();
  else __syncthreads();  // the G private arenas are complete
#undef P2GT_LDS_ORDER
  // flush.  The group's nodes (6 x 6 x 6 G: the G = 2 bins differ in z) go to the grid once each: an apron node between two bins is
  // the sum of what their private arenas hold for it.
  {
    const int wz = G == 1 ? 0 : (w & 1) * 4;
    const int o0[3] = {geo.o[0], geo.o[1], geo.o[2] - wz};  // origin of the group inside its block = the origin of its first bin
    constexpr int NODES = AL::WX * AL::WY * AL::WZ, ITER = (NODES + 64 * G - 1) / (64 * G);
    float4 va[ITER], vb[ITER];
    int goff[ITER];  // element offset of the node's first channel in the grid, -1: no such block / no such node
#pragma unroll
    for (int it = 0; it < ITER; ++it) {  // every LDS read of the flush first ...
      const int node = (int)threadIdx.x + it * 64 * G;
      va[it] = vb[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      goff[it] = -1;
      if (node < NODES) {
        const int x = node / (AL::WY * AL::WZ), y = (node / AL::WZ) % AL::WY, z = node % AL::WZ;
        int slot2, cell;
        arena_to_grid<SIDE>(o0, x, y, z, slot2, cell);
        const int b01 = (slot2 & 1) ? nbs[1] : nbs[0], b23 = (slot2 & 1) ? nbs[3] : nbs[2], b45 = (slot2 & 1) ? nbs[5] : nbs[4],
                  b67 = (slot2 & 1) ? nbs[7] : nbs[6];
        const int b03 = (slot2 & 2) ? b23 : b01, b47 = (slot2 & 2) ? b67 : b45;
        const int bn = (slot2 & 4) ? b47 : b03;
        if (bn >= 0) goff[it] = bn * (7 * NC) + cell;
#pragma unroll
        for (int gz = 0; gz < G; ++gz) {
          const int lz = z - 4 * gz;
          if ((unsigned)y < 6u && (unsigned)lz < 6u) {
            const float4 *a = reinterpret_cast<const float4 *>(lds + gz * WBUF) + AP::at(x, y, lz);
            const float4 pa = a[0], pb = a[AP::PLANE];
            va[it] = make_float4(va[it].x + pa.x, va[it].y + pa.y, va[it].z + pa.z, va[it].w + pa.w);
            vb[it] = make_float4(vb[it].x + pb.x, vb[it].y + pb.y, vb[it].z + pb.z, 0.f);
          }
        }
      }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it)  // ... then the float atomics
      if (goff[it] >= 0) {
        float *g = grid + (size_t)(unsigned)goff[it];
        const float val[7] = {va[it].x, va[it].y, va[it].z, va[it].w, vb[it].x, vb[it].y, vb[it].z};
#pragma unroll
        for (int ch = 0; ch < 7; ++ch)
          if (val[ch] != 0.f) unsafeAtomicAdd(g + ch * NC, val[ch]);
      }
  }
}

// exact path for the queued particles (persistent grid-stride over a device-side count)
template <int SIDE, int MODEL>
static __global__ __launch_bounds__(256) void p2g_stale_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, float *grid, const int *stale,
                                                        const int *staleCount) {
  const int n = *staleCount;
  const float dxi = mp.dxi;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    p2g_scatter_global<SIDE, MODEL>(mp, ps, (size_t)stale[j], t, grid, 4.f * dxi * dxi);
}

}  // namespace zsr
