#pragma once
// mpm_arena.hpp -- device code shared by the stand-alone transfers (mpm_p2g_kernels.hpp, mpm_g2p_kernels.hpp) and the fused steps
// (mpm_fused_kernels.hpp, mpm_slot.hpp): bins and their LDS arenas, the arena <-> grid passes of the slotted per-bin step
// (arena_gather_velocities, arena_flush_to_grid), the round-robin walk, the G2P gather from an arena, the tail of G2P
// (state advance + constitutive update for the next P2G) and the exact gather by hash queries.  No kernel lives here.
//
// The transfers replace, behind include/zs_rocm.h:
//   P2GTransfer::operator()                  simulation/transfer/P2G.hpp:51-125 (+ cuda/simulation/transfer/P2G.hpp:38-116)
//   G2PTransfer::operator()                  simulation/transfer/G2P.hpp:44-83
//
// The reference's CUDA P2G issues 27 hash queries + 189 global float atomics per particle.  Here:
//   * particles are binned by the 4x4x4 cell group ("bin") of their base node (count -> scan -> distribute,
//     the IndexBuckets idea of simulation/particle/Query.tpp:9-58) and stored round-robin over the 64 cells
//     of a bin: round r holds the r-th particle of every cell that has one;
//   * one wavefront owns one bin, lane c owns cell c.  All particles of a cell share the same 27 stencil
//     nodes, so the lane accumulates its 27 x 7 node contributions IN REGISTERS across its particles, then
//     adds them into a per-wave LDS arena of 6^3 nodes x 7 channels in 27 conflict-free phases (plain
//     ds_read/ds_write: for a fixed stencil offset the 64 cells map to 64 distinct nodes on 32 distinct
//     banks per half-wave), and the arena is flushed ONCE to the grid with global_atomic_add_f32.
//     LDS float atomics are deliberately NOT used: ds_add_f32 measures 193 cycles per wave-instruction on
//     gfx950 (3 cycles per lane, serialised) against 4.2 for ds_add_u32 and 11 for a read-add-write pair
//     (tools/lds_bench.hip, profiles/); the first version of this kernel spent 94 % of its time in them;
//   * particles that left their cell since the last re-binning are queued and handled by the exact
//     particle-order kernel afterwards, so results never depend on how fresh the bins are;
//   * the 3x3 SVD is per-lane scalar VALU (quaternion Jacobi, v_rsq_f32): it is not a dense
//     contraction, so no MFMA;
//   * G2P: the lane loads the 27 x 3 node velocities of its cell from the LDS arena once and keeps them in
//     registers for all its particles.
// Algorithmic HBM bytes per particle: P2G 100 B read (+ 7 B grid), G2P 48 B read + 96 B write (+1.5 B grid).
#include "bht.hpp"
#include "mpm_particles.hpp"

namespace zsr {

// A "bin" is a 4x4x4 group of cells = 64 cells = one wavefront.  SIDE 4: bin == grid block.  SIDE 8: a grid
// block holds 2x2x2 bins, bin = block * 8 + sub, sub = ((lx>>2)*2 + (ly>>2))*2 + (lz>>2).
// Launch order of the per-bin kernels: plain blockIdx.  (r04, measured: giving XCD k the k-th contiguous eighth of the bins -- the
// dispatcher deals workgroups round-robin over the 8 XCDs -- changes neither the atomics' write traffic, which is write-through per
// touched 32-byte sector whatever the order, nor the time for the better: the empty apron bins end up on a few XCDs and the
// stand-alone P2G runs 1.83 -> 2.09 ms, the slotted step 7.9 -> 11.3 ms; numbering the blocks lexicographically or along the Morton
// curve instead of in insertion order: 1.86 / 1.91 ms and 8.5 / 8.2 ms.  profiles/r04_launch_order.md.)

template <int SIDE> constexpr int bins_per_block() { return (SIDE / 4) * (SIDE / 4) * (SIDE / 4); }

// ---- binned path
// LDS arena of one bin: 6^3 nodes, strides (floats) z + 8 y + 52 x: for a fixed stencil offset the 64 cells of
// a bin land on 32 distinct banks per 32-lane half.
struct ArenaLds {
  static constexpr int W = 6;
  static constexpr int SY = 8, SX = 52, CH = W * SX;
  __device__ static constexpr int at(int x, int y, int z) { return x * SX + y * SY + z; }
};

// LDS arena of one 8^3 block: 10^3 nodes (the block's cells + the two node layers of the quadratic stencil), dense
struct ArenaBlk {
  static constexpr int W = 10;
  static constexpr int SY = 10, SX = 100, CH = 1000;
  __device__ static constexpr int at(int x, int y, int z) { return x * SX + y * SY + z; }
};

// geometry of bin `bin`: grid block, origin of the bin inside the block (cells), origin in world cells
template <int SIDE> struct BinGeom {
  int block, o[3], org[3];
  __device__ __forceinline__ explicit BinGeom(int bin) {  // block and origin inside it; the caller fills org
    constexpr int BPB = bins_per_block<SIDE>();
    block = bin / BPB;
    const int sub = bin % BPB;
    o[0] = SIDE == 4 ? 0 : ((sub >> 2) & 1) * 4;
    o[1] = SIDE == 4 ? 0 : ((sub >> 1) & 1) * 4;
    o[2] = SIDE == 4 ? 0 : (sub & 1) * 4;
  }
  __device__ __forceinline__ BinGeom(const BhtDev &t, int bin, int kscale) : BinGeom(bin) {
#pragma unroll
    for (int d = 0; d < 3; ++d) org[d] = t.activeKeys[3 * (size_t)block + d] * (SIDE / kscale) + o[d];
  }
};

// arena node (x,y,z) of a bin -> (neighbour slot 0..7, cell id) in the grid block layout
template <int SIDE> __device__ __forceinline__ void arena_to_grid(const int (&o)[3], int x, int y, int z, int &slot, int &cell) {
  const int gx = o[0] + x, gy = o[1] + y, gz = o[2] + z;
  slot = ((gx >= SIDE) << 2) | ((gy >= SIDE) << 1) | (gz >= SIDE);
  cell = ((gx & (SIDE - 1)) * SIDE + (gy & (SIDE - 1))) * SIDE + (gz & (SIDE - 1));
}

// grid A -> the velocity arena of a bin (6^3 nodes x 3 channels, zero where the node's block is not in the partition); threads 0..215 of
// the workgroup, one node each.  nbr: [nblocks][8] blocks at offsets {0,1}^3
template <int SIDE>
__device__ __forceinline__ void arena_gather_velocities(const BinGeom<SIDE> &geo, const int *nbr, const float *gridA, float *varena, int tid) {
  using AL = ArenaLds;
  constexpr int NC = SIDE * SIDE * SIDE;
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

// the P2G arena of a bin (6^3 nodes x 7 channels) -> grid B: one global float atomic per non-zero value; threads 0..215.  *lostFlag is
// set if a node whose block is not in the partition has mass: the partition no longer covers the particles
template <int SIDE>
__device__ __forceinline__ void arena_flush_to_grid(const BinGeom<SIDE> &geo, const int *nbr, const float *parena, float *gridB, int *lostFlag,
                                                    int tid) {
  using AL = ArenaLds;
  constexpr int NC = SIDE * SIDE * SIDE;
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
      *lostFlag = 1;
    }
  }
}

// round-robin walk of one bin: round r visits the r-th particle of every cell (lane) that has one; the lanes
// that take part in a round read consecutive particles (coalesced), the index needs only ballots on the counts,
// so the loads of round r+1 can be issued before round r is computed (software pipelining: with ~220 VGPRs only
// two waves share a SIMD and memory latency must be hidden inside the wave).
struct RoundWalk {
  unsigned cnt, r = 0;
  int base;
  unsigned long long lt;
  __device__ __forceinline__ RoundWalk(unsigned cnt_, int start) : cnt(cnt_), base(start), lt(lanemask_lt()) {}
  // returns whether this lane has a particle in the next round; any = some lane has
  __device__ __forceinline__ bool next(int &i, bool &any) {
    const bool has = cnt > r;
    const unsigned long long m = __ballot(has);
    any = m != 0ull;
    i = base + __popcll(m & lt);
    base += __popcll(m);
    ++r;
    return has;
  }
};
template <int MODEL, int LW> struct RecB {  // sweep B inputs: x, F (, logJp) -- or x, cached P F^T vol; fluid: x, J, C
  float pos[3], F[9], logJp;
  float C[model_is_fluid(MODEL) ? 9 : 1];
  __device__ __forceinline__ void load(const ParticlesDev &ps, size_t i) {
    const POff<LW> o = particle_offset<LW>(ps.pos.chns, i);
    pload<LW, 3>(ps.pos, o, pos);
    if constexpr (MODEL == MPM_CACHED_STRESS) {
      float S[STRESS_N];
      pload<LW, STRESS_N>(ps.stress, o, S);
      stress_unpack(S, F);
    } else pload_state<LW, model_is_fluid(MODEL)>(ps.F, o, F);
    if constexpr (model_uses_logjp(MODEL)) logJp = pload1<LW>(ps.logJp, o);
    if constexpr (MODEL == ZS_MPM_EQUATION_OF_STATE) pload<LW, 9>(ps.C, o, C);  // P2G sweep only (G2P recomputes C)
  }
};

// ======================================================================================= G2P
// constitutive update for the NEXT P2G, fused into the tail of G2P where the VALU is otherwise idle (G2P is HBM-bound, P2G
// is VALU-bound by the SVD): stress(F_new, logJp) -> particles.stress (P F^T vol, unscaled), logJp updated.  Exactly what the
// next P2G would compute from the same F (P2G.hpp:60-101); SMODEL < 0: disabled.
template <int SMODEL, int LW = 0, bool NT = false>
__device__ __forceinline__ void update_stress(const MpmDev &mp, const ParticlesDev &ps, POff<LW> o, float (&F)[9], const float (&C)[9]) {
  if constexpr (SMODEL >= 0) {
    float PF[9], Fl[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) Fl[d] = F[d];  // the plastic models project their local copy only
    float lj = 0.f;
    if constexpr (model_uses_logjp(SMODEL)) lj = pload1<LW>(ps.logJp, o);
    model_stress<SMODEL>(mp.mat, lj, Fl, PF, C);
    if constexpr (model_uses_logjp(SMODEL)) pstore1<LW, NT>(ps.logJp, o, lj);
    float S[STRESS_N];
    stress_pack(PF, S);
    pstore<LW, STRESS_N, NT>(ps.stress, o, S);
  }
}

template <int SIDE, int SMODEL, int LW = 0, bool NT = false>
__device__ __forceinline__ void g2p_finish_loaded(const MpmDev &mp, const ParticlesDev &ps, size_t i, float (&pos)[3], const float (&oldF)[9],
                                                  const float (&vel)[3], const float (&C)[9]) {
  const POff<LW> o = particle_offset<LW>(ps.pos.chns, i);
#pragma unroll
  for (int d = 0; d < 3; ++d) pos[d] += vel[d] * mp.dt;
  float F[9];
  advance_state<model_is_fluid(SMODEL)>(oldF, C, mp.dt, F);
  pstore_state<LW, model_is_fluid(SMODEL), NT>(ps.F, o, F);
  pstore<LW, 3, NT>(ps.pos, o, pos);
  pstore<LW, 3, NT>(ps.vel, o, vel);
  pstore<LW, 9, NT>(ps.C, o, C);
  update_stress<SMODEL, LW, NT>(mp, ps, o, F, C);
}
template <int SIDE, int SMODEL>
__device__ __forceinline__ void g2p_finish(const MpmDev &mp, const ParticlesDev &ps, size_t i, float (&pos)[3], const float (&vel)[3],
                                           const float (&C)[9]) {
  float oldF[9];
  load_state<model_is_fluid(SMODEL)>(ps.F, i, oldF);
  g2p_finish_loaded<SIDE, SMODEL>(mp, ps, i, pos, oldF, vel, C);
}

template <int SIDE, int SMODEL>
__device__ __forceinline__ void g2p_gather_global(const MpmDev &mp, const ParticlesDev &ps, size_t i, const BhtDev &t, const float *grid,
                                                  float D_inv) {
  constexpr int NC = SIDE * SIDE * SIDE;
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
  float vel[3] = {0.f, 0.f, 0.f}, C[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
        float vi[3] = {0.f, 0.f, 0.f};
        if (bn >= 0) {
          const float *g = grid + (size_t)bn * 7 * NC + ((x & (SIDE - 1)) * SIDE + (y & (SIDE - 1))) * SIDE + (z & (SIDE - 1));
          vi[0] = g[1 * NC];
          vi[1] = g[2 * NC];
          vi[2] = g[3 * NC];
        }
        const float xi[3] = {(float)a * mp.dx - ar.lp[0], (float)b * mp.dx - ar.lp[1], (float)c * mp.dx - ar.lp[2]};
        float W = ar.w[0][a];
        W *= ar.w[1][b];
        W *= ar.w[2][c];
#pragma unroll
        for (int d = 0; d < 3; ++d) vel[d] += vi[d] * W;
#pragma unroll
        for (int d = 0; d < 9; ++d) C[d] += W * vi[d % 3] * xi[d / 3] * D_inv;
      }
  g2p_finish<SIDE, SMODEL>(mp, ps, i, pos, vel, C);
}

// v = sum W v_i and B = sum W v_i (xi - xp)^T over the 27 node velocities of the particle's cell, read from an LDS arena (81
// ds_read per particle), by sum factorisation over z, then y, then x (W = wx wy wz): ~290 VALU ops instead of ~1000 for the
// node-by-node form of G2P.hpp:54-66 (same sums, different association).  The fused kernel is VALU-bound and needs the 81 VGPRs a
// register-resident copy would cost for its P2G stencil.
template <class AL>
__device__ __forceinline__ void g2p_gather_lds(const MpmDev &mp, const Arena &ar, const float *a0, float D_inv, float (&vel)[3],
                                               float (&C)[9]) {
  float xz[3], xy[3], xx[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xx[k] = ar.w[0][k] * node_off(mp.dx, k, ar.lp[0]);
    xy[k] = ar.w[1][k] * node_off(mp.dx, k, ar.lp[1]);
    xz[k] = ar.w[2][k] * node_off(mp.dx, k, ar.lp[2]);
  }
  float B[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
#pragma unroll
  for (int j = 0; j < 3; ++j) vel[j] = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float t0[3] = {0.f, 0.f, 0.f}, t1[3] = {0.f, 0.f, 0.f}, t2[3] = {0.f, 0.f, 0.f};
    // the slab's 27 node values first, then the arithmetic: one LDS latency per slab instead of one per pair of reads
    float nv[3][3][3];
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
      const float *g = a0 + AL::at(a, bb, 0);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        nv[bb][j][0] = g[j * AL::CH];
        nv[bb][j][1] = g[j * AL::CH + 1];
        nv[bb][j][2] = g[j * AL::CH + 2];
      }
    }
    asm volatile("" ::: "memory");  // (keeps the compiler from sinking the reads back between the fmas)
#pragma unroll
    for (int bb = 0; bb < 3; ++bb) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float v0 = nv[bb][j][0], v1 = nv[bb][j][1], v2 = nv[bb][j][2];
        const float s0 = fmaf(ar.w[2][2], v2, fmaf(ar.w[2][1], v1, ar.w[2][0] * v0));
        const float s1 = fmaf(xz[2], v2, fmaf(xz[1], v1, xz[0] * v0));
        t0[j] = fmaf(ar.w[1][bb], s0, t0[j]);
        t1[j] = fmaf(xy[bb], s0, t1[j]);
        t2[j] = fmaf(ar.w[1][bb], s1, t2[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      vel[j] = fmaf(ar.w[0][a], t0[j], vel[j]);
      B[j][0] = fmaf(xx[a], t0[j], B[j][0]);
      B[j][1] = fmaf(ar.w[0][a], t1[j], B[j][1]);
      B[j][2] = fmaf(ar.w[0][a], t2[j], B[j][2]);
    }
  }
#pragma unroll
  for (int d = 0; d < 9; ++d) C[d] = B[d % 3][d / 3] * D_inv;
}

}  // namespace zsr
