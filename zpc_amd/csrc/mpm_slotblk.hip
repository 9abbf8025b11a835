// mpm_slotblk.hip -- the fused G2P2G step on slotted storage with ONE WORKGROUP PER 8^3 GRID BLOCK (r05).
//
// Why.  g2p2g_slot_kernel (mpm_slotted.hip) gives every bin (4^3 cells, ~512 particles = 1.9 chunks of 256) a workgroup of its own: a
// producer -> consumer pipeline that is filled and drained once per bin, in front of it a head (occupancy words, entry table, velocity
// arena: three dependent memory round trips) and behind it a tail (arena flush, grid atomics).  The cycle stamps of that kernel
// (profiles/r05_slot_probe.md) put head + drain + flush + tail at half of a workgroup's life; the two workgroups of a CU overlap them only by
// chance.  Here the 8 bins of a block are one pipeline:
//   * the chunk sequence runs through all bins of the block (bin 0 chunk 0, bin 0 chunk 1, bin 1 chunk 0, ...): producers prefetch the
//     records of chunk g + 1 -- whichever bin it belongs to -- while they compute chunk g; the consumers flush a bin's accumulators and
//     send its arena to the grid while the producers are already in the next bin.  Fill and drain are paid once per block;
//   * head once per block: the occupancy words of all 8 bins in one load, ONE velocity arena of 10^3 nodes for the whole block
//     (12 KB; the bins' own 6^3 arenas overlap by half);
//   * the staging ring holds ONE chunk (+ the group a round may straddle): 5 groups of 64 records instead of 9 (35 KB, which is what pays
//     for the block arena).  A producer waits, right before it stages, until all four consumers have counted the previous chunk done (an
//     LDS counter, no barrier: the consumers finish a chunk in half the time the producers need for the next); one barrier per chunk
//     hands the staged chunk over;
//   * per-bin state (entry table, tickets, departures, outbox count, neighbour bins) is double-buffered by bin parity and kept by the
//     CONSUMER waves, which have the time: the entry table of a bin is built three chunks ahead, its neighbour bins two chunks ahead,
//     a finished bin's departures are written out with its last chunk (blk_consumer spells out when each buffer is free); everything
//     the loops need to know about a chunk sits in one packed word (ChunkDesc), read once per iteration into SGPRs;
//   * (r07) the ticket counters of all eight bins live for the whole workgroup (s_arrLocal[8][64]): a mover into another bin of the
//     block takes its new slot here (slot_produce_entry, INBLK) instead of an outbox record and a slot_rehome_kernel ticket -- about
//     half of all cross-bin movers.  The arrivals per cell (claim words, high half) are written once, after the block's last barrier;
//   * 128 VGPRs and NO scratch: the uniform constants of the per-particle code come from the host (MpmDev::dxi, D_inv, fscale;
//     Material::smu, dpCoef, expCohesion -- kernel arguments live in SGPRs), one producer body serves the four producer waves.  On gfx9
//     loads and stores share vmcnt, so a spill reload inside the chunk loop waits for the record prefetch of the next chunk and for the
//     particle stores just issued (profiles/r05_block_kernel.md, section 7; tests/test_host_cpu.py keeps it that way);
//   * the bin's P2G arena has 8^3 nodes (ArenaBin8): a mover into a neighbour bin adds its 27 node terms there (plain LDS
//     read-add-write) and they reach the grid with the bin's one flush -- no global atomics per mover.  ONE consumer wave (LIST_CS, the
//     set with one accumulator per node) scatters a chunk's list for all seven channels: decode, weights, arena offset and face bits
//     once per entry instead of once per set (91 VALU per pass of two entries against 247 over the four waves).  The other consumers
//     wait at a bin's end, on an LDS word, until that wave has finished the bin's last list; the barrier that hands the next bin's
//     first chunk over keeps its list behind their flush (blk_consumer; profiles/block_list.md);
//   * the flush visits what can be non-zero, not the 512 nodes: the 6^3 core the register planes write (4 dense passes) and those 8 x 8
//     faces of the shell a list entry of the bin has reached (a 6-bit mask kept while the lists are scattered; none at rest).  Every LDS
//     read of a pass is issued before the first is used, and a pass writes zero over what it read: the arena is cleared once per
//     workgroup, never per bin (blk_flush_nodes and the bin end of blk_consumer; profiles/block_flush.md).
//   * the step call's grid reset rides here: with SlotArgs::gridClear set, every workgroup writes zero over its own block of a third grid,
//     the NEXT step's target, as the last thing it does (blk_clear_block; an empty block at its early exit) -- three grids rotate and no
//     memset stands in front of the step's first workgroup (dist.hip, profiles/grid_rotation.md).
// The per-particle code (slot_produce_entry), the consumers' accumulation (g2p2g_consume_set), the mover protocol, slot_rehome_kernel
// and slot_commit_kernel are those of mpm_slotted.hip; results differ only in summation order.
#include "mpm_slot.hpp"
// -DZS_SLOTBLK_CHECK_ARENA (a measurement build: tools/ab_build.sh check "-DZS_SLOTBLK_CHECK_ARENA" mpm_slotblk.hip, selected with
// ZS_ROCM_LIB) asserts after every bin's flush that the flushing wave's channels of the arena are all zero.  Never in the product build.
#ifdef ZS_SLOTBLK_CHECK_ARENA
#include <cassert>
#endif

namespace zsr {

constexpr int SB_NG = 5;       // ring: the four groups of a chunk + the group a straddling round keeps alive
constexpr int SB_MAXCH = 64;   // chunks per block: 8 bins x (32 rounds x 64 cells / 256)
constexpr int LIST_CS = 3;     // the consumer wave that scatters the chunks' lists: one accumulator per node, the most free registers

struct SubGeom {  // what the shared scatter helpers need of a bin: origin inside the block, origin in world cells
  int o[3], org[3];
};
__device__ __forceinline__ SubGeom sub_geom(const int (&borg)[3], int b) {
  SubGeom g;
  g.o[0] = ((b >> 2) & 1) * 4;
  g.o[1] = ((b >> 1) & 1) * 4;
  g.o[2] = (b & 1) * 4;
#pragma unroll
  for (int d = 0; d < 3; ++d) g.org[d] = borg[d] + g.o[d];
  return g;
}

struct BlkShared {
  float *varena, *parena, *stage;
  unsigned long long *smask;
  unsigned short (*tab)[SL_KMAX * 64];       // [2]
  unsigned (*masks)[64];                     // [8]
  unsigned (*clr)[64];                       // [2]
  unsigned (*arrLocal)[64];                  // [8]: ticket counters of the block's bins, for the whole step (in-block movers)
  unsigned (*arrCnt)[64];                    // [3]
  unsigned short (*arrQ)[64][SL_ARRQ];       // [3]
  unsigned *xCnt;                            // [3]
  unsigned (*xq)[SL_XQ];                     // [3]
  int *nbrBlk, (*nbrBin)[27], *nbr8;
  int (*cnt)[4];                             // [2]: outCount, sent, homed, xOver of the bin of that parity
  int *oc;                                   // [8] per bin: outbox records (after the bin has been finished)
  const unsigned *desc;                      // [SB_MAXCH + 5] desc[g + 1] = packed descriptor of chunk g (ChunkDesc), zero outside [0, G)
  unsigned *done;                            // consumer waves x chunks consumed
  unsigned *listDone;                        // chunks whose list the list wave has scattered into the bin's arena
  unsigned *faces;                           // [2] by bin parity: faces of the arena's shell the bin's lists have reached (blk_xlist_lds)
  int *sums;                                 // [0] sent, [1] homed, [2] bins whose outbox holds records that still have to be scattered
};

// Everything the chunk loop needs to know about a chunk, in one word: the loops read desc[g .. g + 3] (chunks g - 1 .. g + 2) in ONE LDS access
// and keep the fields in SGPRs.  (Read field by field -- chBin[g], then binQ / total / gbase / nch of that bin, for three chunks -- the top of
// a producer iteration was ~20 dependent LDS round trips behind the consumers' traffic: 4.1 k of its 17 k cycles, r05 stamps.)
struct ChunkDesc {
  unsigned w;
  __device__ static unsigned pack(int b, int c, int qp, bool last, int total, int gbase) {
    return (unsigned)b | ((unsigned)c << 3) | ((unsigned)(qp & 1) << 7) | ((unsigned)last << 8) | ((unsigned)total << 9) | ((unsigned)gbase << 21) | (1u << 31);
  }
  __device__ int bin() const { return (int)(w & 7u); }             // bin of the block
  __device__ int idx() const { return (int)((w >> 3) & 15u); }     // chunk number inside the bin
  __device__ int qp() const { return (int)((w >> 7) & 1u); }       // parity of the bin among the block's non-empty bins
  __device__ bool last() const { return (w >> 8) & 1u; }           // last chunk of its bin
  __device__ int total() const { return (int)((w >> 9) & 4095u); } // occupied slots of the bin
  __device__ int gbase() const { return (int)((w >> 21) & 127u); } // number of the bin's first chunk
};
template <int N> __device__ __forceinline__ void blk_chunk_descs(const unsigned *desc, int g, ChunkDesc (&d)[N]) {  // d[k] = chunk g - 1 + k
#pragma unroll
  for (int k = 0; k < N; ++k) d[k].w = desc[g + k];
#pragma unroll
  for (int k = 0; k < N; ++k) d[k].w = (unsigned)__builtin_amdgcn_readfirstlane((int)d[k].w);
}

// entry table of one bin: round-major enumeration of its occupied slots; wave w of nw writes the rows of rounds = w mod nw
__device__ __forceinline__ void blk_build_tab(unsigned mask, int lane, int w, int nw, unsigned short *tab) {
  const unsigned long long lt = lanemask_lt();
  int total = 0;
#pragma unroll 1
  for (int r = 0; r < SL_KMAX; ++r) {  // (ballots only: no cross-lane data movement, nothing that waits for the record loads in flight)
    if (__ballot((mask >> r) != 0u) == 0ull) break;
    const bool has = (mask >> r) & 1u;
    const unsigned long long occ = __ballot(has);
    if ((r % nw) == w && has) tab[total + __popcll(occ & lt)] = (unsigned short)(r * 64 + lane);
    total += __popcll(occ);
  }
}

// a finished bin (all of its chunks produced by all producer waves): departures of its cells for slot_rehome_kernel / slot_commit_kernel,
// its outbox count; the parity's counters are zero again (its arrivals can still grow: the kernel writes them after its last barrier).  One wave, lane = cell; every LDS read is issued before the
// first use (ONE round trip: as a chain of lane-0 reads this was 4.9 k cycles per bin on the producers' critical path, r05 stamps).
__device__ __forceinline__ void blk_finish_bin(const BlkShared &sh, const SlotArgs &A, int bin0, int b, int qp, int lane) {
  const int bin = bin0 + b;
  const unsigned c = sh.clr[qp][lane];
  const int cv = sh.cnt[qp][lane & 3];  // outCount, sent, homed, xOver
  if (c) A.claim[((size_t)A.nbinsAll + (size_t)bin) * 64 + lane] = c;
  sh.clr[qp][lane] = 0u;
  const int c0 = __builtin_amdgcn_readlane(cv, 0), c1 = __builtin_amdgcn_readlane(cv, 1), c2 = __builtin_amdgcn_readlane(cv, 2),
            c3 = __builtin_amdgcn_readlane(cv, 3);
  if (lane == 0) {
    const int oc = c0 < A.cap ? c0 : A.cap;
    A.moverCount[bin] = oc;
    sh.oc[b] = oc;
  }
  if (lane < 3) {  // sums: sent, homed, bins whose outbox holds records that still have to be scattered (one bit per bin: + is |)
    const int add = lane == 0 ? c1 : (lane == 1 ? c2 : (c3 > 0 ? 1 << b : 0));
    if (add) atomicAdd(&sh.sums[lane], add);
  }
  if (lane < 4) sh.cnt[qp][lane] = 0;
}

// P2G arena of ONE bin in the block kernel: 8^3 nodes = the bin's 6^3 stencil nodes + one layer around them, origin at the bin's node -1.
// A mover whose new cell lies in a neighbour bin (base node -1 .. 4 per axis) has its 27 nodes inside, so its grid terms are added HERE
// (plain LDS read-add-write) and reach the grid with the bin's one flush -- instead of 189 global float atomics per mover (0.4 ms and
// 1.8 GB of write-through sectors per step of the 64 Mi-particle column).  Strides: for a fixed stencil offset the 64 cells of a bin land
// on 32 distinct banks per 32-lane half (z + 8 y + 68 x: x adds 4 mod 32).
struct ArenaBin8 {
  static constexpr int W = 8;
  static constexpr int SY = 8, SX = 68, CH = W * SX;
  __device__ static constexpr int at(int x, int y, int z) { return x * SX + y * SY + z; }
};

// The chunk's list (movers into neighbour bins, arrival-queue overflow, stayers whose local position rounded onto 1.5): ALL SEVEN grid
// channels of their 27 node terms into the bin's 8^3 arena `parena`, by ONE wave (the consumer of set 3, blk_consumer).  Two list entries
// per pass, lane = (entry parity, stencil node): the entry's decode, its three axis weights, the node's arena offset and the face bits
// are formed once and serve seven values and seven read-add-writes (the seven reads of a half issued together).  The two entries of a
// pass may share nodes, so the halves do their read-add-write one after the other (LDS operations of a wave execute in order).
// Weights and values: StencilNodeLane, as slot_xlist_scatter -- term by term what the four per-set passes of this list added before
// (profiles/block_list.md), in the same order.
// `faces` (per lane, ORed): the faces of the arena's shell the entries of this lane reach -- bit 2 d: node 0 of the stencil sits on arena
// coordinate 0 of axis d (the entry's coordinate is 0), bit 2 d + 1: node 2 sits on coordinate 7 (the entry's coordinate is 5).
__device__ __forceinline__ void blk_xlist_lds(const float *stage, const unsigned *xq, int nx, int lane, float *parena, unsigned &faces) {
  using A8 = ArenaBin8;
  const int node = lane & 31, half = lane >> 5;
  if (nx <= 0) return;
  const StencilNodeLane sn(node);
#pragma unroll 1
  for (int k0 = 0; k0 < nx; k0 += 2) {
    const int k = k0 + half;
    const bool act = node < 27 && k < nx;
    float val[7];
    int an = 0;
    if (act) {
      const unsigned e = xq[k];
      const float *st = stage + (size_t)((e & 1023u) >> 6) * (G2P2G_QF * 64) + (e & 63u);
      float Wt = 1.f;
#pragma unroll
      for (int q = 0; q < 3; ++q) Wt *= sn.weight(q, st[(1 + q) * 64]);
      // (the entry carries new cell + 1 per axis = the arena coordinate of the stencil's node 0)
      const int ex = (int)((e >> 10) & 7u), ey = (int)((e >> 13) & 7u), ez = (int)((e >> 16) & 7u);
      an = A8::at(ex + sn.sel[0], ey + sn.sel[1], ez + sn.sel[2]);
      faces |= (ex == 0 ? 1u : 0u) | (ex == 5 ? 2u : 0u) | (ey == 0 ? 4u : 0u) | (ey == 5 ? 8u : 0u) | (ez == 0 ? 16u : 0u) | (ez == 5 ? 32u : 0u);
      sn.values(st, Wt, val);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (act && half == h) {
        float a[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) a[q] = parena[q * A8::CH + an];
#pragma unroll
        for (int q = 0; q < 7; ++q) parena[q * A8::CH + an] = a[q] + val[q];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
  }
}

// The flush of a bin's arena (this wave's channels, `pa`) to grid B, NP passes of 64 nodes at once: node p of a lane sits at arena offset
// aoff[p], node (gx, gy, gz)[p] in cells of this block (-1 .. 10 per axis).  Every LDS read of the NP passes -- the nodes' blocks and their
// NA values -- is issued before the first is used (one round trip, none waits for another); the nodes are then written back as zero, so
// the arena is clear again where it was read, and the non-zero values go to the grid, one float atomic each.  A node whose block is not in
// the partition and that has mass is reported (status[2]).  CORE: no node lies below the block (gx, gy, gz >= 0).
template <int CS, int NP, bool CORE>
__device__ __forceinline__ void blk_flush_nodes(float *pa, const int (&aoff)[NP], const int (&gx)[NP], const int (&gy)[NP], const int (&gz)[NP],
                                                const int *nbrBlk, const SlotArgs &A) {
  using S = ConsumerSet<CS>;
  constexpr int NC = 512;
  int bn[NP];
  float v[NP][S::NA];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    auto side = [](int g) { return !CORE && g < 0 ? 0 : (g >= 8 ? 2 : 1); };
    bn[p] = nbrBlk[(side(gx[p]) * 3 + side(gy[p])) * 3 + side(gz[p])];
#pragma unroll
    for (int q = 0; q < S::NA; ++q) v[p][q] = pa[q * ArenaBin8::CH + aoff[p]];
  }
  asm volatile("" ::: "memory");  // (keeps the compiler from sinking the reads to their uses)
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int q = 0; q < S::NA; ++q) pa[q * ArenaBin8::CH + aoff[p]] = 0.f;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (bn[p] >= 0) {
      float *gq = A.gridB + ((size_t)bn[p] * 7 + S::CH0) * NC + (((gx[p] & 7) * 8 + (gy[p] & 7)) * 8 + (gz[p] & 7));
#pragma unroll
      for (int q = 0; q < S::NA; ++q)
        if (v[p][q] != 0.f) unsafeAtomicAdd(gq + q * NC, v[p][q]);
    } else if (S::MASS && v[p][0] != 0.f) {
      A.status[2] = 1;  // mass for a node whose block is not in the partition
    }
  }
}

// producer wave W (0..3): entries [64 (4 c + W), +64) of every chunk c of every bin of the block.  W is a wave-uniform RUNTIME value: one
// copy of the 17 KB producer body for the four waves (as a template parameter the kernel carried four: 87 KB of code, 70 KB of it hot in
// every chunk -- more than the instruction cache two CUs share)
template <int SMODEL, bool WRITE_ALL>
__device__ __forceinline__ void blk_producer(const MpmDev &mp, const ParticlesDev &ps, const int (&borg)[3], int blk, int lane, int G,
                                             const BlkShared &sh, const SlotArgs &A, const int W) {
  constexpr int LW = 64;
  constexpr bool DP = model_uses_logjp(SMODEL);
  constexpr bool FLUID = model_is_fluid(SMODEL);
  const int bin0 = blk * 8;
  const unsigned kmask = A.K >= 32 ? 0xffffffffu : ((1u << A.K) - 1u);
  RecG<LW, DP, FLUID> cur, nxt;
  bool has0 = false, has1 = false;
  unsigned code0 = 0, code1 = 0;  // round * 64 + cell of the entry (its element index is rebuilt from it where needed: two VGPRs less across the loop)
  auto elem = [&](int b, unsigned code) { return ((size_t)(bin0 + b) * (size_t)A.K + (size_t)(code >> 6)) * 64 + (size_t)(code & 63u); };
  {
    ChunkDesc d[2];
    blk_chunk_descs(sh.desc, 0, d);
    const int b = d[1].bin();
    const int j = 64 * W + lane;
    has1 = j < d[1].total();
    if (has1) {
      code1 = sh.tab[d[1].qp()][j];
      nxt.load(ps, elem(b, code1));
    }
  }
  __syncthreads();  // every producer has read the first bin's entry table (iteration 0 may rebuild that buffer for the bin of chunk 2)
  for (int g = 0; g < G; ++g) {
    ChunkDesc d[3];  // chunks g - 1, g, g + 1
    blk_chunk_descs(sh.desc, g, d);
    const int b = d[1].bin();
    const int qp = d[1].qp();
    const int grp = 4 * g + W, slot = grp % SB_NG, par = g % 3;
    float *myStage = sh.stage + (size_t)slot * (G2P2G_QF * 64);
    cur = nxt;
    has0 = has1;
    code0 = code1;
    has1 = false;
    if (g + 1 < G) {  // the records of the next chunk (this bin's or the next bin's): in flight during this chunk
      const int b1 = d[2].bin();
      const int j1 = 256 * d[2].idx() + 64 * W + lane;
      has1 = j1 < d[2].total();
      if (has1) {
        code1 = sh.tab[d[2].qp()][j1];
        nxt.load(ps, elem(b1, code1));
      }
    }
    // (per-bin state around the bin boundaries -- a finished bin's counters, the next bins' entry tables and neighbour bins -- is kept by the
    // consumer waves, which have the time: see blk_consumer)
    const SubGeom sg = sub_geom(borg, b);
    const SlotBinView bv{bin0 + b, {sg.org[0], sg.org[1], sg.org[2]}, (size_t)(bin0 + b) * (size_t)A.K, kmask,
                         sh.varena + ArenaBlk::at(sg.o[0], sg.o[1], sg.o[2]), sh.masks[b], sh.clr[qp], sh.arrLocal[b], sh.nbrBin[qp],
                         &sh.cnt[qp][0], &sh.cnt[qp][1], &sh.cnt[qp][2], &sh.cnt[qp][3], sh.arrLocal, sh.masks};
    // the ring slot this wave stages into was last read by the consumers of chunk g - 1 (its groups 0..2, or the straddle group of
    // chunk g - 2, consumed with chunk g - 1): all four consumer waves have counted that chunk done
    auto ringFree = [&] {
      while (__hip_atomic_load(sh.done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 4u * (unsigned)g) __builtin_amdgcn_s_sleep(2);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    bool valid = false;
    if (has0)
      valid = slot_produce_entry<8, SMODEL, WRITE_ALL, ArenaBlk, true>(mp, ps, cur, code0, elem(b, code0), lane, (unsigned)(slot * 64 + lane), myStage + lane, bv, A,
                                                                 sh.arrCnt[par], sh.arrQ[par], &sh.xCnt[par], sh.xq[par], ringFree);
    ringFree();
    {
      const unsigned long long vm = __ballot(valid);
      if (lane == 0) sh.smask[slot] = vm;
    }
    __syncthreads();  // chunk g is staged
  }
  __syncthreads();  // the consumers have accumulated the last chunk and flushed the last bin
}

// consumer wave of channel set CS: lane = cell of the current bin; chunk g is consumed while the producers work on chunk g + 1
template <int CS>
__device__ __forceinline__ void blk_consumer(const MpmDev &mp, const int (&borg)[3], int blk, int lane, int G, const BlkShared &sh, const SlotArgs &A) {
  using S = ConsumerSet<CS>;
  using AL = ArenaBin8;
  const int cx = lane >> 4, cy = (lane >> 2) & 3, cz = lane & 3;
  const unsigned long long lt = lanemask_lt();
  const float *const stage = sh.stage;
  float *const pa = sh.parena + (size_t)S::CH0 * AL::CH;  // this wave's channels of the bin's arena
  float acc[27][S::NA];
#pragma unroll
  for (int k = 0; k < 27; ++k)
#pragma unroll
    for (int q = 0; q < S::NA; ++q) acc[k][q] = 0.f;
  unsigned mask = 0u;
  unsigned faces = 0u;  // (list wave) faces of the arena's shell the lists of the current bin have reached (blk_xlist_lds)
  int r = 0, off = 0;  // next round to consume, entry number of its first particle
  // The bin's arena (this wave's channels) is cleared HERE, once: every flush leaves it all zero again (see the bin end below), and the
  // padding of the 68-float stride is never written.
  for (int k = lane; k < S::NA * AL::CH; k += 64) pa[k] = 0.f;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __syncthreads();  // (the producers' first record requests are out)
  // Per-bin state, kept by the consumers (off the producers' critical path; every buffer named here is dead for its previous owner, see the
  // file comment).  In iteration g, i.e. between the barriers "chunk g staged" and "chunk g + 1 staged", while the producers work on
  // chunk g + 1:
  //   * entry table of the bin that starts with chunk g + 3 (its first records are requested at the top of the producers' iteration g + 2;
  //     the table of the bin two bins earlier, same parity, was last read at the top of their iteration g at the latest), all four waves;
  //   * neighbour bins of the bin that starts with chunk g + 2 (used by the producers from their iteration g + 2 on), wave of set 2;
  //   * the counters of the bin that ENDS with chunk g (all of it was produced before the barrier "chunk g staged"; the parity's next
  //     owner starts with chunk g + 2 at the earliest), wave of set 3.
  // The kernel head has done the bins that start with chunks 0 and 1; the one that starts with chunk 2 is "iteration -1", here.
  auto binState = [&](int g, const ChunkDesc &c2, const ChunkDesc &c3) {  // c2 / c3: chunks g + 2 / g + 3
    if (g + 3 < G && c3.idx() == 0) blk_build_tab(sh.masks[c3.bin()][lane], lane, CS, 4, sh.tab[c3.qp()]);
    if (CS == 2 && g >= 0 && g + 2 < G && c2.idx() == 0 && lane < 27) sh.nbrBin[c2.qp()][lane] = neighbour_bin8(sh.nbrBlk, blk, c2.bin(), lane);
  };
  {
    ChunkDesc d[5];
    blk_chunk_descs(sh.desc, -1 + 1, d);  // chunks -1 .. 3
    binState(-1, d[2], d[3]);
  }
  for (int g = 0; g < G; ++g) {
    __syncthreads();  // chunk g is staged
    ChunkDesc d[5];  // chunks g - 1 .. g + 3
    blk_chunk_descs(sh.desc, g, d);
    const int b = d[1].bin(), c = d[1].idx(), total = d[1].total(), par = g % 3;
    const int gb = 4 * d[1].gbase();  // ring group number of the bin's entry 0
    if (c == 0) {
      r = 0;
      off = 0;
      mask = sh.masks[b][lane];
    }
    const int produced = 256 * (c + 1) < total ? 256 * (c + 1) : total;
    const unsigned qn = sh.arrCnt[par][lane];
    const int na = qn < (unsigned)SL_ARRQ ? (int)qn : SL_ARRQ;
    int ai = 0;
    if (CS == 0) sh.arrCnt[(g + 2) % 3][lane] = 0u;  // the counters chunk g + 2 will use (last read with chunk g - 1, which every consumer has left)
#pragma unroll 1
    for (;;) {
      bool roundOk = false, has = false;
      unsigned long long occ = 0ull;
      int cnt = 0;
      if (off < total) {
        has = (mask >> r) & 1u;
        occ = __ballot(has);
        cnt = __popcll(occ);
        roundOk = off + cnt <= produced;  // else: the round's last entries belong to the chunk in production
      }
      const bool pend = ai < na;
      if (!roundOk && __ballot(pend) == 0ull) break;
      int spos = -1;
      if (roundOk) {
        if (has) {
          const int e = off + __popcll(occ & lt);
          const int slot = (gb + (e >> 6)) % SB_NG, pos = e & 63;
          if ((sh.smask[slot] >> pos) & 1ull) spos = slot * (G2P2G_QF * 64) + pos;
        }
        off += cnt;
        ++r;
      }
      if (spos < 0 && pend) {  // a lane without a particle of its own in this round takes an arrival
        const unsigned p = sh.arrQ[par][lane][ai++];
        spos = (int)(p >> 6) * (G2P2G_QF * 64) + (int)(p & 63u);
      }
      if (spos >= 0) g2p2g_consume_set<CS>(mp, stage, spos, acc);
    }
    if (CS == 0 && lane == 0) sh.xCnt[(g + 2) % 3] = 0u;  // (last read by the list wave with chunk g - 1)
    if (CS == LIST_CS) {
      // The chunk's list, all seven channels, by this wave alone.  It writes into channels the other three consumers flush, so:
      //   * bin end: a set wave adds its planes and flushes only after listDone has reached this chunk (below) -- an LDS word this wave
      //     alone writes, behind a release fence, like s_done; no barrier inside the chunk loop;
      //   * next bin: this wave's first write for the next bin comes behind the barrier "chunk g + 1 staged" at the top of the next
      //     iteration, which every set wave reaches only after it has flushed and zeroed this bin.  That barrier must stay in front of the list.
      const int nx = sh.xCnt[par] < (unsigned)SL_XQ ? (int)sh.xCnt[par] : SL_XQ;
      blk_xlist_lds(stage, sh.xq[par], nx, lane, sh.parena, faces);
      if (d[1].last()) {  // the faces of the shell the bin's lists have reached, for all four flushing waves (one word per bin parity)
        unsigned fm = 0u;
#pragma unroll
        for (int f = 0; f < 6; ++f) fm |= __ballot((faces >> f) & 1u) != 0ull ? 1u << f : 0u;
        faces = 0u;
        if (lane == 0) sh.faces[d[1].qp()] = fm;
      }
    }
    // this wave has read what it needs of chunk g: the producers may stage chunk g + 1 over it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) {
      if (CS == LIST_CS) __hip_atomic_store(sh.listDone, (unsigned)(g + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      atomicAdd(sh.done, 1u);
    }
    binState(g, d[3], d[4]);
    if (CS == 3 && d[1].last()) blk_finish_bin(sh, A, blk * 8, b, d[1].qp(), lane);
    if (d[1].last()) {
      // last chunk of the bin: once the list wave is through with it, the set's channels of the bin's arena belong to this wave alone
      // until the next bin's first barrier -- add the 27 register planes on top of the lists' terms (phases ordered inside the wave),
      // send the arena's nodes to the grid.
      //   * The register planes write the 6^3 CORE of the arena only (coordinates 1..6): it is flushed densely, 216 nodes in 4 passes
      //     (the 40 idle lanes of the last pass read and zero a padding word).  A bin sits at offset 0 or 4 of its block, so a core node
      //     lies in this block or in its +1 neighbour per axis.
      //   * The 296 nodes of the SHELL (a coordinate 0 or 7) are written by the lists alone: a term at coordinate 0 of an axis comes from
      //     node 0 of an entry whose coordinate on that axis is 0, a term at coordinate 7 from node 2 of an entry at coordinate 5 -- and
      //     every such entry has set that face's bit in `faces`.  So every shell node that can be non-zero lies on a flagged face; the
      //     flagged faces are flushed as 8 x 8 slabs, one pass each, and a bin without such movers (all of them at rest) flushes none.
      //     Edges and corners belong to several faces: the first visit leaves them zero, the later ones skip them.
      //   * Every pass writes zero over what it has read (LDS operations of a wave execute in order), so after the flush the wave's
      //     channels are all zero again -- core: every node visited; shell: zero unless flagged -- and the next bin's lists add into a
      //     clear arena without a clear loop of their own.
      if (CS != LIST_CS) {  // the list wave has finished the list of this chunk, the bin's last: its terms are in this wave's channels
        while (__hip_atomic_load(sh.listDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (unsigned)(g + 1)) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
      acc_to_arena<AL, true>(pa + AL::at(cx + 1, cy + 1, cz + 1), acc);  // (and the planes are zero again for the next bin)
      const SubGeom sg = sub_geom(borg, b);
      // (the lane number made opaque: the node offsets below depend on the lane alone, and hoisted out of the chunk loop they would be
      // a dozen registers carried across the accumulation -- the kernel has none to spare; recomputed per bin they cost ~60 VALU)
      int ln = lane;
      asm volatile("" : "+v"(ln));
      {
        int aoff[4], gx[4], gy[4], gz[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int n = ln + 64 * p;
          const int x = n / 36, y = (n / 6) % 6, z = n % 6;  // core node, 0..5 per axis
          const bool in = p < 3 || n < 216;
          aoff[p] = in ? AL::at(x + 1, y + 1, z + 1) : AL::at(0, 8, 0);  // (x = 0, word 64: padding, always zero)
          gx[p] = in ? sg.o[0] + x : 0;
          gy[p] = in ? sg.o[1] + y : 0;
          gz[p] = in ? sg.o[2] + z : 0;
        }
        blk_flush_nodes<CS, 4, true>(pa, aoff, gx, gy, gz, sh.nbrBlk, A);
      }
      unsigned fm = (unsigned)__builtin_amdgcn_readfirstlane((int)sh.faces[d[1].qp()]);  // (written by the list wave in front of listDone)
#pragma unroll 1
      while (fm) {
        const int f = __builtin_ctz(fm);
        fm &= fm - 1u;
        const int ax = f >> 1, fix = (f & 1) * 7, u = ln >> 3, v = ln & 7;  // lane = the face's two free coordinates
        const int x = ax == 0 ? fix : u, y = ax == 1 ? fix : (ax == 0 ? u : v), z = ax == 2 ? fix : v;
        const int aoff[1] = {AL::at(x, y, z)}, gx[1] = {sg.o[0] - 1 + x}, gy[1] = {sg.o[1] - 1 + y}, gz[1] = {sg.o[2] - 1 + z};
        blk_flush_nodes<CS, 1, false>(pa, aoff, gx, gy, gz, sh.nbrBlk, A);
      }
#ifdef ZS_SLOTBLK_CHECK_ARENA  // debug builds only (see the top of the file): the flush has left this wave's channels of the arena all zero
      for (int k = lane; k < S::NA * AL::CH; k += 64) assert(pa[k] == 0.f);
#endif
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next bin's lists add into the arena only after these writes)
    }
  }
  __syncthreads();  // the last bin is flushed
}

// The workgroup's own block of the grid that rotates in as the NEXT step's target (A.gridClear; NULL: the caller clears with a memset):
// 7 x 512 floats = 896 plain 16-byte stores over the 512 threads, fire and forget.  The grid is neither gathered from nor scattered into in
// this step and block `blk` of it belongs to this workgroup alone, so the kernel boundary is all the ordering there is.
// blockClear = the block's first float (NULL: nothing to clear).
__device__ __forceinline__ void blk_clear_block(float *blockClear, int tid) {
  if (!blockClear) return;
  float4 *const p = reinterpret_cast<float4 *>(blockClear);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  p[tid] = z;
  if (tid < 7 * 512 / 4 - 512) p[512 + tid] = z;
}

template <int SMODEL, bool WRITE_ALL>
static __global__ __launch_bounds__(512, 4) void g2p2g_slotblk_kernel(MpmDev mp, ParticlesDev ps, BhtDev t, SlotArgs A) {
  constexpr int NC = 512;
  __shared__ float s_varena[3 * ArenaBlk::CH];
  __shared__ float s_parena[7 * ArenaBin8::CH];
  __shared__ float s_stage[SB_NG * G2P2G_QF * 64];
  __shared__ unsigned long long s_smask[SB_NG];
  __shared__ unsigned short s_tab[2][SL_KMAX * 64];
  __shared__ unsigned s_masks[8][64];
  __shared__ unsigned s_clr[2][64], s_arrLocal[8][64], s_arrCnt[3][64];
  __shared__ unsigned short s_arrQ[3][64][SL_ARRQ];
  __shared__ unsigned s_xCnt[3], s_xq[3][SL_XQ];
  __shared__ int s_nbrBlk[27], s_nbrBin[2][27], s_nbr8[8];
  __shared__ int s_cnt[2][4];
  __shared__ int s_total[8], s_gbase[8], s_binQ[8], s_oc[8];
  __shared__ unsigned char s_chBin[SB_MAXCH], s_chIdx[SB_MAXCH];
  __shared__ unsigned s_desc[SB_MAXCH + 5];
  __shared__ unsigned s_done, s_listDone, s_faces[2];
  __shared__ int s_sums[3], s_G;
  __shared__ float *s_clear;  // this block of A.gridClear (NULL: none), parked here from the head to the tail of the kernel
  const BlkShared sh{s_varena, s_parena, s_stage, s_smask, s_tab, s_masks, s_clr, s_arrLocal, s_arrCnt, s_arrQ, s_xCnt, s_xq, s_nbrBlk, s_nbrBin, s_nbr8,
                     s_cnt, s_oc, s_desc, &s_done, &s_listDone, s_faces, s_sums};
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int blk = (int)blockIdx.x + A.binBase / 8;
  const int bin0 = blk * 8;
  // occupancy of the block's 8 bins: wave w <-> bin w
  const unsigned mask = A.cellMask[(size_t)(bin0 + w) * 64 + lane];
  s_masks[w][lane] = mask;
  s_arrLocal[w][lane] = 0u;
  {
    int n = __popc(mask);
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) n += __shfl_xor(n, sft, 64);
    if (lane == 0) s_total[w] = n;
  }
  if (tid < 128) s_clr[tid >> 6][tid & 63] = 0u;
  if (tid < 192) s_arrCnt[tid >> 6][tid & 63] = 0u;
  if (tid < 3) {
    s_xCnt[tid] = 0u;
    s_sums[tid] = 0;
  }
  if (tid < 8) (&s_cnt[0][0])[tid] = 0;
  if (tid == 0) {
    s_done = 0u;
    s_listDone = 0u;
    s_clear = A.gridClear ? A.gridClear + (size_t)blk * 7 * NC : nullptr;
  }
  if (tid >= 64 && tid < 64 + 27) s_nbrBlk[tid - 64] = A.nbr27[(size_t)blk * 27 + (tid - 64)];
  if (tid >= 96 && tid < 104) s_nbr8[tid - 96] = A.nbr[(size_t)blk * 8 + (tid - 96)];
  int borg[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) borg[d] = t.activeKeys[3 * (size_t)blk + d] * (8 / mp.kscale);
  __syncthreads();
  if ((s_total[0] | s_total[1] | s_total[2] | s_total[3] | s_total[4] | s_total[5] | s_total[6] | s_total[7]) == 0) {
    // an empty block (the partition's apron: a quarter to a half of all blocks) leaves before it gathers a velocity arena; it has no grid
    // sums, so it reports to the one-launch schedule's counter at once
    if (tid < 8) A.moverCount[bin0 + tid] = 0;
    if (A.signal && blk < A.signalBlocks && tid == 0) atomicAdd(A.signal, 1ull);
    blk_clear_block(s_clear, tid);
    return;
  }
  if (tid == 0) {  // the block's chunk sequence
    int G = 0, q = 0;
    for (int b = 0; b < 8; ++b) {
      const int nch = (s_total[b] + 255) >> 8;
      s_gbase[b] = G;
      s_binQ[b] = q;
      s_oc[b] = 0;
      if (nch) ++q;
      for (int c = 0; c < nch; ++c) {
        s_chBin[G] = (unsigned char)b;
        s_chIdx[G] = (unsigned char)c;
        s_desc[G + 1] = ChunkDesc::pack(b, c, s_binQ[b], c == nch - 1, s_total[b], s_gbase[b]);
        ++G;
      }
    }
    s_desc[0] = 0u;
    for (int k = G + 1; k < G + 5; ++k) s_desc[k] = 0u;
    s_G = G;
    // early warning of the closed-loop re-partition: the block holds particles and a block within {-1..2}^3 of it is missing
    if (G && A.blockEdge && A.blockEdge[blk]) A.status[3] = 1;
  }
  // the block's velocity arena: 10^3 nodes of grid A (this block and the 7 blocks at offsets {0,1}^3)
  for (int n = tid; n < 1000; n += 512) {
    const int x = n / 100, y = (n / 10) % 10, z = n % 10;
    const int slot = ((x >= 8) << 2) | ((y >= 8) << 1) | (z >= 8);
    const int cell = ((x & 7) * 8 + (y & 7)) * 8 + (z & 7);
    const int bn = s_nbr8[slot];
    float *a = s_varena + ArenaBlk::at(x, y, z);
    const float *g = A.gridA + ((size_t)(bn < 0 ? 0 : bn) * 7 + 1) * NC + cell;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) a[ch * ArenaBlk::CH] = bn >= 0 ? g[ch * NC] : 0.f;
  }
  __syncthreads();
  const int G = s_G;
  if (tid < 8 && s_total[tid] == 0) A.moverCount[bin0 + tid] = 0;
  {  // entry tables and neighbour bins of the bins of chunks 0 and 1 (all eight waves; later ones: the producers, two chunks ahead)
    const int b0 = s_chBin[0];
    blk_build_tab(s_masks[b0][lane], lane, w, 8, s_tab[s_binQ[b0] & 1]);
    if (tid < 27) s_nbrBin[s_binQ[b0] & 1][tid] = neighbour_bin8(s_nbrBlk, blk, b0, tid);
    if (G > 1 && s_chIdx[1] == 0) {
      const int b1 = s_chBin[1];
      blk_build_tab(s_masks[b1][lane], lane, w, 8, s_tab[s_binQ[b1] & 1]);
      if (tid >= 64 && tid < 64 + 27) s_nbrBin[s_binQ[b1] & 1][tid - 64] = neighbour_bin8(s_nbrBlk, blk, b1, tid - 64);
    }
  }
  __syncthreads();
  if (w < 4) blk_producer<SMODEL, WRITE_ALL>(mp, ps, borg, blk, lane, G, sh, A, __builtin_amdgcn_readfirstlane(w));
  else {
    if (w == 4) blk_consumer<0>(mp, borg, blk, lane, G, sh, A);
    else if (w == 5) blk_consumer<1>(mp, borg, blk, lane, G, sh, A);
    else if (w == 6) blk_consumer<2>(mp, borg, blk, lane, G, sh, A);
    else blk_consumer<3>(mp, borg, blk, lane, G, sh, A);
  }
  __syncthreads();  // the last bin is finished (blk_finish_bin by the consumer wave of set 3)
  {  // this step's arrivals from inside the block per cell (in-bin and in-block movers, lowered stayers: all tickets drawn), thread = (bin, cell).
     // High half of the claim word: slot_rehome_kernel puts the arrivals from other blocks above them (low half)
    const unsigned nl = s_arrLocal[w][lane];
    if (nl) A.claim[(size_t)(bin0 + w) * 64 + lane] = nl << 16;
  }
  if (tid == 0) {
    // movers sent / re-homed: running sums spread over SL_NCTR words (one device-wide word serves ~90 atomics per microsecond)
    if (s_sums[0]) atomicAdd(&A.status[SL_SENT + (blk & (SL_NCTR - 1))], s_sums[0]);
    if (s_sums[1]) atomicAdd(&A.status[SL_DELIVERED + (blk & (SL_NCTR - 1))], s_sums[1]);
  }
  if (s_sums[2]) {  // (rare) a chunk had more than SL_XQ movers for the consumers' list: the flagged records of those bins -> grid, all eight waves
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's record stores have reached L2 ...
    __syncthreads();                                    // ... and so have everybody else's
    constexpr int RB = SB_NG * G2P2G_QF * 64 / SL_REC;  // records per batch: the staging ring is free now
    for (int b = 0; b < 8; ++b) {
      if (!((s_sums[2] >> b) & 1)) continue;
      const SubGeom sg = sub_geom(borg, b);
      const int oc = s_oc[b];
      for (int j0 = 0; j0 < oc; j0 += RB) {
        const int nb = oc - j0 < RB ? oc - j0 : RB;
        const float *src = A.moverRec + ((size_t)(bin0 + b) * A.cap + (size_t)j0) * SL_REC;
        // agent-scope loads: served by L2, where the stores are (never by an L1 line of this CU)
        for (int k = tid; k < nb * SL_REC; k += 512) s_stage[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        outbox_scatter_global<8>(mp, sg, s_stage, nb, w, lane, s_nbrBlk, A.gridB, A.status);
        __syncthreads();
      }
    }
  }
  if (A.signal && blk < A.signalBlocks) {  // (workgroup-uniform) one of the blocks whose grid sums somebody is waiting for
    // this wave's atomic adds to grid B have been performed (they are device-wide operations: nothing of them sits in this XCD's L2, so
    // no release fence -- an agent-scope fence writes the whole L2 back, and a thousand workgroups doing that cost a third of the step) ...
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // ... and every wave's
    if (tid == 0) atomicAdd(A.signal, 1ull);
  }
  // last of all (behind the role functions' last barrier, nothing of the chunk loop alive, and behind the signal, whose vmcnt(0) must not
  // wait for these stores).  The address comes back from LDS, on this path and at the early exit: with A.gridClear read at the early exit
  // every instantiation spilled two more SGPRs across the chunk loop and NACC's a VGPR as well (8 B of private segment).
  blk_clear_block(s_clear, tid);
}

template <int M, bool WA> static void launch_blk(hipStream_t stream, unsigned nblk, const MpmDev &mp, const ParticlesDev &pd, const BhtDev &t, const SlotArgs &A) {
  hipLaunchKernelGGL((g2p2g_slotblk_kernel<M, WA>), dim3(nblk), dim3(512), 0, stream, mp, pd, t, A);
}

// launched by zs_rocm_mpm_g2p2g_slots (mpm_slotted.hip) for 8^3 blocks: blocks [A.binBase / 8, + A.nbins / 8)
void launch_g2p2g_slotblk(hipStream_t stream, int model, bool writeAll, const MpmDev &mp, const ParticlesDev &pd, const BhtDev &t, const SlotArgs &A) {
  const unsigned nblk = (unsigned)(A.nbins / 8);
  if (!nblk) return;
#define CALL_BLK(SS, M)                                            \
  do {                                                             \
    if (writeAll) launch_blk<M, true>(stream, nblk, mp, pd, t, A); \
    else launch_blk<M, false>(stream, nblk, mp, pd, t, A);         \
  } while (0)
  ZSR_DISPATCH_PURE_(8, model, CALL_BLK)  // (the caller has rejected anything that is not one of the five models)
#undef CALL_BLK
}

}  // namespace zsr
