// levelset_transition.hip -- keyframed level-set colliders for gfx950: the blend of two sparse level sets (TransitionLevelSetView,
// include/zensim_rocm/levelset_device.hpp) as the boundary of ApplyBoundaryConditionOnGridBlocks and of ImplicitMPMSystem::project, the
// bulk point entries, and the reduction behind get_level_set_max_speed (geometry/LevelSetUtils.tpp).
//
// The block kernels follow levelset.hip's plan, ONE WORKGROUP PER MPM GRID BLOCK, over two level sets:
//   footprint   per level set, the bounding box of the block's 8 corner nodes in that level set's index space, padded like the single
//               level set's (floor(min) - 1 .. floor(max) + 2) and widened on every side by
//                   widen = ceil(stepDt * max(alpha, 1 - alpha) * maxSpeed / h) + 1   cells:
//               a sample point moves by alpha stepDt v or (1 - alpha) stepDt v, and every component of v is a mean of two trilinear
//               samples, i.e. a convex combination of "v" cell values and backgrounds, so |v_d| <= maxSpeed; the + 1 takes the roundings
//   blocks      the level-set blocks under each footprint, one 16-lane tile query per block
//   staging     both footprints' sdf cells go to LDS
//   cull        no staged sdf value of either level set negative => no node is inside (the blend weights 1 - alpha and alpha are >= 0
//               and so are the trilinear weights): done before any read of the MPM grid
//   evaluation  otherwise the "v" boxes are staged next to their sdf boxes and every node with mass evaluates from LDS
//   budget      TR_STAGE_FLOATS floats of LDS per workgroup, shared by the two level sets ("keyframed level sets") and handed
//               out in the order sdf of src, sdf of dst, "v" of src, "v" of dst.  A "v" box that no longer fits is read directly
//               (its level set keeps the sdf box: the cull and the 14 sdf samples per node stay in LDS); a level set whose sdf box
//               does not fit (or that spans more than TR_STAGE_BLOCKS level-set blocks) is read through direct hash queries, and the
//               block is not culled
// Staged and direct cells go through the same fetch interface into the same sums, and a cell outside a staged box is read directly:
// every evaluated node gets the bits of zs_rocm_levelset_transition_collider_resolve whatever maxSpeed says.  (The cull trusts the
// footprint: it is right for any maxSpeed that is a bound, and for a smaller one as long as the real displacement stays within the
// widening assumed plus the 1.75 cells of pad.)  Built with -ffp-contract=off.
#include <cmath>

#include "common.hpp"
#include "bht.hpp"
#include "../../include/zensim_rocm/levelset_device.hpp"

namespace zsr {

// 76 KB per workgroup: two workgroups stay resident in a CU's 160 KB.  19456 floats hold all four channels of both level sets over the
// 13^3 cells an 8^3-node block covers at h = dx with widen = 1 (17 576), and at widen = 2 (15^3) both sdf boxes and one "v" box (16 875).
constexpr int TR_STAGE_FLOATS = 19456, TR_STAGE_BLOCKS = 64;
constexpr int TR_MAX_EXTENT = 4096;  // cells per axis (and of widening) beyond which a footprint is not even measured: it cannot fit
enum { TR_CULLED = 0, TR_STAGED = 1, TR_DIRECT = 2, TR_V_DIRECT = 3 };

// cell values of one level set: sdf and / or [v0 | v1 | v2] from its staged boxes in LDS (z fastest; a null pointer: not staged), all
// else directly
struct TransitionStagedFetch {
  LevelSetDirectFetch direct;
  const float *sdfCells, *velCells;
  int lo[3], n[3], stride, sdfChannel, velChannel;
  __device__ __forceinline__ explicit TransitionStagedFetch(const LevelSetView &l)
      : direct(l), sdfCells(nullptr), velCells(nullptr), lo{0, 0, 0}, n{0, 0, 0}, stride(0), sdfChannel(l.sdfChannel), velChannel(l.velChannel) {}
  __device__ __forceinline__ float operator()(int chn, int ix, int iy, int iz) const {
    const unsigned a = (unsigned)(ix - lo[0]), b = (unsigned)(iy - lo[1]), c = (unsigned)(iz - lo[2]);
    const float *box = chn == sdfChannel ? sdfCells : (velCells ? velCells + (chn - velChannel) * stride : nullptr);
    if (box && a < (unsigned)n[0] && b < (unsigned)n[1] && c < (unsigned)n[2]) return box[((int)a * n[1] + (int)b) * n[2] + (int)c];
    return direct(chn, ix, iy, iz);
  }
};

// one level set's footprint under a grid block
struct TransitionFootprint {
  int lo[3], n[3], blo[3], bn[3], ncell, nblk;
  bool fits;  // the sdf box fits `cap` floats and the blocks fit s_bno
};

template <int SIDE>
__device__ __forceinline__ TransitionFootprint transition_footprint(const ColliderDev &motion, const LevelSetView &ls, const int *key, int kscale,
                                                                    float dx, int widen, int cap) {
  TransitionFootprint fp;
  fp.fits = false;
  fp.ncell = fp.nblk = 0;
  float mn[3], mx[3];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float pos[3], xmb[3], X[3], I[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) pos[d] = (float)(key[d] / kscale * SIDE + (((c >> (2 - d)) & 1) ? SIDE - 1 : 0)) * dx;
    motion.to_material(pos, xmb, X);
    ls.worldToIndex(X, I);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      mn[d] = c == 0 ? I[d] : fminf(mn[d], I[d]);
      mx[d] = c == 0 ? I[d] : fmaxf(mx[d], I[d]);
    }
  }
  bool sane = widen < TR_MAX_EXTENT;
#pragma unroll
  for (int d = 0; d < 3; ++d) sane = sane && mn[d] > -1e9f && mx[d] < 1e9f && mx[d] - mn[d] < (float)TR_MAX_EXTENT;  // (false for NaN)
  if (!sane) return fp;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    fp.lo[d] = (int)floorf(mn[d]) - 1 - widen;
    fp.n[d] = (int)floorf(mx[d]) + 2 + widen - fp.lo[d] + 1;
    fp.blo[d] = fp.lo[d] >> 3;
    fp.bn[d] = ((fp.lo[d] + fp.n[d] - 1) >> 3) - fp.blo[d] + 1;
  }
  // (each n[d] < 3 * TR_MAX_EXTENT + 8, each bn[d] below an eighth of that + 2: the partial products are tested before the full ones)
  if (fp.n[0] * fp.n[1] > cap || fp.bn[0] * fp.bn[1] > TR_STAGE_BLOCKS) return fp;
  fp.ncell = fp.n[0] * fp.n[1] * fp.n[2];
  fp.nblk = fp.bn[0] * fp.bn[1] * fp.bn[2];
  fp.fits = fp.ncell <= cap && fp.nblk <= TR_STAGE_BLOCKS;
  return fp;
}

// block numbers of the footprint's level-set blocks into bno[]; returns (on this thread) whether one it looked at is stored
__device__ __forceinline__ int transition_resolve_blocks(const LevelSetView &ls, const BhtDev &t, const TransitionFootprint &fp, int *bno) {
  int present = 0;
  BhtWaveTile tile(BHT_BUCKET);
  const int tileId = (int)threadIdx.x / BHT_BUCKET, ntiles = (int)blockDim.x / BHT_BUCKET;
  for (int k = tileId; k < fp.nblk; k += ntiles) {
    const int org[3] = {(fp.blo[0] + k / (fp.bn[1] * fp.bn[2])) * LS_SIDE, (fp.blo[1] + k / fp.bn[2] % fp.bn[1]) * LS_SIDE,
                        (fp.blo[2] + k % fp.bn[2]) * LS_SIDE};
    int b = bht_tile_query<3>(t, org, tile);
    if (!(b >= 0 && (size_t)b < ls.numBlocks)) b = -1;  // as LevelSetView::block_of
    if (tile.thread_rank() == 0) bno[k] = b;
    present |= b >= 0;
  }
  return present;
}

// one channel of the footprint into dst[ncell]; returns (on this thread) whether a value it wrote is negative
__device__ __forceinline__ int transition_stage(const LevelSetView &ls, const TransitionFootprint &fp, const int *bno, int chn, float *dst) {
  int neg = 0;
  for (int c = (int)threadIdx.x; c < fp.ncell; c += (int)blockDim.x) {
    const int iz = fp.lo[2] + c % fp.n[2], iy = fp.lo[1] + c / fp.n[2] % fp.n[1], ix = fp.lo[0] + c / (fp.n[2] * fp.n[1]);
    const int b = bno[(((ix >> 3) - fp.blo[0]) * fp.bn[1] + ((iy >> 3) - fp.blo[1])) * fp.bn[2] + ((iz >> 3) - fp.blo[2])];
    const float v = ls.cell_value(chn, b, ix, iy, iz);
    dst[c] = v;
    neg |= v < 0.f;
  }
  return neg;
}

// What every thread of the workgroup runs before the evaluation; `lds` = cap floats.  Returns TR_CULLED / TR_STAGED / TR_DIRECT (the
// same on every thread), sets up the two fetches and *vDirect (a "v" box that did not fit).
template <int SIDE>
__device__ __forceinline__ int transition_block_prepare(const TransitionColliderDev &col, const int *key, int kscale, float dx, int widenS,
                                                        int widenD, int cap, float *lds, TransitionStagedFetch &fS,
                                                        TransitionStagedFetch &fD, bool *vDirect) {
  __shared__ int s_bno[2][TR_STAGE_BLOCKS];
  const LevelSetView &S = col.tr.src, &D = col.tr.dst;
  const TransitionFootprint fpS = transition_footprint<SIDE>(col.motion, S, key, kscale, dx, widenS, cap);
  int used = fpS.fits ? fpS.ncell : 0;  // floats of `lds` handed out
  const TransitionFootprint fpD = transition_footprint<SIDE>(col.motion, D, key, kscale, dx, widenD, cap - used);
  *vDirect = false;
  int present = 0;
  if (fpS.fits) present |= transition_resolve_blocks(S, fS.direct.t, fpS, s_bno[0]);
  if (fpD.fits) present |= transition_resolve_blocks(D, fD.direct.t, fpD, s_bno[1]);
  present = __syncthreads_or(present);
  const bool both = fpS.fits && fpD.fits;
  if (both && !present && !(S.background < 0.f) && !(D.background < 0.f)) return TR_CULLED;  // nothing but backgrounds under the block
  float *ldsD = lds + used;
  if (fpD.fits) used += fpD.ncell;
  int neg = 0;
  if (fpS.fits) neg |= transition_stage(S, fpS, s_bno[0], S.sdfChannel, lds);
  if (fpD.fits) neg |= transition_stage(D, fpD, s_bno[1], D.sdfChannel, ldsD);
  neg = __syncthreads_or(neg);
  if (both && !neg) return TR_CULLED;
  auto finish = [&](const LevelSetView &ls, const TransitionFootprint &fp, const int *bno, float *cells, TransitionStagedFetch &f) {
    if (!fp.fits) return;
    if (ls.velChannel >= 0) {
      if (3 * fp.ncell <= cap - used) {
        float *vel = lds + used;
        used += 3 * fp.ncell;
#pragma unroll 1
        for (int k = 0; k < 3; ++k) transition_stage(ls, fp, bno, ls.velChannel + k, vel + k * fp.ncell);
        f.velCells = vel;
      } else {
        *vDirect = true;
      }
    }
    f.sdfCells = cells;
    f.stride = fp.ncell;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      f.lo[d] = fp.lo[d];
      f.n[d] = fp.n[d];
    }
  };
  finish(S, fpS, s_bno[0], lds, fS);
  finish(D, fpD, s_bno[1], ldsD, fD);
  __syncthreads();
  return both ? TR_STAGED : TR_DIRECT;
}

// PROJECT as in levelset_block_kernel
template <int SIDE, bool PROJECT>
__global__ __launch_bounds__(SIDE == 8 ? 256 : 64) void transition_block_kernel(TransitionColliderDev col, const int *activeKeys, float *grid,
                                                                                float *dof, float dx, int kscale, int widenS, int widenD,
                                                                                int cap) {
  constexpr int NC = SIDE * SIDE * SIDE;
  extern __shared__ float lds[];
  const size_t blk = blockIdx.x;
  const int key[3] = {activeKeys[3 * blk], activeKeys[3 * blk + 1], activeKeys[3 * blk + 2]};
  TransitionStagedFetch fS(col.tr.src), fD(col.tr.dst);
  bool vDirect;
  const int path = transition_block_prepare<SIDE>(col, key, kscale, dx, widenS, widenD, cap, lds, fS, fD, &vDirect);
  unsigned *stats = col.tr.src.stats;
  if (stats && threadIdx.x == 0) {
    atomicAdd(stats + path, 1u);
    if (path == TR_STAGED && vDirect) atomicAdd(stats + TR_V_DIRECT, 1u);
  }
  if (!PROJECT && path == TR_CULLED) return;
  const float *mass = grid + blk * 7 * NC;
  for (int cell = (int)threadIdx.x; cell < NC; cell += (int)blockDim.x) {
    float *v = PROJECT ? dof + 3 * (blk * NC + cell) : grid + blk * 7 * NC + NC + cell;
    constexpr int VS = PROJECT ? 1 : NC;
    if (!(mass[cell] > 0.f)) {
      if (PROJECT) v[0] = v[1] = v[2] = 0.f;
      continue;
    }
    if (path == TR_CULLED) continue;
    const int cc[3] = {cell / (SIDE * SIDE), (cell / SIDE) % SIDE, cell % SIDE};
    float pos[3], vel[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      pos[d] = (float)(key[d] / kscale * SIDE + cc[d]) * dx;
      vel[d] = v[d * VS];
    }
    if (col.resolveCollision(fS, fD, pos, vel)) {
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d * VS] = vel[d];
    }
  }
}

__global__ __launch_bounds__(256) void transition_resolve_kernel(TransitionColliderDev col, const float *x, float *v, size_t n, int *inside) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  float u[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
  const bool in = col.resolveCollision(p, u);
  if (in) { v[3 * i] = u[0]; v[3 * i + 1] = u[1]; v[3 * i + 2] = u[2]; }
  if (inside) inside[i] = in ? 1 : 0;
}

__global__ __launch_bounds__(256) void transition_sample_kernel(TransitionLevelSetView tr, const float *x, size_t n, float *sdf, float *normal,
                                                                float *vel) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  const LevelSetDirectFetch fs(tr.src), fd(tr.dst);
  float x0[3], x1[3], r[3];
  tr.displaced(fs, fd, p, x0, x1);
  if (sdf) sdf[i] = tr.sdf_at(fs, fd, x0, x1);
  if (normal) {
    tr.normal_at(fs, fd, x0, x1, r);
    normal[3 * i] = r[0]; normal[3 * i + 1] = r[1]; normal[3 * i + 2] = r[2];
  }
  if (vel) {
    tr.velocity_at(fs, fd, x0, x1, r);
    vel[3 * i] = r[0]; vel[3 * i + 1] = r[1]; vel[3 * i + 2] = r[2];
  }
}

// max |v_d| over the 3 * 512 "v" values of every stored block (contiguous in a tile): the bit patterns of non-negative floats order
// like the values, so the maximum is an integer atomicMax on the zeroed word.  NaN cells are passed over (fmaxf).
__global__ __launch_bounds__(256) void levelset_max_speed_kernel(LevelSetView ls, size_t nvalues, unsigned *out) {
  float m = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvalues; i += (size_t)gridDim.x * blockDim.x) {
    const size_t bno = i / (3 * LS_BLOCK), r = i % (3 * LS_BLOCK);
    m = fmaxf(m, fabsf(ls.tiles[(bno * ls.numChannels + ls.velChannel) * LS_BLOCK + r]));
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, shfl_down(m, d));
  if (lane_id() == 0 && m > 0.f) atomicMax(out, __float_as_uint(m));
}

static bool finite_nonneg(float v) { return v >= 0.f && v <= 3.4028234e38f; }  // (false for NaN)
bool transition_ok(const zs_rocm_levelset_transition *t) {
  return t && levelset_ok(&t->src) && levelset_ok(&t->dst) && t->alpha >= 0.f && t->alpha <= 1.f && finite_nonneg(t->stepDt) &&
         finite_nonneg(t->maxSpeed);
}
bool transition_collider_ok(const zs_rocm_collider *c, const zs_rocm_levelset_transition *t) {
  return c && c->type >= ZS_ROCM_COLLIDER_STICKY && c->type <= ZS_ROCM_COLLIDER_SEPARATE && c->s != 0.f && transition_ok(t);
}

// cells a footprint is widened by on every side (header comment); beyond the staging budget it is all the same: direct
static int transition_widen(const zs_rocm_levelset_transition *t, float h) {
  const float cells = std::ceil(t->stepDt * std::fmax(t->alpha, 1.f - t->alpha) * t->maxSpeed / h);
  return cells < (float)TR_MAX_EXTENT ? (int)cells + 1 : TR_MAX_EXTENT;  // (NaN, inf: too wide to stage)
}
// LDS floats a level set can use: an upper bound of its footprint's cells (the block's edges through R^T / s / h, bounded per axis by
// the 1-norm of the row) times its channels, at most the budget.  Only sizes the allocation: the kernel tests the real footprint
// against it.
static int transition_cap(const zs_rocm_mpm_params *p, const zs_rocm_collider *c, const zs_rocm_levelset *l, int widen) {
  double cells = 1.0;
  for (int d = 0; d < 3; ++d) {
    const double row = std::fabs((double)c->R[d]) + std::fabs((double)c->R[3 + d]) + std::fabs((double)c->R[6 + d]);
    const double ext = row * (p->side - 1) * (double)p->dx / std::fabs((double)c->s) / (double)l->h;
    cells *= std::floor(ext) + 6.0 + 2.0 * widen;  // floor(max) - floor(min) <= floor(ext) + 1, the pad of 4, one for the float map
  }
  const double want = cells * (l->velChannel >= 0 ? 4 : 1);
  return want < (double)TR_STAGE_FLOATS ? (int)want : TR_STAGE_FLOATS;  // (NaN: the budget)
}

bool transition_blocks_enqueue(hipStream_t stream, const zs_rocm_mpm_params *p, const int *activeKeys, float *grid, size_t nblocks,
                               const zs_rocm_collider *collider, const zs_rocm_levelset_transition *tr, float *dof) {
  if (!nblocks) return true;
  TransitionColliderDev col;
  col.motion = ColliderDev(*collider);
  col.tr = TransitionLevelSetView(*tr);
  const int kscale = p->keyIsOrigin ? p->side : 1;
  const int widenS = transition_widen(tr, tr->src.h), widenD = transition_widen(tr, tr->dst.h);
  int cap = transition_cap(p, collider, &tr->src, widenS) + transition_cap(p, collider, &tr->dst, widenD);
  if (cap > TR_STAGE_FLOATS) cap = TR_STAGE_FLOATS;
  const size_t shm = sizeof(float) * (size_t)cap;
  float dx = p->dx;
  int ks = kscale, wS = widenS, wD = widenD;
  void *args[] = {&col, &activeKeys, &grid, &dof, &dx, &ks, &wS, &wD, &cap};
  hipError_t err = hipSuccess;
#define CALL_TR_BLOCKS(S, PRJ)                                                                                                   \
  do {                                                                                                                           \
    const void *kernel = (const void *)transition_block_kernel<S, PRJ>;                                                          \
    if (shm > 64 * 1024) err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);                \
    if (err == hipSuccess) err = hipLaunchKernel(kernel, dim3((unsigned)nblocks), dim3(S == 8 ? 256 : 64), args, shm, stream);   \
  } while (0)
  if (p->side == 4) {
    if (dof) CALL_TR_BLOCKS(4, true);
    else CALL_TR_BLOCKS(4, false);
  } else {
    if (dof) CALL_TR_BLOCKS(8, true);
    else CALL_TR_BLOCKS(8, false);
  }
#undef CALL_TR_BLOCKS
  return err == hipSuccess;
}

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_levelset_max_speed(zs_rocm_policy *pol, const zs_rocm_levelset *levelset, float *out) {
  if (!pol || !levelset_ok(levelset) || !out) return -1;
  Launch L(pol, "get_level_set_max_speed");
  (void)hipMemsetAsync(out, 0, sizeof(float), L.stream);
  const size_t nvalues = levelset->velChannel >= 0 ? levelset->numBlocks * 3 * LS_BLOCK : 0;
  if (!nvalues) return 0;
  const unsigned blocks = ceil_div(nvalues, 256 * 8) < 4096u ? ceil_div(nvalues, 256 * 8) : 4096u;
  hipLaunchKernelGGL(levelset_max_speed_kernel, dim3(blocks), dim3(256), 0, L.stream, LevelSetView(*levelset), nvalues, (unsigned *)out);
  return 0;
}

int zs_rocm_levelset_transition_sample(zs_rocm_policy *pol, const zs_rocm_levelset_transition *tr, const float *x, size_t n, float *sdf,
                                       float *normal, float *vel) {
  if (!pol || !transition_ok(tr) || (n && !x)) return -1;
  Launch L(pol, "TransitionLevelSetView sample");
  if (!n) return 0;
  hipLaunchKernelGGL(transition_sample_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, TransitionLevelSetView(*tr), x, n, sdf, normal,
                     vel);
  return 0;
}

int zs_rocm_levelset_transition_collider_resolve(zs_rocm_policy *pol, const zs_rocm_collider *collider, const zs_rocm_levelset_transition *tr,
                                                 const float *x, float *v, size_t n, int *inside) {
  if (!pol || !transition_collider_ok(collider, tr) || (n && (!x || !v))) return -1;
  Launch L(pol, "Collider<TransitionLevelSet>::resolveCollision");
  if (!n) return 0;
  TransitionColliderDev col;
  col.motion = ColliderDev(*collider);
  col.tr = TransitionLevelSetView(*tr);
  hipLaunchKernelGGL(transition_resolve_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, col, x, v, n, inside);
  return 0;
}

int zs_rocm_mpm_apply_boundary_transition(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, const zs_rocm_bht_3 *tab, float *grid, size_t nblocks,
                                          const zs_rocm_collider *collider, const zs_rocm_levelset_transition *tr) {
  if (!pol || !p || !tab || !grid || (p->side != 4 && p->side != 8) || !(p->dx > 0.f) || !transition_collider_ok(collider, tr)) return -1;
  if (nblocks > (size_t)0x7fffffff) return -1;
  Launch L(pol, "ApplyBoundaryConditionOnGridBlocks (level-set transition)");
  return transition_blocks_enqueue(L.stream, p, (const int *)tab->t.dev().activeKeys, grid, nblocks, collider, tr, nullptr) ? 0 : -1;
}

}  // extern "C"
