// levelset.hip -- sparse level-set colliders for gfx950: LevelSetBoundary<SparseGrid<3, f32, 8>> as the boundary of
// ApplyBoundaryConditionOnGridBlocks (simulation/grid/GridOp.hpp:128-134) and of ImplicitMPMSystem::project
// (simulation/mpm/ImplicitMPM.hpp:110-114), plus the bulk point entries.  The arithmetic is include/zensim_rocm/levelset_device.hpp.
//
// A node inside the collider needs 7 trilinear samples of "sdf" (value + 6 for the normal) and one of the 3 "v" channels: ~80 cell
// reads, each behind a hash query when sampled point by point.  The block kernels run ONE WORKGROUP PER MPM GRID BLOCK instead:
//   footprint   the 8 corners of the block's node box go through the collider transform and worldToIndex; their bounding box in
//               level-set index space, floor(min) - 1 .. floor(max) + 2 per axis, holds every cell any sample of any node reads (the
//               stencil's upper corner is +1, the +- h / 4 shifts of the normal stay inside the one-cell pad)
//   blocks      the level-set blocks the footprint touches (2^3 for an 8^3-node block at h = dx) are resolved by one 16-lane tile
//               each, one cooperative hash query per block
//   staging     the footprint's sdf cells go to LDS, z fastest (runs of up to 8 consecutive floats of a tile); cells of absent blocks
//               get the background
//   cull        no staged sdf value negative => no node of the block is inside (the weights are >= 0): the block is done, before any
//               read of the MPM grid.  The common case of a large scene.
//   evaluation  otherwise the "v" cells are staged too and every node with mass evaluates all its samples from LDS
//   fallback    a footprint of more than LS_STAGE_CELLS = 2048 cells (8 KB of LDS for sdf, 32 KB with "v"; five workgroups still fit
//               a CU's 160 KB) or more than LS_STAGE_BLOCKS = 64 level-set blocks -- strong rotation, h << dx -- is evaluated
//               through direct hash queries per cell.  No cull there.
// Staged and direct cells go through the same fetch functor interface into the same sums: a node gets the same bits on either path and
// from zs_rocm_levelset_collider_resolve.  A cell outside the staged box (never expected; the box is padded) is read directly.
// Built with -ffp-contract=off (zpc_amd/build.py).
#include "common.hpp"
#include "bht.hpp"
#include "../../include/zensim_rocm/levelset_device.hpp"

namespace zsr {

constexpr int LS_STAGE_CELLS = 2048, LS_STAGE_BLOCKS = 64;
enum { LS_CULLED = 0, LS_STAGED = 1, LS_DIRECT = 2 };

// cell values from the staged box in LDS ([sdf | v0 | v1 | v2] x cells, z fastest); an empty box makes it the direct fetch
struct LevelSetStagedFetch {
  LevelSetDirectFetch direct;
  const float *cells;
  int lo[3], n[3], stride, sdfChannel, velChannel;
  __device__ __forceinline__ explicit LevelSetStagedFetch(const LevelSetView &l) : direct(l), cells(nullptr), lo{0, 0, 0}, n{0, 0, 0}, stride(0),
                                                                                 sdfChannel(l.sdfChannel), velChannel(l.velChannel) {}
  __device__ __forceinline__ float operator()(int chn, int ix, int iy, int iz) const {
    const unsigned a = (unsigned)(ix - lo[0]), b = (unsigned)(iy - lo[1]), c = (unsigned)(iz - lo[2]);
    if (a < (unsigned)n[0] && b < (unsigned)n[1] && c < (unsigned)n[2]) {
      const int slot = chn == sdfChannel ? 0 : 1 + (chn - velChannel);
      return cells[slot * stride + ((int)a * n[1] + (int)b) * n[2] + (int)c];
    }
    return direct(chn, ix, iy, iz);
  }
};

// The per-block body both kernels share.  Every thread of the workgroup calls it; `lds` = LS_STAGE_CELLS floats (x 4 with "v").
// Returns LS_CULLED / LS_STAGED / LS_DIRECT (the same on every thread) and sets up `f` for the evaluation.
template <int SIDE>
__device__ __forceinline__ int levelset_block_prepare(const LevelSetColliderDev &col, const int *key, int kscale, float dx, float *lds,
                                                      LevelSetStagedFetch &f) {
  __shared__ int s_bno[LS_STAGE_BLOCKS];
  const LevelSetView &ls = col.ls;
  // footprint: bounding box of the 8 corner nodes in level-set index space (the map is affine)
  float mn[3], mx[3];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float pos[3], xmb[3], X[3], I[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) pos[d] = (float)(key[d] / kscale * SIDE + (((c >> (2 - d)) & 1) ? SIDE - 1 : 0)) * dx;
    col.motion.to_material(pos, xmb, X);
    ls.worldToIndex(X, I);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      mn[d] = c == 0 ? I[d] : fminf(mn[d], I[d]);
      mx[d] = c == 0 ? I[d] : fmaxf(mx[d], I[d]);
    }
  }
  bool fits = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) fits = fits && mn[d] > -1e9f && mx[d] < 1e9f && mx[d] - mn[d] < (float)LS_STAGE_CELLS;  // (false for NaN)
  if (!fits) return LS_DIRECT;
  int lo[3], n[3], blo[3], bn[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = (int)floorf(mn[d]) - 1;
    n[d] = (int)floorf(mx[d]) + 2 - lo[d] + 1;
    blo[d] = lo[d] >> 3;
    bn[d] = ((lo[d] + n[d] - 1) >> 3) - blo[d] + 1;
  }
  // (each n[d] < 2052, each bn[d] < 259: the partial products are tested before the full ones are formed)
  if (n[0] * n[1] > LS_STAGE_CELLS || bn[0] * bn[1] > LS_STAGE_BLOCKS) return LS_DIRECT;
  const int ncell = n[0] * n[1] * n[2], nblk = bn[0] * bn[1] * bn[2];
  if (ncell > LS_STAGE_CELLS || nblk > LS_STAGE_BLOCKS) return LS_DIRECT;
  // the level-set blocks under the footprint, one 16-lane tile each: the tile's lanes look at the 16 slots of a bucket together (one load
  // per lane and bucket; most blocks of a large scene are far from the collider, and an ABSENT key costs a lane of its own all 3 x 16
  // slots one after the other)
  int present = 0;
  {
    BhtWaveTile tile(BHT_BUCKET);
    const int tileId = (int)threadIdx.x / BHT_BUCKET, ntiles = (int)blockDim.x / BHT_BUCKET;
    for (int t = tileId; t < nblk; t += ntiles) {
      const int org[3] = {(blo[0] + t / (bn[1] * bn[2])) * LS_SIDE, (blo[1] + t / bn[2] % bn[1]) * LS_SIDE, (blo[2] + t % bn[2]) * LS_SIDE};
      int bno = bht_tile_query<3>(f.direct.t, org, tile);
      if (!(bno >= 0 && (size_t)bno < ls.numBlocks)) bno = -1;  // as LevelSetView::block_of
      if (tile.thread_rank() == 0) s_bno[t] = bno;
      present |= bno >= 0;
    }
  }
  present = __syncthreads_or(present);
  if (!present && !(ls.background < 0.f)) return LS_CULLED;  // nothing but background under the block
  auto stage = [&](int chn, float *dst) {
    int neg = 0;
    for (int c = (int)threadIdx.x; c < ncell; c += (int)blockDim.x) {
      const int iz = lo[2] + c % n[2], iy = lo[1] + c / n[2] % n[1], ix = lo[0] + c / (n[2] * n[1]);
      const int bno = s_bno[(((ix >> 3) - blo[0]) * bn[1] + ((iy >> 3) - blo[1])) * bn[2] + ((iz >> 3) - blo[2])];
      const float v = ls.cell_value(chn, bno, ix, iy, iz);
      dst[c] = v;
      neg |= v < 0.f;
    }
    return neg;
  };
  if (!__syncthreads_or(stage(ls.sdfChannel, lds))) return LS_CULLED;
  if (ls.velChannel >= 0) {
#pragma unroll 1
    for (int k = 0; k < 3; ++k) stage(ls.velChannel + k, lds + (1 + k) * ncell);
    __syncthreads();
  }
  f.cells = lds;
  f.stride = ncell;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    f.lo[d] = lo[d];
    f.n[d] = n[d];
  }
  return LS_STAGED;
}

// PROJECT = false: ApplyBoundaryConditionOnGridBlocks on the grid's velocity channels; true: Projector on a dof vector (nodes without
// mass zeroed, also in culled blocks).
template <int SIDE, bool PROJECT>
__global__ __launch_bounds__(SIDE == 8 ? 256 : 64) void levelset_block_kernel(LevelSetColliderDev col, const int *activeKeys, float *grid, float *dof,
                                                                              float dx, int kscale) {
  constexpr int NC = SIDE * SIDE * SIDE;
  extern __shared__ float lds[];
  const size_t blk = blockIdx.x;
  const int key[3] = {activeKeys[3 * blk], activeKeys[3 * blk + 1], activeKeys[3 * blk + 2]};
  LevelSetStagedFetch f(col.ls);
  const int path = levelset_block_prepare<SIDE>(col, key, kscale, dx, lds, f);
  if (col.ls.stats && threadIdx.x == 0) atomicAdd(col.ls.stats + path, 1u);
  if (!PROJECT && path == LS_CULLED) return;
  const float *mass = grid + blk * 7 * NC;
  for (int cell = (int)threadIdx.x; cell < NC; cell += (int)blockDim.x) {
    float *v = PROJECT ? dof + 3 * (blk * NC + cell) : grid + blk * 7 * NC + NC + cell;
    constexpr int VS = PROJECT ? 1 : NC;  // stride between the components of a node's velocity
    if (!(mass[cell] > 0.f)) {
      if (PROJECT) v[0] = v[1] = v[2] = 0.f;  // clear non-dof nodes as well (ImplicitMPM.hpp:85-88)
      continue;
    }
    if (path == LS_CULLED) continue;
    const int cc[3] = {cell / (SIDE * SIDE), (cell / SIDE) % SIDE, cell % SIDE};
    float pos[3], vel[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      pos[d] = (float)(key[d] / kscale * SIDE + cc[d]) * dx;  // as apply_boundary_kernel forms it
      vel[d] = v[d * VS];
    }
    if (col.resolveCollision(f, pos, vel)) {
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d * VS] = vel[d];
    }
  }
}

__global__ __launch_bounds__(256) void levelset_resolve_kernel(LevelSetColliderDev col, const float *x, float *v, size_t n, int *inside) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  float u[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
  const bool in = col.resolveCollision(p, u);
  if (in) { v[3 * i] = u[0]; v[3 * i + 1] = u[1]; v[3 * i + 2] = u[2]; }
  if (inside) inside[i] = in ? 1 : 0;
}

__global__ __launch_bounds__(256) void levelset_sample_kernel(LevelSetView ls, const float *x, size_t n, float *sdf, float *normal, float *vel) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  const LevelSetDirectFetch f(ls);
  if (sdf) sdf[i] = ls.getSignedDistance(f, p);
  float r[3];
  if (normal) {
    ls.getNormal(f, p, r);
    normal[3 * i] = r[0]; normal[3 * i + 1] = r[1]; normal[3 * i + 2] = r[2];
  }
  if (vel) {
    ls.getMaterialVelocity(f, p, r);
    vel[3 * i] = r[0]; vel[3 * i + 1] = r[1]; vel[3 * i + 2] = r[2];
  }
}

bool levelset_ok(const zs_rocm_levelset *l) {
  if (!l || !l->tiles || !l->table.keys || !l->table.indices) return false;
  if ((size_t)l->table.numBuckets * BHT_BUCKET > l->table.tableSize) return false;
  if (l->numChannels < 1 || l->sdfChannel < 0 || l->sdfChannel >= l->numChannels) return false;
  if (l->velChannel != -1 && (l->velChannel < 0 || l->velChannel + 3 > l->numChannels)) return false;
  if (l->velChannel != -1 && l->sdfChannel >= l->velChannel && l->sdfChannel < l->velChannel + 3) return false;
  return l->h > 0.f && l->h <= 3.0e38f;
}
bool levelset_collider_ok(const zs_rocm_collider *c, const zs_rocm_levelset *l) {
  return c && c->type >= ZS_ROCM_COLLIDER_STICKY && c->type <= ZS_ROCM_COLLIDER_SEPARATE && c->s != 0.f && levelset_ok(l);
}

// arguments checked by the caller.  dof == nullptr: the boundary pass on `grid`; else the projection of `dof` (grid is only read)
void levelset_blocks_enqueue(hipStream_t stream, const zs_rocm_mpm_params *p, const int *activeKeys, float *grid, size_t nblocks,
                             const zs_rocm_collider *collider, const zs_rocm_levelset *levelset, float *dof) {
  if (!nblocks) return;
  LevelSetColliderDev col;
  col.motion = ColliderDev(*collider);
  col.ls = LevelSetView(*levelset);
  const int kscale = p->keyIsOrigin ? p->side : 1;
  const size_t shm = sizeof(float) * LS_STAGE_CELLS * (levelset->velChannel >= 0 ? 4 : 1);
  const dim3 g((unsigned)nblocks);
#define CALL_LS_BLOCKS(S, PRJ) \
  hipLaunchKernelGGL((levelset_block_kernel<S, PRJ>), g, dim3(S == 8 ? 256 : 64), shm, stream, col, activeKeys, grid, dof, p->dx, kscale)
  if (p->side == 4) {
    if (dof) CALL_LS_BLOCKS(4, true);
    else CALL_LS_BLOCKS(4, false);
  } else {
    if (dof) CALL_LS_BLOCKS(8, true);
    else CALL_LS_BLOCKS(8, false);
  }
#undef CALL_LS_BLOCKS
}

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_levelset_sample(zs_rocm_policy *pol, const zs_rocm_levelset *levelset, const float *x, size_t n, float *sdf, float *normal,
                            float *vel) {
  if (!pol || !levelset_ok(levelset) || (n && !x)) return -1;
  Launch L(pol, "LevelSetBoundary sample");
  if (!n) return 0;
  hipLaunchKernelGGL(levelset_sample_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, LevelSetView(*levelset), x, n, sdf, normal, vel);
  return 0;
}

int zs_rocm_levelset_collider_resolve(zs_rocm_policy *pol, const zs_rocm_collider *collider, const zs_rocm_levelset *levelset, const float *x,
                                      float *v, size_t n, int *inside) {
  if (!pol || !levelset_collider_ok(collider, levelset) || (n && (!x || !v))) return -1;
  Launch L(pol, "Collider<LevelSet>::resolveCollision");
  if (!n) return 0;
  LevelSetColliderDev col;
  col.motion = ColliderDev(*collider);
  col.ls = LevelSetView(*levelset);
  hipLaunchKernelGGL(levelset_resolve_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, col, x, v, n, inside);
  return 0;
}

int zs_rocm_mpm_apply_boundary_levelset(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, const zs_rocm_bht_3 *tab, float *grid, size_t nblocks,
                                        const zs_rocm_collider *collider, const zs_rocm_levelset *levelset) {
  if (!pol || !p || !tab || !grid || (p->side != 4 && p->side != 8) || !(p->dx > 0.f) || !levelset_collider_ok(collider, levelset)) return -1;
  if (nblocks > (size_t)0x7fffffff) return -1;
  Launch L(pol, "ApplyBoundaryConditionOnGridBlocks (level set)");
  levelset_blocks_enqueue(L.stream, p, (const int *)tab->t.dev().activeKeys, grid, nblocks, collider, levelset, nullptr);
  return 0;
}

}  // extern "C"
