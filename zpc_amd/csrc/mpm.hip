// mpm.hip -- partition, index buckets, binning, grid update, constitutive test entries, owner classification, halo pack/unpack: kernels and entry points.
// Replaces, behind include/zs_rocm.h:
//   ComputeSparsity / EnlargeSparsity        simulation/sparsity/SparsityOp.hpp:59-115
//   ComputeGridBlockVelocity                 simulation/grid/GridOp.hpp:71-108
#include "hashtable.hpp"
#include "mpm_update_stress_kernel.hpp"

namespace zsr {

void exclusive_scan_u32(Launch &L, const unsigned *in, size_t n, unsigned *out);
void radix_sort_pair_u32(Launch &L, const unsigned *kin, const int *vin, unsigned *kout, int *vout, size_t n, int sbit, int ebit);

// ======================================================================================= sparsity
static __global__ __launch_bounds__(256) void compute_sparsity_kernel(BhtDev t, Port<float> pos, size_t n, float dxinv, int side, int kscale) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int b[3] = {0, 0, 0};
  if (valid) {
    float p[3];
    load_attr<3>(pos, i, p);
#pragma unroll
    for (int d = 0; d < 3; ++d) b[d] = floordiv((int)floorf(p[d] * dxinv + 0.5f) + (-2), side) * kscale;
  }
  // neighbouring lanes usually carry the same block: let only the first lane of a run insert (the others
  // would get sentinel_v back from insert anyway)
  const int px = shfl_up(b[0], 1), py = shfl_up(b[1], 1), pz = shfl_up(b[2], 1);
  const bool pvalid = shfl_up((int)valid, 1) != 0;
  const bool dup = lane_id() != 0 && pvalid && px == b[0] && py == b[1] && pz == b[2];
  if (valid && !dup) bht_insert<3>(t, b);
}
static __global__ __launch_bounds__(256) void enlarge_sparsity_kernel(BhtDev t, int nblocks, int lo0, int lo1, int lo2, int e0, int e1, int e2, int kscale) {
  // thread per (block, offset)
  const int per = e0 * e1 * e2;
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)nblocks * per) return;
  const int i = (int)(g / per), o = (int)(g % per);
  const int dx = lo0 + o / (e1 * e2), dy = lo1 + (o / e2) % e1, dz = lo2 + o % e2;
  int k[3] = {t.activeKeys[3 * (size_t)i] + dx * kscale, t.activeKeys[3 * (size_t)i + 1] + dy * kscale, t.activeKeys[3 * (size_t)i + 2] + dz * kscale};
  bht_insert<3>(t, k);
}
// the same functors on a zs::HashTable<i32,3,int> (simulation/sparsity/SparsityOp.hpp:59-115 are written against HashTableView)
static __global__ __launch_bounds__(256) void compute_sparsity_ht_kernel(HtDev t, Port<float> pos, size_t n, float dxinv, int side) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int b[3] = {0, 0, 0};
  if (valid) {
    float p[3];
    load_attr<3>(pos, i, p);
#pragma unroll
    for (int d = 0; d < 3; ++d) b[d] = floordiv((int)floorf(p[d] * dxinv + 0.5f) + (-2), side);
  }
  const int px = shfl_up(b[0], 1), py = shfl_up(b[1], 1), pz = shfl_up(b[2], 1);
  const bool pvalid = shfl_up((int)valid, 1) != 0;
  const bool dup = lane_id() != 0 && pvalid && px == b[0] && py == b[1] && pz == b[2];
  if (valid && !dup) ht_insert<3>(t, b);
}
static __global__ __launch_bounds__(256) void enlarge_sparsity_ht_kernel(HtDev t, int nblocks, int lo0, int lo1, int lo2, int e0, int e1, int e2) {
  const int per = e0 * e1 * e2;
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)nblocks * per) return;
  const int i = (int)(g / per), o = (int)(g % per);
  int k[3] = {t.activeKeys[3 * (size_t)i] + lo0 + o / (e1 * e2), t.activeKeys[3 * (size_t)i + 1] + lo1 + (o / e2) % e1,
              t.activeKeys[3 * (size_t)i + 2] + lo2 + o % e2};
  ht_insert<3>(t, k);
}
// index_buckets_for_particles (simulation/particle/Query.tpp:9-58): ComputeSparsity with blockLen 1 / offset 0, then
// SpatiallyCount (sparsity/SparsityOp.hpp:117-152)
static __global__ __launch_bounds__(256) void ib_cells_kernel(HtDev t, Port<float> pos, size_t n, float dxinv, float displacement, int *full) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int b[3] = {0, 0, 0};
  if (valid) {
    float p[3];
    load_attr<3>(pos, i, p);
#pragma unroll
    for (int d = 0; d < 3; ++d) b[d] = (int)floorf(p[d] * dxinv + displacement);
  }
  const int px = shfl_up(b[0], 1), py = shfl_up(b[1], 1), pz = shfl_up(b[2], 1);
  const bool pvalid = shfl_up((int)valid, 1) != 0;
  const bool dup = lane_id() != 0 && pvalid && px == b[0] && py == b[1] && pz == b[2];
  if (valid && !dup && ht_insert<3>(t, b) == HT_FAIL) *full = 1;  // table too small for the occupied cells: the host grows it and retries
}
static __global__ __launch_bounds__(256) void ib_count_kernel(HtDev t, Port<float> pos, size_t n, float dxinv, float displacement, unsigned *counts,
                                                       unsigned *cellOf, int *ids) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[3];
  load_attr<3>(pos, i, p);
  int b[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) b[d] = (int)floorf(p[d] * dxinv + displacement);
  int c = ht_query<3>(t, b);
  if (c < 0) c = *t.cnt;  // not in the table (cannot happen after a successful cell pass): the spare last bucket, never out of bounds
  cellOf[i] = (unsigned)c;
  ids[i] = (int)i;
  atomicAdd(&counts[c], 1u);
}
// buckets over the cells of a block partition (zs_rocm_index_buckets_for_partition): bucket = block * side^3 + cell id of the cell
// that contains the particle; particles whose cell is not in the partition go to the extra bucket `nbuckets`
static __global__ __launch_bounds__(256) void ib_dense_count_kernel(BhtDev t, Port<float> pos, size_t n, float dxinv, int side, int kscale,
                                                             int nbuckets, unsigned *counts, unsigned *cellOf, int *ids) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[3];
  load_attr<3>(pos, i, p);
  int key[3], loc[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int c = (int)floorf(p[d] * dxinv);
    loc[d] = c & (side - 1);
    key[d] = (c - loc[d]) / side * kscale;
  }
  const int b = bht_query<3>(t, key);
  const int bucket = b < 0 ? nbuckets : b * side * side * side + (loc[0] * side + loc[1]) * side + loc[2];
  cellOf[i] = (unsigned)bucket;
  ids[i] = (int)i;
  atomicAdd(&counts[bucket], 1u);
}
static __global__ __launch_bounds__(256) void build_neighbors_kernel(BhtDev t, int nblocks, int *nbr, int kscale) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)nblocks * 8) return;
  const int i = (int)(g >> 3), o = (int)(g & 7);
  int k[3] = {t.activeKeys[3 * (size_t)i] + (o >> 2) * kscale, t.activeKeys[3 * (size_t)i + 1] + ((o >> 1) & 1) * kscale,
              t.activeKeys[3 * (size_t)i + 2] + (o & 1) * kscale};
  nbr[g] = bht_query<3>(t, k);
}

// ======================================================================================= binning
template <int SIDE>
static __global__ __launch_bounds__(256) void bin_count_kernel(BhtDev t, Port<float> pos, size_t n, float dx, unsigned *cellCount,
                                                        unsigned *cellOf, unsigned *rankOf, int *err, int kscale) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[3];
  load_attr<3>(pos, i, p);
  int key[3], loc[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int c = (int)floorf(p[d] * (1.0f / dx) - 0.5f);
    loc[d] = c & (SIDE - 1);
    key[d] = (c - loc[d]) / SIDE * kscale;
  }
  const int b = bht_query<3>(t, key);
  if (b < 0) {
    *err = 1;
    cellOf[i] = 0xffffffffu;
    return;
  }
  const int sub = SIDE == 4 ? 0 : (((loc[0] >> 2) * 2 + (loc[1] >> 2)) * 2 + (loc[2] >> 2));
  const unsigned cell = ((unsigned)b * bins_per_block<SIDE>() + sub) * 64u +
                        (unsigned)(((loc[0] & 3) * 4 + (loc[1] & 3)) * 4 + (loc[2] & 3));
  cellOf[i] = cell;
  rankOf[i] = atomicAdd(&cellCount[cell], 1u);
}
static __global__ __launch_bounds__(256) void bin_place_kernel(size_t n, const unsigned *cellStart, const unsigned *cellOf,
                                                        const unsigned *rankOf, int *byCell) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned c = cellOf[i];
  if (c != 0xffffffffu) byCell[cellStart[c] + rankOf[i]] = (int)i;
}
// one wave per bin, lane = cell: (cell, rank) order -> (rank, cell) order.  The ranks handed out by the counting pass are in
// arrival order of its atomics; the lane first sorts its cell's particle ids (odd-even transposition network in registers,
// K = 8 / 16 / 32 chosen per bin), so that within a cell the particles keep their previous relative order: a particle that
// did not change cell stays in "its" round, and the permutation of a re-ordering fused step is the identity except around the
// movers (coalesced reads through `order`).
template <int K>
__device__ __forceinline__ void bin_rr_emit(unsigned cnt, unsigned st, const int *byCell, int *order, unsigned &base, unsigned long long lt) {
  int ids[K];
#pragma unroll
  for (int k = 0; k < K; ++k) ids[k] = (unsigned)k < cnt ? byCell[st + k] : 0x7fffffff;
#pragma unroll
  for (int pass = 0; pass < K; ++pass)
#pragma unroll
    for (int k = pass & 1; k + 1 < K; k += 2) {
      const int a = ids[k], b = ids[k + 1];
      ids[k] = a < b ? a : b;
      ids[k + 1] = a < b ? b : a;
    }
#pragma unroll
  for (int r = 0; r < K; ++r) {
    const bool has = cnt > (unsigned)r;
    const unsigned long long m = __ballot(has);
    if (!m) return;
    if (has) order[base + (unsigned)__popcll(m & lt)] = ids[r];
    base += (unsigned)__popcll(m);
  }
}
static __global__ __launch_bounds__(64) void bin_roundrobin_kernel(int nbins, const unsigned *cellStart, const unsigned *cellCount,
                                                            const int *byCell, int *order, int *binStart, unsigned total) {
  const int bin = blockIdx.x, c = threadIdx.x;
  const unsigned cnt = cellCount[(size_t)bin * 64 + c], st = cellStart[(size_t)bin * 64 + c];
  unsigned base = shfl(st, 0);
  if (c == 0) {
    binStart[bin] = (int)base;
    if (bin == nbins - 1) binStart[nbins] = (int)total;
  }
  const unsigned long long lt = lanemask_lt();
  unsigned mx = cnt;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned o = shfl_down(mx, d);
    mx = o > mx ? o : mx;
  }
  mx = shfl(mx, 0);
  if (mx <= 8u) bin_rr_emit<8>(cnt, st, byCell, order, base, lt);
  else if (mx <= 16u) bin_rr_emit<16>(cnt, st, byCell, order, base, lt);
  else bin_rr_emit<32>(cnt, st, byCell, order, base, lt);
  for (unsigned r = 32;; ++r) {  // cells with more than 32 particles: the rest in arrival order
    const bool has = cnt > r;
    const unsigned long long m = __ballot(has);
    if (!m) break;
    if (has) order[base + (unsigned)__popcll(m & lt)] = byCell[st + r];
    base += (unsigned)__popcll(m);
  }
}

// ======================================================================================= grid update
template <int SIDE>
static __global__ __launch_bounds__(256) void grid_update_kernel(float *grid, size_t nblocks, float dt, float e0, float e1, float e2,
                                                          float *maxVelSqr) {
  constexpr int NC = SIDE * SIDE * SIDE;
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  float vsq = 0.f;
  if (g < nblocks * NC) {
    const size_t b = g / NC, c = g % NC;
    float *blk = grid + b * 7 * NC + c;
    float mass = blk[0];
    if (mass != 0.f) {
      mass = 1.f / mass;
      const float v0 = blk[1 * NC] * mass + e0 * dt, v1 = blk[2 * NC] * mass + e1 * dt, v2 = blk[3 * NC] * mass + e2 * dt;
      blk[1 * NC] = v0;
      blk[2 * NC] = v1;
      blk[3 * NC] = v2;
      vsq = v0 * v0 + v1 * v1 + v2 * v2;
    }
  }
  if (maxVelSqr) {  // atomic_max(maxVel, |v|^2) (GridOp.hpp:103-104): workgroup max, then at most one int-ordered atomic
    // One device-wide word takes ~90 atomics per microsecond: an atomic per wave of a 27 200-block grid (217 k of them) cost 2.4 ms.
    // The maximum only grows, so a workgroup first looks at the current value and stays silent unless it can raise it.
    __shared__ float wmax[4];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) vsq = fmaxf(vsq, shfl_down(vsq, d));
    if (lane_id() == 0) wmax[wave_id()] = vsq;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      if (m > 0.f && __float_as_int(m) > __hip_atomic_load((int *)maxVelSqr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax((int *)maxVelSqr, __float_as_int(m));
    }
  }
}

// ======================================================================================= misc kernels
template <int MODEL> __global__ void stress_kernel(MpmDev mp, float *F, float *logJp, size_t n, float *PF) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float f[9], pf[9];
#pragma unroll
  for (int d = 0; d < 9; ++d) f[d] = F[9 * i + d];
  float lj = 0.f;
  if constexpr (model_uses_logjp(MODEL)) lj = logJp[i];
  const float C0[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // the fluid's viscous part needs C: zero through this entry
  model_stress<MODEL, true>(mp.mat, lj, f, pf, C0);
  if constexpr (model_uses_logjp(MODEL)) logJp[i] = lj;
  if constexpr (MODEL != ZS_MPM_FIXED_COROTATED) {  // the plastic models return the projected F
#pragma unroll
    for (int d = 0; d < 9; ++d) F[9 * i + d] = f[d];
  }
#pragma unroll
  for (int d = 0; d < 9; ++d) PF[9 * i + d] = pf[d];
}
static __global__ void svd_kernel(const float *F, size_t n, float *U, float *S, float *V) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float f[9], u[9], s[3], v[9];
#pragma unroll
  for (int d = 0; d < 9; ++d) f[d] = F[9 * i + d];
  svd3(f, u, s, v);
#pragma unroll
  for (int d = 0; d < 9; ++d) {
    U[9 * i + d] = u[d];
    V[9 * i + d] = v[d];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) S[3 * i + d] = s[d];
}
// owner rank of every particle under the block-aligned box split of zpc_amd/dist.py (cell_box): cell = floor(x / dx) clamped to
// the global box; along axis d the box [lo, hi) is cut at lo + (n k / dims) rounded down to a multiple of `align`
struct OwnerSplit {
  int lo[3], hi[3], dims[3], align;
};
static __global__ __launch_bounds__(256) void owner_rank_kernel(Port<float> pos, size_t n, float dxinv, OwnerSplit sp, int *owner) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[3];
  load_attr<3>(pos, i, p);
  int rc[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int c = (int)floorf(p[d] * dxinv);
    c = c < sp.lo[d] ? sp.lo[d] : (c >= sp.hi[d] ? sp.hi[d] - 1 : c);
    const int len = sp.hi[d] - sp.lo[d];
    int r = 0;
    for (int k = 1; k < sp.dims[d]; ++k) {
      int cut = sp.lo[d] + (int)(((long long)len * k) / sp.dims[d]);
      cut = floordiv(cut, sp.align) * sp.align;
      r += c >= cut;
    }
    rc[d] = r;
  }
  owner[i] = (rc[0] * sp.dims[1] + rc[1]) * sp.dims[2] + rc[2];
}
// per-workgroup LDS histogram of the owner ranks, one global atomic per (workgroup, rank that occurs)
static __global__ __launch_bounds__(256) void owner_count_kernel(const int *owner, size_t n, int world, int *counts) {
  extern __shared__ int ocHist[];
  for (int r = threadIdx.x; r < world; r += 256) ocHist[r] = 0;
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int o = owner[i];
    if ((unsigned)o < (unsigned)world) atomicAdd(&ocHist[o], 1);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < world; r += 256)
    if (ocHist[r]) atomicAdd(&counts[r], ocHist[r]);
}
static __global__ void halo_pack_kernel(const float *grid, const int *blocks, size_t nb, int nc, int chn0, int nchn, float *buf) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per = (size_t)nchn * nc;
  if (g >= nb * per) return;
  const size_t i = g / per, r = g % per;
  buf[g] = grid[((size_t)blocks[i] * 7 + chn0) * nc + r];
}
// MODE 0: set, 1: add (each block appears once in `blocks`), 2: atomic add (the list may name a block several times, e.g. the
// concatenated messages of several peers that all share a corner block)
template <int MODE> __global__ void halo_unpack_kernel(float *grid, const int *blocks, size_t nb, int nc, int chn0, int nchn, const float *buf) {
  size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per = (size_t)nchn * nc;
  if (g >= nb * per) return;
  const size_t i = g / per, r = g % per;
  float *dst = grid + ((size_t)blocks[i] * 7 + chn0) * nc + r;
  if constexpr (MODE == 2) unsafeAtomicAdd(dst, buf[g]);
  else if constexpr (MODE == 1) *dst += buf[g];
  else *dst = buf[g];
}

}  // namespace zsr

using namespace zsr;

extern "C" {


void zs_rocm_mpm_compute_sparsity(zs_rocm_policy *pol, zs_rocm_bht_3 *tab, zs_rocm_attr pos, size_t n, float dx, int side,
                                  int keyIsOrigin) {
  Launch L(pol, "ComputeSparsity");
  if (!n) return;
  hipLaunchKernelGGL(compute_sparsity_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, tab->t.dev(), make_port<float>(pos), n,
                     1.0f / dx, side, keyIsOrigin ? side : 1);
}
void zs_rocm_mpm_partition_for_particles(zs_rocm_policy *pol, zs_rocm_hashtable *tab, zs_rocm_attr pos, size_t n, float dx,
                                         int blocklen) {
  if (tab->dim != 3) return;
  zs_rocm_hashtable_reset(pol, tab, 1);  // CleanSparsity (SparsityCompute.tpp:19)
  Launch L(pol, "partition_for_particles");
  if (!n) return;
  hipLaunchKernelGGL(compute_sparsity_ht_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, tab->dev(), make_port<float>(pos), n,
                     1.0f / dx, blocklen);
}
zs_rocm_index_buckets *zs_rocm_index_buckets_create(void) { return new zs_rocm_index_buckets; }
void zs_rocm_index_buckets_destroy(zs_rocm_index_buckets *ib) {
  if (!ib) return;
  if (ib->table) zs_rocm_hashtable_destroy(ib->table);
  (void)hipFree(ib->indices); (void)hipFree(ib->offsets); (void)hipFree(ib->counts);
  delete ib;
}
void zs_rocm_index_buckets_get_view(const zs_rocm_index_buckets *ib, zs_rocm_index_buckets_view *v) {
  v->table = ib->table; v->indices = ib->indices; v->offsets = ib->offsets; v->counts = ib->counts;
  v->numBuckets = ib->numBuckets; v->numEntries = ib->numEntries; v->dx = ib->dx;
}
void zs_rocm_index_buckets_for_particles(zs_rocm_policy *pol, zs_rocm_index_buckets *ib, zs_rocm_attr pos, size_t n, float dx,
                                         float displacement, size_t expectedCells) {
  ib->dx = dx;
  ib->displacement = displacement;
  ib->dense = 0;
  // a time loop rebuilds the buckets every step: table and arrays are kept while they are large enough (hipMalloc / hipFree
  // synchronise the device and cost more than the kernels below)
  size_t want = expectedCells ? expectedCells : n;
  // the table lives on the device the policy runs on (one process per GPU: that is the rank's device, not device 0)
  const int tdev = pol->device >= 0 ? pol->device : current_device();
  if (ib->table && ib->table->devid != tdev) { zs_rocm_hashtable_destroy(ib->table); ib->table = nullptr; ib->tableFor = 0; }
  if (ib->table && ib->tableFor >= want && ib->tableFor <= 4 * want) {
    want = ib->tableFor;
    zs_rocm_hashtable_reset(pol, ib->table, 1);
  } else {
    if (ib->table) zs_rocm_hashtable_destroy(ib->table);
    ib->table = zs_rocm_hashtable_create(3, want, 1, tdev);  // Query.tpp:27 (created reset)
    ib->tableFor = want;
  }
  ib->numEntries = (int)n;
  ib->numBuckets = 0;
  if (!n) return;
  Launch L(pol, "index_buckets_for_particles");
  const float dxinv = 1.0f / dx;
  int nc = 0;
  int *full = (int *)L.temp(sizeof(int));
  for (;;) {
    ZSR_CHECK(hipMemsetAsync(full, 0, sizeof(int), L.stream));
    hipLaunchKernelGGL(ib_cells_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, ib->table->dev(), make_port<float>(pos), n, dxinv,
                       displacement, full);
    int isFull = 0;
    ZSR_CHECK(hipMemcpyAsync(&nc, ib->table->cnt, sizeof(int), hipMemcpyDeviceToHost, L.stream));
    ZSR_CHECK(hipMemcpyAsync(&isFull, full, sizeof(int), hipMemcpyDeviceToHost, L.stream));
    ZSR_CHECK(hipStreamSynchronize(L.stream));
    if (!isFull) break;
    // `expectedCells` underestimated the occupied cells by more than the table's 16x headroom: a larger table, again.  The
    // reference sizes the table by the particle count (an upper bound of the cells), which ends the loop at the latest.
    if (want >= n) {
      report_error(hipErrorOutOfMemory, "index_buckets_for_particles: hash table full at one slot per particle", __FILE__, __LINE__);
      ib->numEntries = 0;
      return;
    }
    want = std::min(n, want * 8);
    zs_rocm_hashtable_destroy(ib->table);
    ib->table = zs_rocm_hashtable_create(3, want, 1, tdev);
    ib->tableFor = want;
  }
  ib->numBuckets = nc;
  const size_t numCells = (size_t)nc + 1;  // Query.tpp:36
  if (numCells > ib->capCells) {
    (void)hipFree(ib->offsets); (void)hipFree(ib->counts);
    ib->capCells = numCells + numCells / 2;
    ZSR_CHECK(hipMalloc((void **)&ib->counts, ib->capCells * sizeof(int)));
    ZSR_CHECK(hipMalloc((void **)&ib->offsets, ib->capCells * sizeof(int)));
  }
  if (n > ib->capEntries) {
    (void)hipFree(ib->indices);
    ib->capEntries = n;
    ZSR_CHECK(hipMalloc((void **)&ib->indices, n * sizeof(int)));
  }
  ZSR_CHECK(hipMemsetAsync(ib->counts, 0, numCells * sizeof(int), L.stream));
  unsigned *cellOf = (unsigned *)L.temp(sizeof(unsigned) * n), *cellSorted = (unsigned *)L.temp(sizeof(unsigned) * n);
  int *ids = (int *)L.temp(sizeof(int) * n);
  hipLaunchKernelGGL(ib_count_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, ib->table->dev(), make_port<float>(pos), n, dxinv,
                     displacement, (unsigned *)ib->counts, cellOf, ids);
  exclusive_scan_u32(L, (const unsigned *)ib->counts, numCells, (unsigned *)ib->offsets);
  // SpatiallyDistribute as a stable sort of (bucket, particle id): ids ascend inside a bucket
  int bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < numCells) ++bits;
  radix_sort_pair_u32(L, cellOf, ids, cellSorted, ib->indices, n, 0, bits);
}
void zs_rocm_index_buckets_for_partition(zs_rocm_policy *pol, zs_rocm_index_buckets *ib, zs_rocm_attr pos, size_t n, float dx,
                                         const zs_rocm_bht_3 *tab, int side, int keyIsOrigin) {
  ib->dx = dx;
  ib->displacement = 0.f;
  if (ib->table) { zs_rocm_hashtable_destroy(ib->table); ib->table = nullptr; ib->tableFor = 0; }
  ib->dense = 1;
  ib->denseSide = side;
  ib->numEntries = (int)n;
  ib->numBuckets = 0;
  Launch L(pol, "index_buckets_for_partition");
  const int nb = bht_size(tab->t, L.stream);
  if (!n || !nb || (side != 4 && side != 8)) return;
  const size_t nbuckets = (size_t)nb * side * side * side, numCells = nbuckets + 2;  // + the bucket of the unlisted particles + end
  ib->numBuckets = (int)nbuckets;
  if (numCells > ib->capCells) {
    (void)hipFree(ib->offsets); (void)hipFree(ib->counts);
    ib->capCells = numCells + numCells / 2;
    ZSR_CHECK(hipMalloc((void **)&ib->counts, ib->capCells * sizeof(int)));
    ZSR_CHECK(hipMalloc((void **)&ib->offsets, ib->capCells * sizeof(int)));
  }
  if (n > ib->capEntries) {
    (void)hipFree(ib->indices);
    ib->capEntries = n;
    ZSR_CHECK(hipMalloc((void **)&ib->indices, n * sizeof(int)));
  }
  ZSR_CHECK(hipMemsetAsync(ib->counts, 0, numCells * sizeof(int), L.stream));
  unsigned *cellOf = (unsigned *)L.temp(sizeof(unsigned) * n), *cellSorted = (unsigned *)L.temp(sizeof(unsigned) * n);
  int *ids = (int *)L.temp(sizeof(int) * n);
  hipLaunchKernelGGL(ib_dense_count_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, tab->t.dev(), make_port<float>(pos), n, 1.0f / dx,
                     side, keyIsOrigin ? side : 1, (int)nbuckets, (unsigned *)ib->counts, cellOf, ids);
  exclusive_scan_u32(L, (const unsigned *)ib->counts, numCells, (unsigned *)ib->offsets);
  int bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < numCells) ++bits;
  radix_sort_pair_u32(L, cellOf, ids, cellSorted, ib->indices, n, 0, bits);  // stable: ids ascend inside a bucket
}
void zs_rocm_mpm_enlarge_sparsity__hashtable(zs_rocm_policy *pol, zs_rocm_hashtable *tab, const int lo[3], const int hi[3]) {
  if (tab->dim != 3) return;
  Launch L(pol, "enlarge_sparsity");
  int nb = 0;
  ZSR_CHECK(hipMemcpyAsync(&nb, tab->cnt, sizeof(int), hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
  const int e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
  if (nb <= 0 || e0 <= 0 || e1 <= 0 || e2 <= 0) return;
  hipLaunchKernelGGL(enlarge_sparsity_ht_kernel, dim3(ceil_div((size_t)nb * e0 * e1 * e2, 256)), dim3(256), 0, L.stream, tab->dev(), nb,
                     lo[0], lo[1], lo[2], e0, e1, e2);
}
void zs_rocm_mpm_enlarge_sparsity(zs_rocm_policy *pol, zs_rocm_bht_3 *tab, const int lo[3], const int hi[3], int keyStride) {
  Launch L(pol, "EnlargeSparsity");
  const int nb = bht_size(tab->t, L.stream);
  const int e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
  if (nb == 0 || e0 <= 0 || e1 <= 0 || e2 <= 0) return;
  hipLaunchKernelGGL(enlarge_sparsity_kernel, dim3(ceil_div((size_t)nb * e0 * e1 * e2, 256)), dim3(256), 0, L.stream, tab->t.dev(), nb,
                     lo[0], lo[1], lo[2], e0, e1, e2, keyStride > 0 ? keyStride : 1);
}
void zs_rocm_mpm_build_neighbors(zs_rocm_policy *pol, const zs_rocm_bht_3 *tab, int *nbr, int keyStride) {
  Launch L(pol, "build_neighbors");
  const int nb = bht_size(tab->t, L.stream);
  if (!nb) return;
  hipLaunchKernelGGL(build_neighbors_kernel, dim3(ceil_div((size_t)nb * 8, 256)), dim3(256), 0, L.stream, tab->t.dev(), nb, nbr, keyStride > 0 ? keyStride : 1);
}

void zs_rocm_mpm_bin_particles(zs_rocm_policy *pol, const zs_rocm_bht_3 *tab, zs_rocm_attr pos, size_t n, float dx, int side,
                               int keyIsOrigin, int *order, int *binStart, unsigned *cellCount) {
  Launch L(pol, "bin_particles");
  const int nb = bht_size(tab->t, L.stream);
  if (nb == 0) return;
  const int nbins = nb * (side == 4 ? 1 : 8);
  const size_t ncells = (size_t)nbins * 64;
  unsigned *cellStart = (unsigned *)L.temp(sizeof(unsigned) * (ncells + 1));
  unsigned *cellOf = (unsigned *)L.temp(sizeof(unsigned) * (n + 1));
  unsigned *rankOf = (unsigned *)L.temp(sizeof(unsigned) * (n + 1));
  int *byCell = (int *)L.temp(sizeof(int) * (n + 1));
  int *err = (int *)L.temp(sizeof(int));
  ZSR_CHECK(hipMemsetAsync(cellCount, 0, sizeof(unsigned) * ncells, L.stream));
  ZSR_CHECK(hipMemsetAsync(err, 0, sizeof(int), L.stream));
  BhtDev t = tab->t.dev();
  Port<float> pp = make_port<float>(pos);
  if (n) {
    if (side == 4)
      hipLaunchKernelGGL((bin_count_kernel<4>), dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, t, pp, n, dx, cellCount, cellOf, rankOf, err, keyIsOrigin ? side : 1);
    else
      hipLaunchKernelGGL((bin_count_kernel<8>), dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, t, pp, n, dx, cellCount, cellOf, rankOf, err, keyIsOrigin ? side : 1);
  }
  exclusive_scan_u32(L, cellCount, ncells, cellStart);
  if (n)
    hipLaunchKernelGGL(bin_place_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, n, (const unsigned *)cellStart,
                       (const unsigned *)cellOf, (const unsigned *)rankOf, byCell);
  hipLaunchKernelGGL(bin_roundrobin_kernel, dim3(nbins), dim3(64), 0, L.stream, nbins, (const unsigned *)cellStart,
                     (const unsigned *)cellCount, (const int *)byCell, order, binStart, (unsigned)n);
  int herr = 0;
  ZSR_CHECK(hipMemcpyAsync(&herr, err, sizeof(int), hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
  if (herr) fprintf(stderr, "[zs_rocm] bin_particles: particles outside the partition were dropped from the bins\n");
}


void zs_rocm_mpm_grid_update(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, float *grid, size_t nblocks, const float extf[3],
                             float *maxVelSqr) {
  Launch L(pol, "ComputeGridBlockVelocity");
  if (!nblocks) return;
  const size_t nc = (size_t)p->side * p->side * p->side;
  if (p->side == 4)
    hipLaunchKernelGGL((grid_update_kernel<4>), dim3(ceil_div(nblocks * nc, 256)), dim3(256), 0, L.stream, grid, nblocks, p->dt, extf[0],
                       extf[1], extf[2], maxVelSqr);
  else
    hipLaunchKernelGGL((grid_update_kernel<8>), dim3(ceil_div(nblocks * nc, 256)), dim3(256), 0, L.stream, grid, nblocks, p->dt, extf[0],
                       extf[1], extf[2], maxVelSqr);
}



int zs_rocm_mpm_stress_channels(void) { return STRESS_N; }
void zs_rocm_mpm_update_stress(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, zs_rocm_particles ps) {
  Launch L(pol, "update_stress");
  if (!ps.n || !ps.stress.base) return;
  MpmDev mp = make_dev(p);
  ParticlesDev pd = make_particles(ps);
#define CALL_UPDATE_STRESS(S, M) hipLaunchKernelGGL((update_stress_kernel<M>), dim3(ceil_div(ps.n, 256)), dim3(256), 0, L.stream, mp, pd)
  if (p->model < ZS_MPM_FIXED_COROTATED || p->model > ZS_MPM_EQUATION_OF_STATE) return;
  ZSR_DISPATCH_PURE_(0, p->model, CALL_UPDATE_STRESS)
}

void zs_rocm_mpm_stress(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, float *F, float *logJp, size_t n, float *PF) {
  Launch L(pol, "compute_stress");
  if (!n) return;
  MpmDev mp = make_dev(p);
#define CALL_STRESS(S, M) hipLaunchKernelGGL((stress_kernel<M>), dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, mp, F, logJp, n, PF)
  if (p->model < ZS_MPM_FIXED_COROTATED || p->model > ZS_MPM_EQUATION_OF_STATE) return;
  ZSR_DISPATCH_PURE_(0, p->model, CALL_STRESS)
}
float zs_rocm_nacc_msqr(float fa) {  // NACCConfig::mohrColumbFriction / M / Msqr, dim = 3 (physics/ConstitutiveModel.hpp:771-785)
  const int dim = 3;
  const float sin_phi = std::sin(fa);  // the reference passes `fa` to sin() as it is
  const float mcf = std::sqrt(2.f / 3.f) * 2.f * sin_phi / (3.f - sin_phi);
  const float M = mcf * dim / std::sqrt(2.f / (6.f - dim));
  return M * M;
}
void zs_rocm_svd3(zs_rocm_policy *pol, const float *F, size_t n, float *U, float *S, float *V) {
  Launch L(pol, "svd3");
  if (!n) return;
  hipLaunchKernelGGL(svd_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, F, n, U, S, V);
}

void zs_rocm_mpm_owner_rank(zs_rocm_policy *pol, zs_rocm_attr pos, size_t n, float dx, const int lo[3], const int hi[3], const int dims[3],
                            int align, int *owner) {
  Launch L(pol, "owner_rank");
  if (!n) return;
  OwnerSplit sp;
  for (int d = 0; d < 3; ++d) { sp.lo[d] = lo[d]; sp.hi[d] = hi[d]; sp.dims[d] = dims[d]; }
  sp.align = align < 1 ? 1 : align;
  hipLaunchKernelGGL(owner_rank_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, make_port<float>(pos), n, 1.0f / dx, sp, owner);
}
// counts[r] = number of i with owner[i] == r, r in [0, world) (world <= 1024): how many particles a migration sends to each rank
void zs_rocm_mpm_owner_counts(zs_rocm_policy *pol, const int *owner, size_t n, int world, int *counts) {
  Launch L(pol, "owner_counts");
  if (world < 1 || world > 1024) return;
  ZSR_CHECK(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)world, L.stream));
  if (!n) return;
  const unsigned blocks = ceil_div(n, 256 * 16) < 2048u ? ceil_div(n, 256 * 16) : 2048u;
  hipLaunchKernelGGL(owner_count_kernel, dim3(blocks), dim3(256), sizeof(int) * (size_t)world, L.stream, owner, n, world, counts);
}
void zs_rocm_mpm_halo_pack(zs_rocm_policy *pol, const float *grid, const int *blocks, size_t nb, int side, int chn0, int nchn, float *buf) {
  Launch L(pol, "halo_pack");
  const int nc = side * side * side;
  if (!nb) return;
  hipLaunchKernelGGL(halo_pack_kernel, dim3(ceil_div(nb * nchn * nc, 256)), dim3(256), 0, L.stream, grid, blocks, nb, nc, chn0, nchn, buf);
}
void zs_rocm_mpm_halo_unpack(zs_rocm_policy *pol, float *grid, const int *blocks, size_t nb, int side, int chn0, int nchn, const float *buf,
                             int add) {
  Launch L(pol, "halo_unpack");
  const int nc = side * side * side;
  if (!nb) return;
  if (add == 2)
    hipLaunchKernelGGL((halo_unpack_kernel<2>), dim3(ceil_div(nb * nchn * nc, 256)), dim3(256), 0, L.stream, grid, blocks, nb, nc, chn0,
                       nchn, buf);
  else if (add)
    hipLaunchKernelGGL((halo_unpack_kernel<1>), dim3(ceil_div(nb * nchn * nc, 256)), dim3(256), 0, L.stream, grid, blocks, nb, nc, chn0,
                       nchn, buf);
  else
    hipLaunchKernelGGL((halo_unpack_kernel<0>), dim3(ceil_div(nb * nchn * nc, 256)), dim3(256), 0, L.stream, grid, blocks, nb, nc, chn0,
                       nchn, buf);
}


}  // extern "C"
