// mesh_barrier.hip -- the IPC contact potential of a mesh on a proximity constraint set for gfx950: total energy and per-vertex gradient
// over the PT and EE pair lists of mesh_proximity.hip, at the mesh's own or at trial positions (include/zensim_rocm/barrier_device.hpp
// has the math).  Bit-reproducible: no float atomics anywhere.
//
//   pairs     lane = pair.  Gathers the four vertices, recomputes distance, parameters and feature at the given positions, writes the
//             pair's energy and (GRAD) its [4][3] contributions to a scratch array, once.  Zero-distance pairs are counted with an integer
//             atomic (a count has no order).  Indices outside the mesh make a pair inactive.
//   energy    float64 sum of the per-pair energies, PT then EE, in a fixed order: workgroup g sums elements [g, g + 1) x RED_CHUNK, thread
//             t the elements t, t + 256, .. of the chunk, then an LDS tree; one workgroup sums the partials the same way.
//   incidence built once per pair of lists, independent of the positions: the 4 (npt + nee) (vertex, 4 pair + corner) entries -- EE pairs
//             numbered behind the PT pairs -- stably sorted by vertex with radix_sort_pair_u32, so a vertex's run is in list order; run
//             starts = exclusive scan of the per-vertex counts (integer atomics).
//   product   the Hessian-vector product H x of the same potential, matrix-free: the pair kernels' siblings write (H_pair x) on a pair's four
//             corners to the same scratch records, and the gather below sums them.  PSD: the positive semi-definite H+ of the header.
//   gradient  lane = vertex: sums the scratch contributions of its run front to back.  The order is the list's, so two calls give the
//             same bytes.  A long run (a hub vertex) costs its lane that many loads and nothing else: runs may straddle anything.
// Built with -ffp-contract=off (zpc_amd/build.py), as every translation unit behind tri_closest / ee_closest.
#include <cfloat>

#include "mesh.hpp"
#include "../../include/zensim_rocm/barrier_device.hpp"

namespace zsr {

void exclusive_scan_u32(Launch &L, const unsigned *in, size_t n, unsigned *out);
void radix_sort_pair_u32(Launch &L, const unsigned *kin, const int *vin, unsigned *kout, int *vout, size_t n, int sbit, int ebit);

constexpr int BAR_BLOCK = 256, RED_CHUNK = 4096;

__global__ __launch_bounds__(256) void barrier_rest_kernel(const float *__restrict__ verts, const int *__restrict__ edges, int ne, float *rest) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int i = edges[2 * (size_t)e], j = edges[2 * (size_t)e + 1];
  const float d0 = verts[3 * (size_t)j] - verts[3 * (size_t)i], d1 = verts[3 * (size_t)j + 1] - verts[3 * (size_t)i + 1];
  const float d2 = verts[3 * (size_t)j + 2] - verts[3 * (size_t)i + 2];
  rest[e] = d0 * d0 + d1 * d1 + d2 * d2;
}

__device__ __forceinline__ void barrier_store(float *contrib, size_t pair, const float (&g)[4][3]) {
  float4 *o = reinterpret_cast<float4 *>(contrib + 12 * pair);  // 48-byte records in a 256-byte aligned array: 16-byte aligned
  o[0] = make_float4(g[0][0], g[0][1], g[0][2], g[1][0]);
  o[1] = make_float4(g[1][1], g[1][2], g[2][0], g[2][1]);
  o[2] = make_float4(g[2][2], g[3][0], g[3][1], g[3][2]);
}

template <bool GRAD>
__global__ __launch_bounds__(BAR_BLOCK) void barrier_pt_kernel(const float *__restrict__ verts, const int *__restrict__ tris, int nv, int nt,
                                                               const int *__restrict__ pairs, int npt, float dHat2, float kappa,
                                                               float *__restrict__ energy, float *__restrict__ contrib, int *status) {
  const int i = blockIdx.x * BAR_BLOCK + threadIdx.x;
  if (i >= npt) return;
  const int vi = pairs[2 * (size_t)i], ti = pairs[2 * (size_t)i + 1];
  float e = 0.f, g[4][3] = {};
  if ((unsigned)vi < (unsigned)nv && (unsigned)ti < (unsigned)nt) {
    const int i0 = tris[3 * (size_t)ti], i1 = tris[3 * (size_t)ti + 1], i2 = tris[3 * (size_t)ti + 2];
    if ((unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv) {
      float p[3], a[3], b[3], c[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        p[d] = verts[3 * (size_t)vi + d];
        a[d] = verts[3 * (size_t)i0 + d];
        b[d] = verts[3 * (size_t)i1 + d];
        c[d] = verts[3 * (size_t)i2 + d];
      }
      if (barrier_pt<GRAD>(p, a, b, c, dHat2, kappa, e, g) == BARRIER_ZERO) atomicAdd(status, 1);
    }
  }
  energy[i] = e;
  if constexpr (GRAD) barrier_store(contrib, (size_t)i, g);
}

template <bool GRAD>
__global__ __launch_bounds__(BAR_BLOCK) void barrier_ee_kernel(const float *__restrict__ verts, const int *__restrict__ edges, int nv, int ne,
                                                               const float *__restrict__ rest, const int *__restrict__ pairs, int nee, float dHat2,
                                                               float kappa, float *__restrict__ energy, float *__restrict__ contrib, int *status) {
  const int i = blockIdx.x * BAR_BLOCK + threadIdx.x;
  if (i >= nee) return;
  const int ei = pairs[2 * (size_t)i], ej = pairs[2 * (size_t)i + 1];
  float e = 0.f, g[4][3] = {};
  if ((unsigned)ei < (unsigned)ne && (unsigned)ej < (unsigned)ne) {
    const int i0 = edges[2 * (size_t)ei], i1 = edges[2 * (size_t)ei + 1], j0 = edges[2 * (size_t)ej], j1 = edges[2 * (size_t)ej + 1];
    float a0[3], a1[3], b0[3], b1[3];  // (the mesh's own edge list: its indices are inside the mesh)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a0[d] = verts[3 * (size_t)i0 + d];
      a1[d] = verts[3 * (size_t)i1 + d];
      b0[d] = verts[3 * (size_t)j0 + d];
      b1[d] = verts[3 * (size_t)j1 + d];
    }
    const float eps = rest ? barrier_ee_eps(rest[ei], rest[ej]) : 0.f;
    if (barrier_ee<GRAD>(a0, a1, b0, b1, dHat2, kappa, eps, e, g) == BARRIER_ZERO) atomicAdd(status + 1, 1);
  }
  energy[i] = e;
  if constexpr (GRAD) barrier_store(contrib, (size_t)i, g);
}

// ---------------------------------------------------------------------------------------------------------------- the float64 total
__device__ __forceinline__ double barrier_block_sum(double s) {
  __shared__ double sm[BAR_BLOCK];
  sm[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int h = BAR_BLOCK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  return sm[0];
}
__global__ __launch_bounds__(BAR_BLOCK) void barrier_partial_kernel(const float *__restrict__ a, size_t na, const float *__restrict__ b, size_t nb,
                                                                    double *partial) {
  const size_t lo = (size_t)blockIdx.x * RED_CHUNK, n = na + nb;
  const size_t hi = lo + RED_CHUNK < n ? lo + RED_CHUNK : n;
  double s = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += BAR_BLOCK) s += (double)(i < na ? a[i] : b[i - na]);
  s = barrier_block_sum(s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(BAR_BLOCK) void barrier_total_kernel(const double *__restrict__ partial, size_t n, double *total) {
  double s = 0.0;
  for (size_t i = threadIdx.x; i < n; i += BAR_BLOCK) s += partial[i];
  s = barrier_block_sum(s);
  if (threadIdx.x == 0) *total = s;
}

// ---------------------------------------------------------------------------------------------------------------- incidence, gradient
// entry c = 4 pair + corner (EE pairs behind the PT pairs): its vertex as the sort key (nv: an index outside the mesh, sorted behind
// every vertex and never read), and the per-vertex counts
__global__ __launch_bounds__(BAR_BLOCK) void barrier_corner_kernel(const int *__restrict__ tris, const int *__restrict__ edges, int nv, int nt, int ne,
                                                                   const int *__restrict__ ptPairs, int npt, const int *__restrict__ eePairs, int nee,
                                                                   unsigned *keys, int *vals, unsigned *counts) {
  const size_t c = (size_t)blockIdx.x * BAR_BLOCK + threadIdx.x;
  if (c >= 4 * ((size_t)npt + (size_t)nee)) return;
  const size_t pair = c >> 2;
  const int k = (int)(c & 3);
  int v = -1;
  if (pair < (size_t)npt) {
    const int vi = ptPairs[2 * pair], ti = ptPairs[2 * pair + 1];
    if ((unsigned)ti < (unsigned)nt) v = k == 0 ? vi : tris[3 * (size_t)ti + (k - 1)];
  } else {
    const int e = eePairs[2 * (pair - npt) + (k >> 1)];
    if ((unsigned)e < (unsigned)ne) v = edges[2 * (size_t)e + (k & 1)];
  }
  const bool ok = (unsigned)v < (unsigned)nv;
  keys[c] = ok ? (unsigned)v : (unsigned)nv;
  vals[c] = (int)c;
  if (ok) atomicAdd(counts + v, 1u);
}

__global__ __launch_bounds__(BAR_BLOCK) void barrier_gather_kernel(const int *__restrict__ starts, const int *__restrict__ entries,
                                                                   const float *__restrict__ contrib, int nv, float *__restrict__ grad) {
  const int v = blockIdx.x * BAR_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const int lo = starts[v], hi = starts[v + 1];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = lo; i < hi; ++i) {
    const float *g = contrib + 3 * (size_t)entries[i];
    s0 += g[0];
    s1 += g[1];
    s2 += g[2];
  }
  grad[3 * (size_t)v] = s0;
  grad[3 * (size_t)v + 1] = s1;
  grad[3 * (size_t)v + 2] = s2;
}

// ---------------------------------------------------------------------------------------------------------------- Hessian-vector product
// lane = pair, as the pair kernels above with the four rows of the direction gathered next to the four vertices: writes (H_pair x) on the
// pair's corners to the same scratch records, which barrier_gather_kernel then sums per vertex in list order
template <bool PSD>
__global__ __launch_bounds__(BAR_BLOCK) void barrier_pt_hvp_kernel(const float *__restrict__ verts, const int *__restrict__ tris, int nv, int nt,
                                                                   const int *__restrict__ pairs, int npt, float dHat2, float kappa,
                                                                   const float *__restrict__ dir, float *__restrict__ contrib, int *status) {
  const int i = blockIdx.x * BAR_BLOCK + threadIdx.x;
  if (i >= npt) return;
  const int vi = pairs[2 * (size_t)i], ti = pairs[2 * (size_t)i + 1];
  float h[4][3] = {};
  if ((unsigned)vi < (unsigned)nv && (unsigned)ti < (unsigned)nt) {
    const int i0 = tris[3 * (size_t)ti], i1 = tris[3 * (size_t)ti + 1], i2 = tris[3 * (size_t)ti + 2];
    if ((unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv) {
      float p[3], a[3], b[3], c[3], x[4][3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        p[d] = verts[3 * (size_t)vi + d];
        a[d] = verts[3 * (size_t)i0 + d];
        b[d] = verts[3 * (size_t)i1 + d];
        c[d] = verts[3 * (size_t)i2 + d];
        x[0][d] = dir[3 * (size_t)vi + d];
        x[1][d] = dir[3 * (size_t)i0 + d];
        x[2][d] = dir[3 * (size_t)i1 + d];
        x[3][d] = dir[3 * (size_t)i2 + d];
      }
      if (barrier_pt_hvp<PSD>(p, a, b, c, x, dHat2, kappa, h) == BARRIER_ZERO) atomicAdd(status, 1);
    }
  }
  barrier_store(contrib, (size_t)i, h);
}

template <bool PSD>
__global__ __launch_bounds__(BAR_BLOCK) void barrier_ee_hvp_kernel(const float *__restrict__ verts, const int *__restrict__ edges, int nv, int ne,
                                                                   const float *__restrict__ rest, const int *__restrict__ pairs, int nee, float dHat2,
                                                                   float kappa, const float *__restrict__ dir, float *__restrict__ contrib,
                                                                   int *status) {
  const int i = blockIdx.x * BAR_BLOCK + threadIdx.x;
  if (i >= nee) return;
  const int ei = pairs[2 * (size_t)i], ej = pairs[2 * (size_t)i + 1];
  float h[4][3] = {};
  if ((unsigned)ei < (unsigned)ne && (unsigned)ej < (unsigned)ne) {
    const int i0 = edges[2 * (size_t)ei], i1 = edges[2 * (size_t)ei + 1], j0 = edges[2 * (size_t)ej], j1 = edges[2 * (size_t)ej + 1];
    float a0[3], a1[3], b0[3], b1[3], x[4][3];  // (the mesh's own edge list: its indices are inside the mesh)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a0[d] = verts[3 * (size_t)i0 + d];
      a1[d] = verts[3 * (size_t)i1 + d];
      b0[d] = verts[3 * (size_t)j0 + d];
      b1[d] = verts[3 * (size_t)j1 + d];
      x[0][d] = dir[3 * (size_t)i0 + d];
      x[1][d] = dir[3 * (size_t)i1 + d];
      x[2][d] = dir[3 * (size_t)j0 + d];
      x[3][d] = dir[3 * (size_t)j1 + d];
    }
    const float eps = rest ? barrier_ee_eps(rest[ei], rest[ej]) : 0.f;
    if (barrier_ee_hvp<PSD>(a0, a1, b0, b1, x, dHat2, kappa, eps, h) == BARRIER_ZERO) atomicAdd(status + 1, 1);
  }
  barrier_store(contrib, (size_t)i, h);
}

static bool barrier_counts_ok(size_t npt, size_t nee) { return npt + nee < ((size_t)1 << 28); }  // 4 (npt + nee) entries: ints, and one radix sort call

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_mesh_set_rest(zs_rocm_policy *pol, zs_rocm_mesh *m, const float *verts) {
  if (!pol || !m || !m->stats) return -1;
  Launch L(pol, "mesh_set_rest");
  if (!m->ne) {
    m->hasRest = true;
    return 0;
  }
  if (!m->restLen2) ZSR_CHECK(hipMalloc((void **)&m->restLen2, sizeof(float) * m->ne));
  hipLaunchKernelGGL(barrier_rest_kernel, dim3(ceil_div(m->ne, 256)), dim3(256), 0, L.stream, verts ? verts : m->verts, m->edges, (int)m->ne,
                     m->restLen2);
  m->hasRest = true;
  return 0;
}

int zs_rocm_mesh_rest(zs_rocm_policy *pol, const zs_rocm_mesh *m, float *restLen2) {
  if (!pol || !m || !m->hasRest || (m->ne && !restLen2)) return -1;
  Launch L(pol, "mesh_rest");
  if (m->ne) ZSR_CHECK(hipMemcpyAsync(restLen2, m->restLen2, sizeof(float) * m->ne, hipMemcpyDeviceToDevice, L.stream));
  return 0;
}

int zs_rocm_mesh_barrier_sizes(const zs_rocm_mesh *m, size_t npt, size_t nee, size_t *sizes) {
  if (!m || !sizes || !barrier_counts_ok(npt, nee)) return -1;
  sizes[0] = m->nv + 1;
  sizes[1] = 4 * (npt + nee);
  sizes[2] = 12 * (npt + nee);
  return 0;
}

int zs_rocm_mesh_barrier_incidence(zs_rocm_policy *pol, const zs_rocm_mesh *m, const int *ptPairs, size_t npt, const int *eePairs, size_t nee,
                                   int *starts, int *entries) {
  if (!pol || !m || !m->stats || !starts || !barrier_counts_ok(npt, nee) || (npt && !ptPairs) || (nee && !eePairs)) return -1;
  const size_t n = 4 * (npt + nee);
  if (n && !entries) return -1;
  Launch L(pol, "mesh_barrier_incidence");
  unsigned *counts = (unsigned *)L.temp(sizeof(unsigned) * (m->nv + 1));
  ZSR_CHECK(hipMemsetAsync(counts, 0, sizeof(unsigned) * (m->nv + 1), L.stream));
  if (n) {
    unsigned *keys = (unsigned *)L.temp(sizeof(unsigned) * n), *sorted = (unsigned *)L.temp(sizeof(unsigned) * n);
    int *vals = (int *)L.temp(sizeof(int) * n);
    hipLaunchKernelGGL(barrier_corner_kernel, dim3(ceil_div(n, BAR_BLOCK)), dim3(BAR_BLOCK), 0, L.stream, m->tris, m->edges, (int)m->nv, (int)m->nt,
                       (int)m->ne, ptPairs, (int)npt, eePairs, (int)nee, keys, vals, counts);
    int bits = 1;
    while (bits < 32 && ((size_t)1 << bits) <= m->nv) ++bits;  // the keys are 0 .. nv
    radix_sort_pair_u32(L, keys, vals, sorted, entries, n, 0, bits);
  }
  exclusive_scan_u32(L, counts, m->nv + 1, (unsigned *)starts);
  return 0;
}

// the shared entry: grad == NULL is energy only
static int barrier_run(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs, size_t nee,
                       float dHat, float kappa, int mollify, const int *starts, const int *entries, float *scratch, float *ptEnergy,
                       float *eeEnergy, double *total, float *grad, int *status) {
  if (!pol || !m || !m->stats || !(dHat > 0.f && dHat <= FLT_MAX) || !(kappa > 0.f && kappa <= FLT_MAX) || (mollify && !m->hasRest)) return -1;
  if (!barrier_counts_ok(npt, nee) || (npt && !ptPairs) || (nee && !eePairs)) return -1;
  if (grad && m->nv && (!starts || (npt + nee && (!entries || !scratch)))) return -1;
  Launch L(pol, grad ? "mesh_barrier_gradient" : "mesh_barrier_energy");
  const float *x = verts ? verts : m->verts;
  const float dHat2 = dHat * dHat;
  int *st = status ? status : (int *)L.temp(sizeof(int) * 2);
  ZSR_CHECK(hipMemsetAsync(st, 0, sizeof(int) * 2, L.stream));
  if (npt && !ptEnergy) ptEnergy = (float *)L.temp(sizeof(float) * npt);
  if (nee && !eeEnergy) eeEnergy = (float *)L.temp(sizeof(float) * nee);
  if (npt) {
    const dim3 grid(ceil_div(npt, BAR_BLOCK)), block(BAR_BLOCK);
    if (grad)
      hipLaunchKernelGGL((barrier_pt_kernel<true>), grid, block, 0, L.stream, x, m->tris, (int)m->nv, (int)m->nt, ptPairs, (int)npt, dHat2, kappa,
                         ptEnergy, scratch, st);
    else
      hipLaunchKernelGGL((barrier_pt_kernel<false>), grid, block, 0, L.stream, x, m->tris, (int)m->nv, (int)m->nt, ptPairs, (int)npt, dHat2, kappa,
                         ptEnergy, (float *)nullptr, st);
  }
  if (nee) {
    const dim3 grid(ceil_div(nee, BAR_BLOCK)), block(BAR_BLOCK);
    const float *rest = mollify ? m->restLen2 : nullptr;
    float *out = grad ? scratch + 12 * npt : nullptr;
    if (grad)
      hipLaunchKernelGGL((barrier_ee_kernel<true>), grid, block, 0, L.stream, x, m->edges, (int)m->nv, (int)m->ne, rest, eePairs, (int)nee, dHat2,
                         kappa, eeEnergy, out, st);
    else
      hipLaunchKernelGGL((barrier_ee_kernel<false>), grid, block, 0, L.stream, x, m->edges, (int)m->nv, (int)m->ne, rest, eePairs, (int)nee, dHat2,
                         kappa, eeEnergy, out, st);
  }
  if (total) {
    const size_t n = npt + nee, parts = (n + RED_CHUNK - 1) / RED_CHUNK;
    double *partial = parts ? (double *)L.temp(sizeof(double) * parts) : nullptr;
    if (parts)
      hipLaunchKernelGGL(barrier_partial_kernel, dim3((unsigned)parts), dim3(BAR_BLOCK), 0, L.stream, ptEnergy, npt, eeEnergy, nee, partial);
    hipLaunchKernelGGL(barrier_total_kernel, dim3(1), dim3(BAR_BLOCK), 0, L.stream, partial, parts, total);
  }
  if (grad && m->nv)
    hipLaunchKernelGGL(barrier_gather_kernel, dim3(ceil_div(m->nv, BAR_BLOCK)), dim3(BAR_BLOCK), 0, L.stream, starts, entries, scratch, (int)m->nv,
                       grad);
  return 0;
}

int zs_rocm_mesh_barrier_energy(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                                size_t nee, float dHat, float kappa, int mollify, float *ptEnergy, float *eeEnergy, double *total, int *status) {
  return barrier_run(pol, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, nullptr, nullptr, nullptr, ptEnergy, eeEnergy, total, nullptr,
                     status);
}

int zs_rocm_mesh_barrier_gradient(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                                  size_t nee, float dHat, float kappa, int mollify, const int *starts, const int *entries, float *scratch,
                                  float *ptEnergy, float *eeEnergy, double *total, float *grad, int *status) {
  if (!grad && m && m->nv) return -1;
  return barrier_run(pol, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, starts, entries, scratch, ptEnergy, eeEnergy, total, grad,
                     status);
}

int zs_rocm_mesh_barrier_hessian_product(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt,
                                         const int *eePairs, size_t nee, float dHat, float kappa, int mollify, int psd, const float *x,
                                         const int *starts, const int *entries, float *scratch, float *hx, int *status) {
  if (!pol || !m || !m->stats || !(dHat > 0.f && dHat <= FLT_MAX) || !(kappa > 0.f && kappa <= FLT_MAX) || (mollify && !m->hasRest)) return -1;
  if (!barrier_counts_ok(npt, nee) || (npt && !ptPairs) || (nee && !eePairs)) return -1;
  if (m->nv && (!x || !hx || !starts || (npt + nee && (!entries || !scratch)))) return -1;
  Launch L(pol, "mesh_barrier_hessian_product");
  const float *pos = verts ? verts : m->verts;
  const float dHat2 = dHat * dHat;
  int *st = status ? status : (int *)L.temp(sizeof(int) * 2);
  ZSR_CHECK(hipMemsetAsync(st, 0, sizeof(int) * 2, L.stream));
  if (npt) {
    const dim3 grid(ceil_div(npt, BAR_BLOCK)), block(BAR_BLOCK);
    if (psd)
      hipLaunchKernelGGL((barrier_pt_hvp_kernel<true>), grid, block, 0, L.stream, pos, m->tris, (int)m->nv, (int)m->nt, ptPairs, (int)npt, dHat2,
                         kappa, x, scratch, st);
    else
      hipLaunchKernelGGL((barrier_pt_hvp_kernel<false>), grid, block, 0, L.stream, pos, m->tris, (int)m->nv, (int)m->nt, ptPairs, (int)npt, dHat2,
                         kappa, x, scratch, st);
  }
  if (nee) {
    const dim3 grid(ceil_div(nee, BAR_BLOCK)), block(BAR_BLOCK);
    const float *rest = mollify ? m->restLen2 : nullptr;
    if (psd)
      hipLaunchKernelGGL((barrier_ee_hvp_kernel<true>), grid, block, 0, L.stream, pos, m->edges, (int)m->nv, (int)m->ne, rest, eePairs, (int)nee,
                         dHat2, kappa, x, scratch + 12 * npt, st);
    else
      hipLaunchKernelGGL((barrier_ee_hvp_kernel<false>), grid, block, 0, L.stream, pos, m->edges, (int)m->nv, (int)m->ne, rest, eePairs, (int)nee,
                         dHat2, kappa, x, scratch + 12 * npt, st);
  }
  if (m->nv)
    hipLaunchKernelGGL(barrier_gather_kernel, dim3(ceil_div(m->nv, BAR_BLOCK)), dim3(BAR_BLOCK), 0, L.stream, starts, entries, scratch, (int)m->nv,
                       hx);
  return 0;
}

}  // extern "C"
