// mesh_barrier.hip -- the IPC contact potential of a mesh on a proximity constraint set for gfx950: total energy, per-vertex gradient and
// matrix-free Hessian-vector product over the PT and EE pair lists of mesh_proximity.hip, at the mesh's own or at trial positions
// (include/zensim_rocm/barrier_device.hpp has the math).  Bit-reproducible: no float atomics anywhere.
//
//   pairs     lane = pair, one kernel template for both kinds and every operation (energy, gradient, the Hessian-vector product H x and its
//             positive semi-definite H+ x of the header).  barrier_corners resolves the pair's four vertices -- indices outside the mesh make
//             a pair inactive -- then the kernel gathers them (a product: the four rows of the direction as well), recomputes distance,
//             parameters and feature at the given positions and writes the pair's energy and / or its [4][3] contributions to a scratch
//             array, once.  Zero-distance pairs are counted with an integer atomic (a count has no order).  A new per-pair quantity is one
//             more BARRIER_OP_* and its branch in barrier_pair_kernel.
//   friction  four such operations (include/zensim_rocm/friction_device.hpp has the math).  The lag step runs at positions like the barrier
//             and writes one 32-byte record (n, lambda, w) per pair, PT pairs first; friction energy, gradient and product gather the
//             displacement u where the barrier gathers positions, read the record and never touch the distance code.  Their per-pair
//             energies and [4][3] contributions go through the same sum and the same gather.
//   energy, incidence, gather: the shared layer of mesh_terms.hip.  The float64 total runs over the PT then the EE energies; the incidence
//             has the 4 (npt + nee) (vertex, 4 pair + corner) entries, EE pairs numbered behind the PT pairs, built once per pair of lists;
//             the gather sums a vertex's one run of the scratch contributions (of the gradient or of a product) in list order.
// Built with -ffp-contract=off (zpc_amd/build.py), as every translation unit behind tri_closest / ee_closest.
#include <cfloat>

#include "mesh_pairs.hpp"

namespace zsr {

constexpr int BAR_BLOCK = TERM_BLOCK;

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

template <bool EE, int OP>
__global__ __launch_bounds__(BAR_BLOCK) void barrier_pair_kernel(const BarrierPairs a) {
  const int i = blockIdx.x * BAR_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  constexpr bool PRODUCT = OP == BARRIER_OP_PRODUCT || OP == BARRIER_OP_PRODUCT_PSD || OP == BARRIER_OP_FRICTION_PRODUCT;
  constexpr bool FRICTION = OP == BARRIER_OP_FRICTION_ENERGY || OP == BARRIER_OP_FRICTION_GRADIENT || OP == BARRIER_OP_FRICTION_PRODUCT;
  int idx[4];
  float eps, e = 0.f, g[4][3] = {};
  [[maybe_unused]] FrictionRecord rec = friction_record_zero();
  if (barrier_corners<EE>(a, i, idx, eps)) {
    float p[4][3];
    vertex_rows<4>(a.verts, idx, p);
    int status;
    if constexpr (OP == BARRIER_OP_LAG) {
      if constexpr (EE)
        status = friction_lag_ee(p[0], p[1], p[2], p[3], a.dHat2, a.kappa, eps, rec);
      else
        status = friction_lag_pt(p[0], p[1], p[2], p[3], a.dHat2, a.kappa, rec);
    } else if constexpr (FRICTION) {
      rec = friction_load(a.record, (size_t)i);
      if constexpr (OP == BARRIER_OP_FRICTION_PRODUCT) {
        float x[4][3];
        vertex_rows<4>(a.dir, idx, x);
        status = friction_product(rec, p, x, a.mu, a.epsv, g);
      } else if constexpr (OP == BARRIER_OP_FRICTION_GRADIENT) {
        status = friction_gradient(rec, p, a.mu, a.epsv, e, g);
      } else {
        status = friction_energy(rec, p, a.mu, a.epsv, e);
      }
    } else if constexpr (PRODUCT) {
      float x[4][3];
      vertex_rows<4>(a.dir, idx, x);
      if constexpr (EE)
        status = barrier_ee_hvp<OP == BARRIER_OP_PRODUCT_PSD>(p[0], p[1], p[2], p[3], x, a.dHat2, a.kappa, eps, g);
      else
        status = barrier_pt_hvp<OP == BARRIER_OP_PRODUCT_PSD>(p[0], p[1], p[2], p[3], x, a.dHat2, a.kappa, g);
    } else if constexpr (EE) {
      status = barrier_ee<OP == BARRIER_OP_GRADIENT>(p[0], p[1], p[2], p[3], a.dHat2, a.kappa, eps, e, g);
    } else {
      status = barrier_pt<OP == BARRIER_OP_GRADIENT>(p[0], p[1], p[2], p[3], a.dHat2, a.kappa, e, g);
    }
    if (status == BARRIER_ZERO) atomicAdd(a.status + EE, 1);
  }
  if constexpr (OP == BARRIER_OP_LAG) {
    friction_store(a.record, (size_t)i, rec);
  } else {
    if constexpr (!PRODUCT) a.energy[i] = e;
    if constexpr (OP != BARRIER_OP_ENERGY && OP != BARRIER_OP_FRICTION_ENERGY) barrier_store(a.contrib, (size_t)i, g);
  }
}

// ---------------------------------------------------------------------------------------------------------------- incidence
// the vertex of entry c = 4 pair + corner (EE pairs behind the PT pairs); a PT pair's triangle index and an EE pair's edge index are
// checked before they are followed, the corner's own vertex by incidence_emit
struct BarrierCornerVertex {
  const int *tris, *edges;
  int nt, ne;
  const int *ptPairs, *eePairs;
  size_t npt;
  __device__ int operator()(size_t c) const {
    const size_t pair = c >> 2;
    const int k = (int)(c & 3);
    if (pair < npt) {
      const int vi = ptPairs[2 * pair], ti = ptPairs[2 * pair + 1];
      return (unsigned)ti >= (unsigned)nt ? -1 : k == 0 ? vi : tris[3 * (size_t)ti + (k - 1)];
    }
    const int e = eePairs[2 * (pair - npt) + (k >> 1)];
    return (unsigned)e < (unsigned)ne ? edges[2 * (size_t)e + (k & 1)] : -1;
  }
};

// the checks the energy, the gradient and the product have in common
bool barrier_args_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, const int *ptPairs, size_t npt, const int *eePairs, size_t nee, float dHat,
                     float kappa, int mollify) {
  if (!pol || !m || !m->stats || !(dHat > 0.f && dHat <= FLT_MAX) || !(kappa > 0.f && kappa <= FLT_MAX) || (mollify && !m->hasRest)) return false;
  return barrier_counts_ok(npt, nee) && !(npt && !ptPairs) && !(nee && !eePairs);
}

template <int OP>
static void barrier_launch_op(Launch &L, const BarrierPairs &pt, const BarrierPairs &ee) {
  const dim3 block(BAR_BLOCK);
  if (pt.n) hipLaunchKernelGGL((barrier_pair_kernel<false, OP>), dim3(ceil_div(pt.n, BAR_BLOCK)), block, 0, L.stream, pt);
  if (ee.n) hipLaunchKernelGGL((barrier_pair_kernel<true, OP>), dim3(ceil_div(ee.n, BAR_BLOCK)), block, 0, L.stream, ee);
}

// the argument blocks of the PT and the EE list: the EE list's scratch (stride floats per pair) and records follow the PT list's
void barrier_pair_args(const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs, size_t nee, float dHat,
                       float kappa, int mollify, const float *dir, float *ptEnergy, float *eeEnergy, float *scratch, size_t stride, int *status,
                       const FrictionArgs &fr, BarrierPairs &pt, BarrierPairs &ee) {
  pt = {verts ? verts : m->verts, m->tris, (int)m->nv, (int)m->nt, nullptr, ptPairs, (int)npt, dHat * dHat, kappa, dir,
        ptEnergy, scratch, status, fr.record, fr.mu, fr.epsv};
  ee = pt;
  ee.prims = m->edges, ee.np = (int)m->ne, ee.rest = mollify ? m->restLen2 : nullptr;
  ee.pairs = eePairs, ee.n = (int)nee, ee.energy = eeEnergy, ee.contrib = scratch ? scratch + stride * npt : nullptr;
  ee.record = fr.record ? fr.record + 8 * npt : nullptr;
}

void barrier_launch_args(Launch &L, int op, const BarrierPairs &pt, const BarrierPairs &ee) {
  switch (op) {
    case BARRIER_OP_ENERGY: return barrier_launch_op<BARRIER_OP_ENERGY>(L, pt, ee);
    case BARRIER_OP_GRADIENT: return barrier_launch_op<BARRIER_OP_GRADIENT>(L, pt, ee);
    case BARRIER_OP_PRODUCT: return barrier_launch_op<BARRIER_OP_PRODUCT>(L, pt, ee);
    case BARRIER_OP_PRODUCT_PSD: return barrier_launch_op<BARRIER_OP_PRODUCT_PSD>(L, pt, ee);
    case BARRIER_OP_LAG: return barrier_launch_op<BARRIER_OP_LAG>(L, pt, ee);
    case BARRIER_OP_FRICTION_ENERGY: return barrier_launch_op<BARRIER_OP_FRICTION_ENERGY>(L, pt, ee);
    case BARRIER_OP_FRICTION_GRADIENT: return barrier_launch_op<BARRIER_OP_FRICTION_GRADIENT>(L, pt, ee);
    default: return barrier_launch_op<BARRIER_OP_FRICTION_PRODUCT>(L, pt, ee);
  }
}

// the pair kernels of one operation: the PT list, then the EE list; the status words (the caller's or a temporary) are zeroed first
void barrier_launch_pairs(Launch &L, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                          size_t nee, float dHat, float kappa, int mollify, int op, const float *dir, float *ptEnergy, float *eeEnergy,
                          float *scratch, int *status, const FrictionArgs &fr) {
  BarrierPairs pt, ee;
  barrier_pair_args(m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, dir, ptEnergy, eeEnergy, scratch, 12, terms_status(L, status), fr,
                    pt, ee);
  barrier_launch_args(L, op, pt, ee);
}

// the checks the friction evaluations have in common
bool friction_args_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *u, const int *ptPairs, size_t npt, const int *eePairs,
                      size_t nee, const float *record, float mu, float epsv) {
  if (!pol || !m || !m->stats || !(mu >= 0.f && mu <= FLT_MAX) || !(epsv > 0.f && epsv <= FLT_MAX) || (m->nv && !u)) return false;
  return barrier_counts_ok(npt, nee) && !(npt && !ptPairs) && !(nee && !eePairs) && !(npt + nee && !record);
}

// the launch names of the operations, in the order of BARRIER_OP_*
static const char *const BARRIER_OP_NAME[] = {"mesh_barrier_energy", "mesh_barrier_gradient", "mesh_barrier_hessian_product",
                                              "mesh_barrier_hessian_product", "mesh_friction_lag", "mesh_friction_energy",
                                              "mesh_friction_gradient", "mesh_friction_hessian_product"};

// what the barrier and friction entries share behind their argument checks.  verts: the positions, or the displacement of a friction
// evaluation (fr set).  Energy (grad == NULL) or energy and gradient:
static int pairs_evaluate(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                          size_t nee, float dHat, float kappa, int mollify, int op, const FrictionArgs &fr, const int *starts, const int *entries,
                          float *scratch, float *ptEnergy, float *eeEnergy, double *total, float *grad, int *status) {
  if (grad && m->nv && (!starts || (npt + nee && (!entries || !scratch)))) return -1;
  Launch L(pol, BARRIER_OP_NAME[op]);
  if (npt && !ptEnergy) ptEnergy = (float *)L.temp(sizeof(float) * npt);
  if (nee && !eeEnergy) eeEnergy = (float *)L.temp(sizeof(float) * nee);
  barrier_launch_pairs(L, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, op, nullptr, ptEnergy, eeEnergy, grad ? scratch : nullptr,
                       status, fr);
  if (total) terms_total(L, ptEnergy, npt, eeEnergy, nee, total);
  const TermRun run = {starts, entries, scratch};
  if (grad) terms_gather(L, &run, 1, m->nv, grad);
  return 0;
}
// ... and the Hessian-vector product:
static int pairs_product(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                         size_t nee, float dHat, float kappa, int mollify, int op, const FrictionArgs &fr, const float *x, const int *starts,
                         const int *entries, float *scratch, float *hx, int *status) {
  if (m->nv && (!x || !hx || !starts || (npt + nee && (!entries || !scratch)))) return -1;
  Launch L(pol, BARRIER_OP_NAME[op]);
  barrier_launch_pairs(L, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, op, x, nullptr, nullptr, scratch, status, fr);
  const TermRun run = {starts, entries, scratch};
  terms_gather(L, &run, 1, m->nv, hx);
  return 0;
}

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
  incidence_build(L, BarrierCornerVertex{m->tris, m->edges, (int)m->nt, (int)m->ne, ptPairs, eePairs, npt}, n, m->nv, starts, entries);
  return 0;
}

int zs_rocm_mesh_barrier_energy(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                                size_t nee, float dHat, float kappa, int mollify, float *ptEnergy, float *eeEnergy, double *total, int *status) {
  if (!barrier_args_ok(pol, m, ptPairs, npt, eePairs, nee, dHat, kappa, mollify)) return -1;
  return pairs_evaluate(pol, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, BARRIER_OP_ENERGY, {}, nullptr, nullptr, nullptr, ptEnergy,
                        eeEnergy, total, nullptr, status);
}

int zs_rocm_mesh_barrier_gradient(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                                  size_t nee, float dHat, float kappa, int mollify, const int *starts, const int *entries, float *scratch,
                                  float *ptEnergy, float *eeEnergy, double *total, float *grad, int *status) {
  if (!barrier_args_ok(pol, m, ptPairs, npt, eePairs, nee, dHat, kappa, mollify) || (!grad && m->nv)) return -1;
  return pairs_evaluate(pol, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, grad ? BARRIER_OP_GRADIENT : BARRIER_OP_ENERGY, {}, starts,
                        entries, scratch, ptEnergy, eeEnergy, total, grad, status);
}

int zs_rocm_mesh_barrier_hessian_product(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt,
                                         const int *eePairs, size_t nee, float dHat, float kappa, int mollify, int psd, const float *x,
                                         const int *starts, const int *entries, float *scratch, float *hx, int *status) {
  if (!barrier_args_ok(pol, m, ptPairs, npt, eePairs, nee, dHat, kappa, mollify)) return -1;
  return pairs_product(pol, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, psd ? BARRIER_OP_PRODUCT_PSD : BARRIER_OP_PRODUCT, {}, x,
                       starts, entries, scratch, hx, status);
}

int zs_rocm_mesh_friction_lag(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const int *ptPairs, size_t npt, const int *eePairs,
                              size_t nee, float dHat, float kappa, int mollify, float *record, int *status) {
  if (!barrier_args_ok(pol, m, ptPairs, npt, eePairs, nee, dHat, kappa, mollify) || (npt + nee && !record)) return -1;
  Launch L(pol, BARRIER_OP_NAME[BARRIER_OP_LAG]);
  barrier_launch_pairs(L, m, verts, ptPairs, npt, eePairs, nee, dHat, kappa, mollify, BARRIER_OP_LAG, nullptr, nullptr, nullptr, nullptr, status,
                       {record, 0.f, 0.f});
  return 0;
}

int zs_rocm_mesh_friction_energy(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *u, const int *ptPairs, size_t npt, const int *eePairs,
                                 size_t nee, const float *record, float mu, float epsv, float *ptEnergy, float *eeEnergy, double *total,
                                 int *status) {
  if (!friction_args_ok(pol, m, u, ptPairs, npt, eePairs, nee, record, mu, epsv)) return -1;
  return pairs_evaluate(pol, m, u, ptPairs, npt, eePairs, nee, 0.f, 0.f, 0, BARRIER_OP_FRICTION_ENERGY, {const_cast<float *>(record), mu, epsv},
                        nullptr, nullptr, nullptr, ptEnergy, eeEnergy, total, nullptr, status);
}

int zs_rocm_mesh_friction_gradient(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *u, const int *ptPairs, size_t npt, const int *eePairs,
                                   size_t nee, const float *record, float mu, float epsv, const int *starts, const int *entries, float *scratch,
                                   float *ptEnergy, float *eeEnergy, double *total, float *grad, int *status) {
  if (!friction_args_ok(pol, m, u, ptPairs, npt, eePairs, nee, record, mu, epsv) || (!grad && m->nv)) return -1;
  return pairs_evaluate(pol, m, u, ptPairs, npt, eePairs, nee, 0.f, 0.f, 0, grad ? BARRIER_OP_FRICTION_GRADIENT : BARRIER_OP_FRICTION_ENERGY,
                        {const_cast<float *>(record), mu, epsv}, starts, entries, scratch, ptEnergy, eeEnergy, total, grad, status);
}

int zs_rocm_mesh_friction_hessian_product(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *u, const float *x, const int *ptPairs, size_t npt,
                                          const int *eePairs, size_t nee, const float *record, float mu, float epsv, const int *starts,
                                          const int *entries, float *scratch, float *hx, int *status) {
  if (!friction_args_ok(pol, m, u, ptPairs, npt, eePairs, nee, record, mu, epsv)) return -1;
  return pairs_product(pol, m, u, ptPairs, npt, eePairs, nee, 0.f, 0.f, 0, BARRIER_OP_FRICTION_PRODUCT, {const_cast<float *>(record), mu, epsv}, x,
                       starts, entries, scratch, hx, status);
}

}  // extern "C"
