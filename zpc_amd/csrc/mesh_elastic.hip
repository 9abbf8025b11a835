// mesh_elastic.hip -- the internal energy of a mesh for gfx950: StVK membrane energy over the triangles and quadratic bending energy over the
// hinges (include/zensim_rocm/elastic_device.hpp has the math), as total energy, per-vertex gradient and matrix-free Hessian-vector product
// at the mesh's own or at trial positions, against a rest shape kept in the mesh object.  Bit-reproducible: no float atomics anywhere.
//
//   rest      zs_rocm_mesh_set_rest_shape.  Topology, once: a run of exactly two equal keys in the mesh's sorted half-edge keys is a hinge
//             (flags -> scan -> compact, so hinges are in unique-edge order; the run is in triangle order, the sort being stable); longer
//             runs are counted as non-manifold.  The hinge incidence is the shared one of mesh_terms.hip over the 4 nh (vertex,
//             4 hinge + corner) entries.  The triangle incidence is the
//             mesh's own cornerKeys / cornerVals; only its run starts are added (a binary search per vertex).  Positions, every call: the
//             triangle and hinge records, degenerate ones zeroed and counted, and the vertex areas (lane = vertex, a third of each
//             incident rest area, summed in corner order).
//   elements  lane = element, one kernel template for triangles and hinges and every operation, selected by if constexpr as in
//             barrier_pair_kernel.  Every vertex index is checked before its load (an index outside the mesh: the element is idle).  The
//             kernel writes the element's energy and / or its [3][3] or [4][3] terms to a scratch array once, hinges behind the triangles.
//             Elements whose result leaves the float range are counted with an integer atomic and contribute exactly zero.
//   energy    the float64 fixed-order sum of the float32 element energies, triangles then hinges (terms_total of mesh_terms.hip).
//   gather    terms_gather over two runs per vertex: the scratch terms of its triangle run front to back, then those of its hinge run.
// mu = lam = 0 skips the membrane launch and kb = 0 the bending launch: their energies and terms are zero bytes.
// Built with -ffp-contract=off (zpc_amd/build.py): tests/ref64_elastic.py replays the float32 chain operation by operation.
#include <cfloat>

#include "mesh.hpp"
#include "../../include/zensim_rocm/elastic_device.hpp"

namespace zsr {

constexpr int EL_BLOCK = TERM_BLOCK;

// ---------------------------------------------------------------------------------------------------------------- the rest pass
// flags[i] = 1 where sorted half-edge i starts a run of exactly two keys of a proper edge; runs of more than two are counted
__global__ __launch_bounds__(EL_BLOCK) void elastic_hinge_flags_kernel(const unsigned long long *__restrict__ keys, size_t n3, unsigned *flags,
                                                                       int *nonManifold) {
  const size_t i = (size_t)blockIdx.x * EL_BLOCK + threadIdx.x;
  if (i > n3) return;
  unsigned f = 0;
  if (i < n3) {
    const unsigned long long k = keys[i];
    if ((i == 0 || keys[i - 1] != k) && (unsigned)(k >> 32) != (unsigned)k) {
      size_t e = i + 1;
      while (e < n3 && keys[e] == k) ++e;
      if (e - i == 2) f = 1u;
      else if (e - i > 2) atomicAdd(nonManifold, 1);
    }
  }
  flags[i] = f;  // (flags[n3] = 0: the scan's last entry is the number of hinges)
}
__global__ __launch_bounds__(EL_BLOCK) void elastic_hinge_compact_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ vals,
                                                                         size_t n3, const unsigned *__restrict__ flags,
                                                                         const unsigned *__restrict__ offsets, const int *__restrict__ tris,
                                                                         int *hinges) {
  const size_t i = (size_t)blockIdx.x * EL_BLOCK + threadIdx.x;
  if (i >= n3 || !flags[i]) return;
  const unsigned long long k = keys[i];
  const int h0 = vals[i], h1 = vals[i + 1];  // 3 t + edge, the smaller triangle first; the opposite corner is edge + 2
  int *o = hinges + 4 * (size_t)offsets[i];
  o[0] = (int)(unsigned)(k >> 32);
  o[1] = (int)(unsigned)k;
  o[2] = tris[h0 / 3 * 3 + (h0 % 3 + 2) % 3];
  o[3] = tris[h1 / 3 * 3 + (h1 % 3 + 2) % 3];
}
// the vertex of incidence entry c = 4 hinge + corner
struct HingeCornerVertex {
  const int *hinges;
  __device__ int operator()(size_t c) const { return hinges[c]; }
};
// starts[v] = the first sorted corner whose key is not below v, v = 0 .. nv
__global__ __launch_bounds__(EL_BLOCK) void elastic_corner_starts_kernel(const unsigned *__restrict__ keys, size_t n3, int nv, int *starts) {
  const int v = blockIdx.x * EL_BLOCK + threadIdx.x;
  if (v > nv) return;
  size_t lo = 0, hi = n3;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (keys[mid] < (unsigned)v) lo = mid + 1;
    else hi = mid;
  }
  starts[v] = (int)lo;
}

// the rest record of element i (16-byte records in a 256-byte aligned array); degenerate ones are counted
template <bool HINGE>
__global__ __launch_bounds__(EL_BLOCK) void elastic_rest_kernel(const float *__restrict__ verts, const int *__restrict__ elems, int nv, int n,
                                                                float *record, int *degenerate) {
  const int i = blockIdx.x * EL_BLOCK + threadIdx.x;
  if (i >= n) return;
  constexpr int N = HINGE ? 4 : 3;
  int idx[N];
  float rec[4] = {0.f, 0.f, 0.f, 0.f};
  int status = ELASTIC_DEGENERATE;
  if (elastic_indices<N>(elems, (size_t)i, nv, idx)) {
    float X[N][3];
    vertex_rows<N>(verts, idx, X);
    if constexpr (HINGE)
      status = elastic_hinge_rest(X[0], X[1], X[2], X[3], rec);
    else
      status = elastic_tri_rest(X[0], X[1], X[2], rec);
  }
  if (status == ELASTIC_DEGENERATE) atomicAdd(degenerate, 1);
  reinterpret_cast<float4 *>(record)[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

// a third of the rest area of every incident triangle, summed in corner order
__global__ __launch_bounds__(EL_BLOCK) void elastic_vertex_area_kernel(const int *__restrict__ starts, const int *__restrict__ cornerVals,
                                                                       const float *__restrict__ triRecord, int nv, float *area) {
  const int v = blockIdx.x * EL_BLOCK + threadIdx.x;
  if (v >= nv) return;
  float s = 0.f;
  for (int i = starts[v]; i < starts[v + 1]; ++i) s += triRecord[4 * (size_t)(cornerVals[i] / 3) + 3] / 3.f;
  area[v] = s;
}

// ---------------------------------------------------------------------------------------------------------------- elements
// one kind of element and what the element kernel reads and writes for it
struct ElasticElems {
  const float *verts;   // [nv][3] positions
  const int *elems;     // tris [n][3] or hinges [n][4]
  int nv, n;
  const float *record;  // [n][4]
  float mu, lam, kb;
  const float *dir;       // [nv][3], a product only
  float *energy, *terms;  // [n] (energy, gradient) and the [n][3][3] or [n][4][3] terms (all but energy)
  int *status;            // [2] overflow counts, triangles then hinges
};

template <bool HINGE, int OP>
__global__ __launch_bounds__(EL_BLOCK) void elastic_elem_kernel(const ElasticElems a) {
  const int i = blockIdx.x * EL_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  constexpr int N = HINGE ? 4 : 3;
  constexpr bool PRODUCT = OP == ELASTIC_OP_PRODUCT || OP == ELASTIC_OP_PRODUCT_PSD;
  int idx[N];
  float e = 0.f, t[N][3] = {};
  if (elastic_indices<N>(a.elems, (size_t)i, a.nv, idx)) {
    const float4 r = reinterpret_cast<const float4 *>(a.record)[i];
    const float rec[4] = {r.x, r.y, r.z, r.w};
    float x[N][3];
    int status;
    if constexpr (HINGE) {
      if constexpr (PRODUCT) {  // H does not depend on the positions
        vertex_rows<N>(a.dir, idx, x);
        status = elastic_hinge_product(rec, x, a.kb, t);
      } else {
        vertex_rows<N>(a.verts, idx, x);
        if constexpr (OP == ELASTIC_OP_GRADIENT)
          status = elastic_hinge_gradient(rec, x, a.kb, e, t);
        else
          status = elastic_hinge_energy(rec, x, a.kb, e);
      }
    } else {
      vertex_rows<N>(a.verts, idx, x);
      if constexpr (PRODUCT) {
        float z[N][3];
        vertex_rows<N>(a.dir, idx, z);
        status = elastic_tri_product<OP == ELASTIC_OP_PRODUCT_PSD>(rec, x, z, a.mu, a.lam, t);
      } else if constexpr (OP == ELASTIC_OP_GRADIENT) {
        status = elastic_tri_gradient(rec, x, a.mu, a.lam, e, t);
      } else {
        status = elastic_tri_energy(rec, x, a.mu, a.lam, e);
      }
    }
    if (status == ELASTIC_OVERFLOW) atomicAdd(a.status + HINGE, 1);
  }
  if constexpr (!PRODUCT) a.energy[i] = e;
  if constexpr (OP != ELASTIC_OP_ENERGY) {
    float *o = a.terms + 3 * N * (size_t)i;
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
      for (int d = 0; d < 3; ++d) o[3 * k + d] = t[k][d];
  }
}

template <int OP>
static void elastic_launch_op(Launch &L, const ElasticElems &tri, bool membrane, const ElasticElems &hinge, bool bending) {
  const dim3 block(EL_BLOCK);
  constexpr int HINGE_OP = OP == ELASTIC_OP_PRODUCT_PSD ? ELASTIC_OP_PRODUCT : OP;  // bending is positive semi-definite as it stands
  if (tri.n && membrane) hipLaunchKernelGGL((elastic_elem_kernel<false, OP>), dim3(ceil_div(tri.n, EL_BLOCK)), block, 0, L.stream, tri);
  if (hinge.n && bending) hipLaunchKernelGGL((elastic_elem_kernel<true, HINGE_OP>), dim3(ceil_div(hinge.n, EL_BLOCK)), block, 0, L.stream, hinge);
}

bool elastic_args_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, float mu, float lam, float kb) {
  return pol && m && m->stats && m->hasRestShape && mu >= 0.f && mu <= FLT_MAX && lam >= 0.f && lam <= FLT_MAX && kb >= 0.f && kb <= FLT_MAX;
}

// the element kernels of one operation: triangles, then hinges, whose terms follow the triangles'; a kind that is skipped (zero stiffness)
// gets zero bytes; st: two zeroed counts
void elastic_launch_status(Launch &L, const zs_rocm_mesh *m, const float *verts, float mu, float lam, float kb, int op, const float *dir,
                           float *triEnergy, float *hingeEnergy, float *scratch, int *st) {
  const bool membrane = mu > 0.f || lam > 0.f, bending = kb > 0.f;
  const ElasticElems tri = {verts ? verts : m->verts, m->tris, (int)m->nv, (int)m->nt, m->triRecord, mu, lam, kb, dir, triEnergy, scratch, st};
  ElasticElems hinge = tri;
  hinge.elems = m->hinges, hinge.n = (int)m->nh, hinge.record = m->hingeRecord, hinge.energy = hingeEnergy;
  hinge.terms = scratch ? scratch + 9 * m->nt : nullptr;
  if (!membrane && m->nt) {
    if (triEnergy) ZSR_CHECK(hipMemsetAsync(triEnergy, 0, sizeof(float) * m->nt, L.stream));
    if (scratch) ZSR_CHECK(hipMemsetAsync(scratch, 0, sizeof(float) * 9 * m->nt, L.stream));
  }
  if (!bending && m->nh) {
    if (hingeEnergy) ZSR_CHECK(hipMemsetAsync(hingeEnergy, 0, sizeof(float) * m->nh, L.stream));
    if (scratch) ZSR_CHECK(hipMemsetAsync(scratch + 9 * m->nt, 0, sizeof(float) * 12 * m->nh, L.stream));
  }
  switch (op) {
    case ELASTIC_OP_ENERGY: return elastic_launch_op<ELASTIC_OP_ENERGY>(L, tri, membrane, hinge, bending);
    case ELASTIC_OP_GRADIENT: return elastic_launch_op<ELASTIC_OP_GRADIENT>(L, tri, membrane, hinge, bending);
    case ELASTIC_OP_PRODUCT: return elastic_launch_op<ELASTIC_OP_PRODUCT>(L, tri, membrane, hinge, bending);
    default: return elastic_launch_op<ELASTIC_OP_PRODUCT_PSD>(L, tri, membrane, hinge, bending);
  }
}

// ... with the status words (the caller's or a temporary) zeroed first
static void elastic_launch(Launch &L, const zs_rocm_mesh *m, const float *verts, float mu, float lam, float kb, int op, const float *dir,
                           float *triEnergy, float *hingeEnergy, float *scratch, int *status) {
  elastic_launch_status(L, m, verts, mu, lam, kb, op, dir, triEnergy, hingeEnergy, scratch, terms_status(L, status));
}

// per vertex the terms of its triangle run (entries 3 t + corner), then of its hinge run (4 h + corner, behind the triangles' terms)
static void elastic_launch_gather(Launch &L, const zs_rocm_mesh *m, const float *scratch, float *out) {
  const TermRun runs[2] = {{m->cornerStarts, m->cornerVals, scratch}, {m->hingeStarts, m->hingeEntries, scratch + 9 * m->nt}};
  terms_gather(L, runs, 2, m->nv, out);
}

// the hinges, their incidence and the run starts of the corner incidence: the first call only
static void elastic_topology(Launch &L, zs_rocm_mesh &m) {
  const size_t n3 = 3 * m.nt, nv = m.nv;
  unsigned *flags = nullptr, *offsets = nullptr, nh = 0;
  if (n3) {
    int *nonManifold = (int *)L.temp(sizeof(int));
    ZSR_CHECK(hipMemsetAsync(nonManifold, 0, sizeof(int), L.stream));
    flags = (unsigned *)L.temp(sizeof(unsigned) * (n3 + 1)), offsets = (unsigned *)L.temp(sizeof(unsigned) * (n3 + 1));
    hipLaunchKernelGGL(elastic_hinge_flags_kernel, dim3(ceil_div(n3 + 1, EL_BLOCK)), dim3(EL_BLOCK), 0, L.stream, m.heKeys, n3, flags, nonManifold);
    exclusive_scan_u32(L, flags, n3 + 1, offsets);
    ZSR_CHECK(hipMemcpyAsync(&nh, offsets + n3, sizeof(unsigned), hipMemcpyDeviceToHost, L.stream));
    ZSR_CHECK(hipMemcpyAsync(&m.restShapeCounts[2], nonManifold, sizeof(int), hipMemcpyDeviceToHost, L.stream));
    ZSR_CHECK(hipStreamSynchronize(L.stream));
  }
  m.nh = nh;
  const size_t nh1 = nh ? nh : 1;
  ZSR_CHECK(hipMalloc((void **)&m.hinges, sizeof(int) * 4 * nh1));
  ZSR_CHECK(hipMalloc((void **)&m.hingeRecord, sizeof(float) * 4 * nh1));
  ZSR_CHECK(hipMalloc((void **)&m.hingeEntries, sizeof(int) * 4 * nh1));
  ZSR_CHECK(hipMalloc((void **)&m.hingeStarts, sizeof(int) * (nv + 1)));
  ZSR_CHECK(hipMalloc((void **)&m.cornerStarts, sizeof(int) * (nv + 1)));
  ZSR_CHECK(hipMalloc((void **)&m.triRecord, sizeof(float) * 4 * (m.nt ? m.nt : 1)));
  ZSR_CHECK(hipMalloc((void **)&m.vertArea, sizeof(float) * (nv ? nv : 1)));
  if (nh) hipLaunchKernelGGL(elastic_hinge_compact_kernel, dim3(ceil_div(n3, EL_BLOCK)), dim3(EL_BLOCK), 0, L.stream, m.heKeys, m.heVals, n3, flags, offsets, m.tris, m.hinges);
  incidence_build(L, HingeCornerVertex{m.hinges}, 4 * (size_t)nh, nv, m.hingeStarts, m.hingeEntries);
  hipLaunchKernelGGL(elastic_corner_starts_kernel, dim3(ceil_div(nv + 1, EL_BLOCK)), dim3(EL_BLOCK), 0, L.stream, m.cornerKeys, n3, (int)nv, m.cornerStarts);
  m.hasHinges = true;
}

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_mesh_set_rest_shape(zs_rocm_policy *pol, zs_rocm_mesh *m, const float *verts) {
  if (!pol || !m || !m->stats || m->nt >= ((size_t)1 << 28)) return -1;
  Launch L(pol, "mesh_set_rest_shape");
  if (!m->hasHinges) elastic_topology(L, *m);
  const float *X = verts ? verts : m->verts;
  int *degenerate = (int *)L.temp(sizeof(int) * 2);
  ZSR_CHECK(hipMemsetAsync(degenerate, 0, sizeof(int) * 2, L.stream));
  if (m->nt)
    hipLaunchKernelGGL((elastic_rest_kernel<false>), dim3(ceil_div(m->nt, EL_BLOCK)), dim3(EL_BLOCK), 0, L.stream, X, m->tris, (int)m->nv, (int)m->nt,
                       m->triRecord, degenerate);
  if (m->nh)
    hipLaunchKernelGGL((elastic_rest_kernel<true>), dim3(ceil_div(m->nh, EL_BLOCK)), dim3(EL_BLOCK), 0, L.stream, X, m->hinges, (int)m->nv, (int)m->nh,
                       m->hingeRecord, degenerate + 1);
  if (m->nv)
    hipLaunchKernelGGL(elastic_vertex_area_kernel, dim3(ceil_div(m->nv, EL_BLOCK)), dim3(EL_BLOCK), 0, L.stream, m->cornerStarts, m->cornerVals,
                       m->triRecord, (int)m->nv, m->vertArea);
  ZSR_CHECK(hipMemcpyAsync(m->restShapeCounts, degenerate, sizeof(int) * 2, hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
  m->hasRestShape = true;
  return 0;
}

int zs_rocm_mesh_rest_shape_sizes(const zs_rocm_mesh *m, size_t *sizes) {
  if (!m || !sizes || !m->hasRestShape) return -1;
  sizes[0] = m->nt;
  sizes[1] = m->nh;
  sizes[2] = m->nv;
  sizes[3] = 9 * m->nt + 12 * m->nh;
  for (int k = 0; k < 3; ++k) sizes[4 + k] = (size_t)m->restShapeCounts[k];
  return 0;
}

int zs_rocm_mesh_rest_shape(zs_rocm_policy *pol, const zs_rocm_mesh *m, float *triRecord, int *hinges, float *hingeRecord, float *vertexArea) {
  if (!pol || !m || !m->hasRestShape) return -1;
  Launch L(pol, "mesh_rest_shape");
  if (triRecord && m->nt) ZSR_CHECK(hipMemcpyAsync(triRecord, m->triRecord, sizeof(float) * 4 * m->nt, hipMemcpyDeviceToDevice, L.stream));
  if (hinges && m->nh) ZSR_CHECK(hipMemcpyAsync(hinges, m->hinges, sizeof(int) * 4 * m->nh, hipMemcpyDeviceToDevice, L.stream));
  if (hingeRecord && m->nh) ZSR_CHECK(hipMemcpyAsync(hingeRecord, m->hingeRecord, sizeof(float) * 4 * m->nh, hipMemcpyDeviceToDevice, L.stream));
  if (vertexArea && m->nv) ZSR_CHECK(hipMemcpyAsync(vertexArea, m->vertArea, sizeof(float) * m->nv, hipMemcpyDeviceToDevice, L.stream));
  return 0;
}

// the shared entry: grad == NULL is energy only
static int elastic_run(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, float mu, float lam, float kb, float *scratch, float *triEnergy,
                       float *hingeEnergy, double *total, float *grad, int *status) {
  if (!elastic_args_ok(pol, m, mu, lam, kb)) return -1;
  if (grad && m->nt + m->nh && !scratch) return -1;
  Launch L(pol, grad ? "mesh_elastic_gradient" : "mesh_elastic_energy");
  if (m->nt && !triEnergy) triEnergy = (float *)L.temp(sizeof(float) * m->nt);
  if (m->nh && !hingeEnergy) hingeEnergy = (float *)L.temp(sizeof(float) * m->nh);
  elastic_launch(L, m, verts, mu, lam, kb, grad ? ELASTIC_OP_GRADIENT : ELASTIC_OP_ENERGY, nullptr, triEnergy, hingeEnergy, grad ? scratch : nullptr,
                 status);
  if (total) terms_total(L, triEnergy, m->nt, hingeEnergy, m->nh, total);
  if (grad) elastic_launch_gather(L, m, scratch, grad);
  return 0;
}

int zs_rocm_mesh_elastic_energy(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, float mu, float lam, float kb, float *triEnergy,
                                float *hingeEnergy, double *total, int *status) {
  return elastic_run(pol, m, verts, mu, lam, kb, nullptr, triEnergy, hingeEnergy, total, nullptr, status);
}

int zs_rocm_mesh_elastic_gradient(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, float mu, float lam, float kb, float *scratch,
                                  float *triEnergy, float *hingeEnergy, double *total, float *grad, int *status) {
  if (!grad && m && m->nv) return -1;
  return elastic_run(pol, m, verts, mu, lam, kb, scratch, triEnergy, hingeEnergy, total, grad, status);
}

int zs_rocm_mesh_elastic_hessian_product(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, float mu, float lam, float kb, int psd,
                                         const float *x, float *scratch, float *hx, int *status) {
  if (!elastic_args_ok(pol, m, mu, lam, kb)) return -1;
  if (m->nv && (!x || !hx || (m->nt + m->nh && !scratch))) return -1;
  Launch L(pol, "mesh_elastic_hessian_product");
  elastic_launch(L, m, verts, mu, lam, kb, psd ? ELASTIC_OP_PRODUCT_PSD : ELASTIC_OP_PRODUCT, x, nullptr, nullptr, scratch, status);
  elastic_launch_gather(L, m, scratch, hx);
  return 0;
}

}  // extern "C"
