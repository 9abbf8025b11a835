// mesh.hpp -- the triangle-mesh object of the C ABI, shared by mesh.hip (colliders, mesh -> level set), mesh_proximity.hip (the
// point-triangle and edge-edge pairs within a contact distance), mesh_barrier.hip (the contact potential on those pairs), mesh_ccd.hip
// (the largest step along a direction that keeps those pairs apart), mesh_elastic.hip (the membrane and bending energy of the mesh itself)
// mesh_terms.hip (incidence, gather and total behind the barrier, friction and elastic terms) and mesh_solve.hip (the Newton system on those
// terms: diagonal blocks, fused operator, preconditioned CG).
#pragma once
#include "common.hpp"
#include "../../include/zensim_rocm/mesh_device.hpp"

// 32-byte node of the proximity walks: box, level and leaf id / escape index in one aligned fetch (the layout of lbvh.hip's bulk queries)
struct alignas(32) MeshPackedNode {
  float lo[3], hi[3];
  int level, aux;
};

struct zs_rocm_mesh {
  size_t nv = 0, nt = 0, ne = 0;
  bool hasVel = false;
  float *verts = nullptr, *vel = nullptr, *faceN = nullptr, *vertN = nullptr, *edgeN = nullptr, *angles = nullptr, *boxes = nullptr;
  int *tris = nullptr, *heVals = nullptr, *cornerVals = nullptr, *stats = nullptr;
  unsigned long long *heKeys = nullptr;  // sorted half-edge keys (min vertex << 32 | max vertex), heVals = 3 t + edge
  unsigned *cornerKeys = nullptr;        // sorted corner keys (vertex), cornerVals = 3 t + corner
  int *edges = nullptr;                  // [ne][2] unique edges, e[0] < e[1], lexicographic
  zs_rocm_lbvh *bvh = nullptr;
  // proximity queries (mesh_proximity.hip): the edge tree is built by the first edge-edge query and refitted with the mesh from then on;
  // the packed nodes of either tree are refreshed lazily after a build / refit
  float *edgeBoxes = nullptr;
  zs_rocm_lbvh *edgeBvh = nullptr;
  mutable MeshPackedNode *triPacked = nullptr;
  MeshPackedNode *edgePacked = nullptr;
  mutable bool triPackedValid = false;
  bool edgePackedValid = false;
  // the hit candidates of the last count pass (PROX_CACHE per vertex / edge-tree leaf, hit-major) and their counts; valid for the dHat of
  // that pass until the next refit
  mutable int *ptCache = nullptr, *ptCacheCounts = nullptr;
  int *eeCache = nullptr, *eeCacheCounts = nullptr;
  mutable float ptCacheDHat = 0.f;
  float eeCacheDHat = 0.f;
  mutable bool ptCacheValid = false;
  bool eeCacheValid = false;
  // the squared rest length of every unique edge (mesh_barrier.hip: the threshold of the edge-edge mollifier), set by zs_rocm_mesh_set_rest
  float *restLen2 = nullptr;
  bool hasRest = false;
  // the rest shape (mesh_elastic.hip), set by zs_rocm_mesh_set_rest_shape.  Topology only, built by the first call: the hinges [nh][4] (the
  // unique edges with exactly two triangles, in edge order: edge, then the opposite vertices of the smaller and the other triangle), their
  // incidence by vertex (entries 4 hinge + corner, hinge order inside a vertex; hingeStarts [nv + 1]) and the run starts of cornerKeys
  // [nv + 1].  From the rest positions, recomputed by every call: the triangle records [nt][4], the hinge records [nh][4], the vertex areas [nv]
  size_t nh = 0;
  int *hinges = nullptr, *hingeStarts = nullptr, *hingeEntries = nullptr, *cornerStarts = nullptr;
  float *triRecord = nullptr, *hingeRecord = nullptr, *vertArea = nullptr;
  int restShapeCounts[3] = {0, 0, 0};  // degenerate triangles, degenerate hinges, non-manifold edges
  bool hasHinges = false, hasRestShape = false;
  zsr::TriMeshDev dev() const {
    zsr::TriMeshDev d;
    d.verts = verts; d.tris = tris; d.vel = hasVel ? vel : nullptr;
    d.faceNormals = faceN; d.vertNormals = vertN; d.edgeNormals = edgeN;
    zs_rocm_lbvh_view v;
    zs_rocm_lbvh_get_view(bvh, &v);
    d.bvh.orderedBvs = (const zsr::AABB3 *)v.orderedBvs; d.bvh.parents = v.parents; d.bvh.levels = v.levels; d.bvh.leafInds = v.leafInds;
    d.bvh.auxIndices = v.auxIndices; d.bvh.numNodes = v.numNodes;
    d.numVerts = (int)nv; d.numTris = (int)nt;
    return d;
  }
};

namespace zsr {

// primitives.hip
void exclusive_scan_u32(Launch &L, const unsigned *in, size_t n, unsigned *out);
void radix_sort_pair_u32(Launch &L, const unsigned *kin, const int *vin, unsigned *kout, int *vout, size_t n, int sbit, int ebit);

// what the kernels over a proximity list (mesh_barrier.hip, mesh_ccd.hip) share: the four corner vertices of pair i of a list pairs [n][2]
// -- (vertex, triangle) against prims = tris [np][3], or (edge, edge) against prims = edges [np][2] -- false: an index outside the mesh, the
// pair is inactive.  Every load sits behind the check of its index; an edge's own two vertices are not checked (the mesh's own edge list:
// they are inside the mesh)
template <bool EE>
__device__ __forceinline__ bool pair_corners(const int *pairs, const int *prims, int nv, int np, int i, int (&idx)[4]) {
  const int p = pairs[2 * (size_t)i], q = pairs[2 * (size_t)i + 1];
  if constexpr (EE) {
    if (!((unsigned)p < (unsigned)np && (unsigned)q < (unsigned)np)) return false;
    idx[0] = prims[2 * (size_t)p], idx[1] = prims[2 * (size_t)p + 1], idx[2] = prims[2 * (size_t)q], idx[3] = prims[2 * (size_t)q + 1];
    return true;
  } else {
    if (!((unsigned)p < (unsigned)nv && (unsigned)q < (unsigned)np)) return false;
    idx[0] = p, idx[1] = prims[3 * (size_t)q], idx[2] = prims[3 * (size_t)q + 1], idx[3] = prims[3 * (size_t)q + 2];
    return (unsigned)idx[1] < (unsigned)nv && (unsigned)idx[2] < (unsigned)nv && (unsigned)idx[3] < (unsigned)nv;
  }
}

// rows idx of an [nv][3] array
template <int N>
__device__ __forceinline__ void vertex_rows(const float *__restrict__ src, const int (&idx)[N], float (&out)[N][3]) {
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) out[k][d] = src[3 * (size_t)idx[k] + d];
}

// 4 (npt + nee) incidence entries are ints and go through one radix sort call
inline bool barrier_counts_ok(size_t npt, size_t nee) { return npt + nee < ((size_t)1 << 28); }

// the bits a radix sort has to look at for the keys 0 .. count - 1 (at least one)
inline int key_bits(size_t count) {
  int b = 1;
  while (b < 32 && ((size_t)1 << b) < count) ++b;
  return b;
}

// ---- mesh_terms.hip: what barrier, friction and elasticity share behind their per-element kernels, which write one float32 energy per
// element and its [corners][3] terms to a scratch array: the incidence by vertex, the gather in run order, the float64 total
constexpr int TERM_BLOCK = 256;

// the incidence of n entries (entry c = corners * element + corner).  IncidenceKeys: the temporaries of one build, the sort key and number
// of every entry and the per-vertex counts (zeroed by incidence_begin), filled through incidence_emit; incidence_end sorts the entries
// stably by key into entries [n], so a vertex's run is in entry order, and scans the counts into starts [nv + 1]
struct IncidenceKeys {
  unsigned *keys;
  int *vals;
  unsigned *counts;
};
IncidenceKeys incidence_begin(Launch &L, size_t n, size_t nv);
void incidence_end(Launch &L, const IncidenceKeys &k, size_t n, size_t nv, int *starts, int *entries);

// entry c belongs to vertex v; an index outside the mesh gets the key nv: sorted behind every vertex and never read
__device__ __forceinline__ void incidence_emit(const IncidenceKeys &k, size_t c, int v, int nv) {
  const bool ok = (unsigned)v < (unsigned)nv;
  k.keys[c] = ok ? (unsigned)v : (unsigned)nv;
  k.vals[c] = (int)c;
  if (ok) atomicAdd(k.counts + v, 1u);
}
// lane = entry; vertexOf(c) is the vertex of entry c, any value outside [0, nv) where it has none
template <class VertexOf>
__global__ __launch_bounds__(TERM_BLOCK) void incidence_kernel(const VertexOf vertexOf, size_t n, int nv, const IncidenceKeys k) {
  const size_t c = (size_t)blockIdx.x * TERM_BLOCK + threadIdx.x;
  if (c < n) incidence_emit(k, c, vertexOf(c), nv);
}
template <class VertexOf>
void incidence_build(Launch &L, const VertexOf &vertexOf, size_t n, size_t nv, int *starts, int *entries) {
  const IncidenceKeys k = incidence_begin(L, n, nv);
  if (n) hipLaunchKernelGGL(incidence_kernel<VertexOf>, dim3(ceil_div(n, TERM_BLOCK)), dim3(TERM_BLOCK), 0, L.stream, vertexOf, n, (int)nv, k);
  incidence_end(L, k, n, nv, starts, entries);
}

// one run per vertex: entries [starts[v], starts[v + 1]) index rows of terms [..][3]
struct TermRun {
  const int *starts, *entries;
  const float *terms;
};
// the rows of one run of vertex v, front to back (the gathers of mesh_terms.hip and mesh_solve.hip)
__device__ __forceinline__ void terms_add_run(const int *__restrict__ starts, const int *__restrict__ entries, const float *__restrict__ terms, int v,
                                              float &s0, float &s1, float &s2) {
  for (int i = starts[v]; i < starts[v + 1]; ++i) {
    const float *g = terms + 3 * (size_t)entries[i];
    s0 += g[0];
    s1 += g[1];
    s2 += g[2];
  }
}
// out [nv][3]: lane = vertex sums the rows of its nruns (1 or 2) runs, one run after the other, each front to back
void terms_gather(Launch &L, const TermRun *runs, int nruns, size_t nv, float *out);
// the float64 total of the floats a [na] then b [nb], summed in a fixed order
void terms_total(Launch &L, const float *a, size_t na, const float *b, size_t nb, double *total);
// the caller's two status counts or a temporary, zeroed
int *terms_status(Launch &L, int *status);

// ---- mesh_elastic.hip: what mesh_solve.hip launches inside its own Launch
// the N vertex indices of element i of elems [n][N]; false: one is outside the mesh and the element is idle
template <int N>
__device__ __forceinline__ bool elastic_indices(const int *__restrict__ elems, size_t i, int nv, int (&idx)[N]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    idx[k] = elems[N * i + k];
    ok = ok && (unsigned)idx[k] < (unsigned)nv;
  }
  return ok;
}
bool elastic_args_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, float mu, float lam, float kb);
// the element kernels of one operation (ELASTIC_OP_*): triangles, then hinges, whose terms follow the triangles' in scratch; st: two zeroed
// counts
void elastic_launch_status(Launch &L, const zs_rocm_mesh *m, const float *verts, float mu, float lam, float kb, int op, const float *dir,
                           float *triEnergy, float *hingeEnergy, float *scratch, int *st);

// mesh_proximity.hip: after new vertex positions -- the packed nodes are stale, the edge tree (if built) is refitted; -1 on failure
int mesh_proximity_refit(zs_rocm_policy *pol, zs_rocm_mesh &m);

}  // namespace zsr
