// mesh.hpp -- the triangle-mesh object of the C ABI, shared by mesh.hip (colliders, mesh -> level set), mesh_proximity.hip (the
// point-triangle and edge-edge pairs within a contact distance), mesh_barrier.hip (the contact potential on those pairs) and mesh_ccd.hip
// (the largest step along a direction that keeps those pairs apart) and mesh_elastic.hip (the membrane and bending energy of the mesh itself).
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
__device__ __forceinline__ void pair_rows(const float *__restrict__ src, const int (&idx)[4], float (&out)[4][3]) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) out[k][d] = src[3 * (size_t)idx[k] + d];
}

// 4 (npt + nee) incidence entries are ints and go through one radix sort call
inline bool barrier_counts_ok(size_t npt, size_t nee) { return npt + nee < ((size_t)1 << 28); }

// mesh_barrier.hip: the float64 total of the floats a [na] then b [nb], summed in a fixed order (its two reduction kernels)
void barrier_launch_total(Launch &L, const float *a, size_t na, const float *b, size_t nb, double *total);

// mesh_proximity.hip: after new vertex positions -- the packed nodes are stale, the edge tree (if built) is refitted; -1 on failure
int mesh_proximity_refit(zs_rocm_policy *pol, zs_rocm_mesh &m);

}  // namespace zsr
