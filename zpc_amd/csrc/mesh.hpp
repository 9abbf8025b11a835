// mesh.hpp -- the triangle-mesh object of the C ABI, shared by mesh.hip (colliders, mesh -> level set), mesh_proximity.hip (the
// point-triangle and edge-edge pairs within a contact distance) and mesh_barrier.hip (the contact potential on those pairs).
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

// mesh_proximity.hip: after new vertex positions -- the packed nodes are stale, the edge tree (if built) is refitted; -1 on failure
int mesh_proximity_refit(zs_rocm_policy *pol, zs_rocm_mesh &m);

}  // namespace zsr
