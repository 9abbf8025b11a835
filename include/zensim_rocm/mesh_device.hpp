// mesh_device.hpp -- device view of a triangle mesh with its LBvh and pseudonormals (zpc_amd/csrc/mesh.hip): the closest point on the mesh
// (LBvhView::find_nearest, container/Bvh.hpp:547-590, with the point-triangle distance of distance_device.hpp as the functor) and the
// signed distance, whose sign is that of (p - closest) . pseudonormal(feature): the face normal on a face, the sum of the adjacent face
// normals on an edge, the angle-weighted sum of the incident face normals at a vertex (Baerentzen & Aanaes, "Signed distance computation
// using the angle weighted pseudonormal", IEEE TVCG 11(3), 2005).
#pragma once
#include "distance_device.hpp"
#include "lbvh_device.hpp"

namespace zsr {

struct MeshClosest {
  float dist;  // cap when no triangle is nearer than cap
  int tri;     // -1 then
  int feature;
  float bary[3], cp[3];
};

struct TriMeshDev {
  const float *verts;        // [numVerts][3]
  const int *tris;           // [numTris][3]
  const float *vel;          // [numVerts][3] or nullptr
  const float *faceNormals;  // [numTris][3] unit (0 for a zero-area triangle)
  const float *vertNormals;  // [numVerts][3] angle-weighted sums (not normalised: only the sign of a dot product is taken)
  const float *edgeNormals;  // [numTris][3][3]: edges ab, bc, ca of each triangle
  LBvhDev bvh;
  int numVerts, numTris;

  __device__ __forceinline__ void triangle(int t, float (&a)[3], float (&b)[3], float (&c)[3]) const {
    const int i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a[d] = verts[3 * i0 + d];
      b[d] = verts[3 * i1 + d];
      c[d] = verts[3 * i2 + d];
    }
  }
  // the result for triangle t as the bulk entries report it
  __device__ __forceinline__ MeshClosest finish(const float (&p)[3], int t, float cap) const {
    MeshClosest m;
    m.dist = cap;
    m.tri = -1;
    m.feature = -1;
#pragma unroll
    for (int d = 0; d < 3; ++d) m.bary[d] = m.cp[d] = 0.f;
    if (t < 0) return m;
    float a[3], b[3], c[3];
    triangle(t, a, b, c);
    const TriClosest r = tri_closest(p, a, b, c);
    m.dist = sqrtf(r.dist2);
    m.tri = t;
    m.feature = r.feature;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      m.bary[d] = r.bary[d];
      m.cp[d] = r.cp[d];
    }
    return m;
  }
  // nearest triangle within cap, -1 if none.  Among the leaves the walk visits equal distances go to the smaller triangle number; a leaf
  // whose box is not nearer than the current best is not visited (find_nearest), so an exact tie may also stay with the first one found
  __device__ __forceinline__ int nearest_triangle(const float (&p)[3], float cap) const {
    float best2 = 3.402823466e+38f;
    int best = -1;
    bvh.find_nearest(
        p,
        [&](int t, float &dist, int &idx) {
          float a[3], b[3], c[3];
          triangle(t, a, b, c);
          const float d2 = tri_closest(p, a, b, c).dist2;
          const float d = sqrtf(d2);
          if (d < cap && (d2 < best2 || (d2 == best2 && t < best))) {
            best2 = d2;
            best = t;
            dist = d;
            idx = t;
          }
        },
        cap);
    return best;
  }
  __device__ __forceinline__ MeshClosest closest_point(const float (&p)[3], float cap = 3.402823466e+38f) const {
    return finish(p, nearest_triangle(p, cap), cap);
  }
  // sign of (p - cp) . pseudonormal of the feature: -1 inside, +1 outside or on the surface
  __device__ __forceinline__ float sign_of(const float (&p)[3], const MeshClosest &m) const {
    const float *n;
    if (m.feature == TRI_FACE) n = faceNormals + 3 * m.tri;
    else if (m.feature >= TRI_EDGE_AB) n = edgeNormals + 9 * m.tri + 3 * (m.feature - TRI_EDGE_AB);
    else n = vertNormals + 3 * tris[3 * m.tri + m.feature];
    const float s = (p[0] - m.cp[0]) * n[0] + (p[1] - m.cp[1]) * n[1] + (p[2] - m.cp[2]) * n[2];
    return s < 0.f ? -1.f : 1.f;
  }
  // vertex velocities interpolated at the closest point (zero without velocities)
  __device__ __forceinline__ void velocity_of(const MeshClosest &m, float (&v)[3]) const {
    v[0] = v[1] = v[2] = 0.f;
    if (!vel || m.tri < 0) return;
    const int i0 = tris[3 * m.tri], i1 = tris[3 * m.tri + 1], i2 = tris[3 * m.tri + 2];
#pragma unroll
    for (int d = 0; d < 3; ++d) v[d] = m.bary[0] * vel[3 * i0 + d] + m.bary[1] * vel[3 * i1 + d] + m.bary[2] * vel[3 * i2 + d];
  }
  // signed distance within cap (+cap when no triangle is nearer); m: the closest point it was taken at
  __device__ __forceinline__ float signed_distance(const float (&p)[3], float cap, MeshClosest &m) const {
    m = closest_point(p, cap);
    return m.tri < 0 ? cap : sign_of(p, m) * m.dist;
  }
  __device__ __forceinline__ float signed_distance(const float (&p)[3], float cap = 3.402823466e+38f) const {
    MeshClosest m;
    return signed_distance(p, cap, m);
  }
};

}  // namespace zsr
