// distance_device.hpp -- tri_closest: squared distance from a point to a triangle with the closest point, its barycentric coordinates and the feature it
// lies on: the counterpart of dist_pt_sqr / pt_category_and_dist2 (geometry/SpatialQuery.hpp:19,146) and of pt_distance_type /
// dist2_pt_unclassified (geometry/Distance.hpp), written from the Voronoi regions of a triangle (Ericson, Real-Time Collision Detection,
// 5.1.5; Eberly, "Distance between point and triangle in 3D"):
//   face region   the projection of p on the plane lies inside all three edge planes:  n . ((v_{i+1} - v_i) x (p - v_i)) >= 0 for every
//                 edge, n = (b - a) x (c - a).  Closest point = projection, barycentrics = the three triple products / |n|^2.
//   otherwise     the closest point lies on the boundary: the nearest of the three edge SEGMENTS.  The clamped parameter of the winning
//                 segment names the feature: t <= 0 / t >= 1 a vertex region, else the edge region.
// A zero-area triangle (|n|^2 <= TRI_DEGENERATE |ab|^2 |ac|^2, i.e. sin of the angle at a below 3.2e-7: the float cross product is rounding
// noise below ~6e-8) skips the face test, so it degrades to the distance to its edges -- their union is its longest edge -- and, with all
// three vertices equal, to the distance to that point (a zero-length edge has t = 0).  No division has a zero denominator: never a NaN
// for finite input.
//
// ee_closest: squared distance between two segments [a0, a1] and [b0, b1] with the parameters of the closest point pair and the feature
// pair it is realised on: the counterpart of dist_ee_sqr / ee_category_and_dist2 (geometry/SpatialQuery.hpp:316-500), same category
// encoding (uCate * 3 + vCate, each 0: first endpoint, 1: second endpoint, 2: interior).  Written from the geometry, not from the
// reference's clamped (a c - b^2) chain, whose absolute eps depends on the scale of the input and whose b e - c d cancels in float32:
//   interior   with u = a1 - a0, v = b1 - b0, w = a0 - b0, n = u x v: the common perpendicular meets the lines at
//              s = ((v x w) . n) / |n|^2, t = ((u x w) . n) / |n|^2.  A candidate only if the edges are not parallel
//              (|n|^2 > EE_PARALLEL |u|^2 |v|^2, the threshold of TRI_DEGENERATE) and 0 < s < 1, 0 < t < 1; its distance is measured
//              between the two points, |w + s u - t v|^2, not as (w . n)^2 / |n|^2.
//   boundary   otherwise the minimum has an endpoint on one side: the four point-segment distances a0, a1 against [b0, b1] and b0, b1
//              against [a0, a1] (segment_dist2).
// The smallest candidate wins, ties to the earlier one in that order.  Every candidate is the distance of two points of the segments, so
// the result is never below the true distance and never NaN for finite input; zero-length and exactly parallel edges have boundary
// candidates only.
// Translation units that use this are built with -ffp-contract=off: a float32 chain in numpy then reproduces every discrete decision.
#pragma once
#include <hip/hip_runtime.h>

namespace zsr {

enum { TRI_VERT_A = 0, TRI_VERT_B = 1, TRI_VERT_C = 2, TRI_EDGE_AB = 3, TRI_EDGE_BC = 4, TRI_EDGE_CA = 5, TRI_FACE = 6 };
constexpr float TRI_DEGENERATE = 1e-13f;

struct TriClosest {
  float dist2;
  float cp[3];    // closest point
  float bary[3];  // cp = bary[0] a + bary[1] b + bary[2] c
  int feature;    // TRI_*
};

// squared distance from p to the segment [u, v]; t = clamped parameter (0 at u)
__host__ __device__ __forceinline__ float segment_dist2(const float (&p)[3], const float (&u)[3], const float (&v)[3], float &t) {
  const float e[3] = {v[0] - u[0], v[1] - u[1], v[2] - u[2]}, d[3] = {p[0] - u[0], p[1] - u[1], p[2] - u[2]};
  const float ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], de = d[0] * e[0] + d[1] * e[1] + d[2] * e[2];
  t = ee > 0.f ? de / ee : 0.f;
  t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
  const float r[3] = {d[0] - t * e[0], d[1] - t * e[1], d[2] - t * e[2]};
  return r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
}

__host__ __device__ __forceinline__ TriClosest tri_closest(const float (&p)[3], const float (&a)[3], const float (&b)[3], const float (&c)[3]) {
  TriClosest r;
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
  const float n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
  const float nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  const float lab = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], lac = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
  if (nn > TRI_DEGENERATE * lab * lac) {
    const float pa[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]}, pb[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    // triple products n . (edge x (p - start)): wc belongs to edge ab (weight of c), wa to bc, wb to ca (= -ac)
    const float xc[3] = {ab[1] * pa[2] - ab[2] * pa[1], ab[2] * pa[0] - ab[0] * pa[2], ab[0] * pa[1] - ab[1] * pa[0]};
    const float xa[3] = {bc[1] * pb[2] - bc[2] * pb[1], bc[2] * pb[0] - bc[0] * pb[2], bc[0] * pb[1] - bc[1] * pb[0]};
    const float xb[3] = {pa[1] * ac[2] - pa[2] * ac[1], pa[2] * ac[0] - pa[0] * ac[2], pa[0] * ac[1] - pa[1] * ac[0]};
    const float wc = n[0] * xc[0] + n[1] * xc[1] + n[2] * xc[2], wa = n[0] * xa[0] + n[1] * xa[1] + n[2] * xa[2];
    const float wb = n[0] * xb[0] + n[1] * xb[1] + n[2] * xb[2];
    if (wa >= 0.f && wb >= 0.f && wc >= 0.f) {
      const float h = n[0] * pa[0] + n[1] * pa[1] + n[2] * pa[2];
      r.dist2 = h * h / nn;
      r.bary[1] = wb / nn;
      r.bary[2] = wc / nn;
      r.bary[0] = 1.f - r.bary[1] - r.bary[2];
#pragma unroll
      for (int d = 0; d < 3; ++d) r.cp[d] = a[d] + (r.bary[1] * ab[d] + r.bary[2] * ac[d]);
      r.feature = TRI_FACE;
      return r;
    }
  }
  float t0, t1, t2;
  const float d0 = segment_dist2(p, a, b, t0), d1 = segment_dist2(p, b, c, t1), d2 = segment_dist2(p, c, a, t2);
  if (d0 <= d1 && d0 <= d2) {
    r.dist2 = d0;
    r.bary[0] = 1.f - t0; r.bary[1] = t0; r.bary[2] = 0.f;
    r.feature = t0 <= 0.f ? TRI_VERT_A : (t0 >= 1.f ? TRI_VERT_B : TRI_EDGE_AB);
#pragma unroll
    for (int d = 0; d < 3; ++d) r.cp[d] = a[d] + t0 * ab[d];
  } else if (d1 <= d2) {
    r.dist2 = d1;
    r.bary[0] = 0.f; r.bary[1] = 1.f - t1; r.bary[2] = t1;
    r.feature = t1 <= 0.f ? TRI_VERT_B : (t1 >= 1.f ? TRI_VERT_C : TRI_EDGE_BC);
#pragma unroll
    for (int d = 0; d < 3; ++d) r.cp[d] = b[d] + t1 * bc[d];
  } else {
    r.dist2 = d2;
    r.bary[0] = t2; r.bary[1] = 0.f; r.bary[2] = 1.f - t2;
    r.feature = t2 <= 0.f ? TRI_VERT_C : (t2 >= 1.f ? TRI_VERT_A : TRI_EDGE_CA);
#pragma unroll
    for (int d = 0; d < 3; ++d) r.cp[d] = c[d] + t2 * (a[d] - c[d]);
  }
  return r;
}

enum { EE_FIRST = 0, EE_SECOND = 1, EE_INTERIOR = 2 };
constexpr float EE_PARALLEL = 1e-13f;

struct EdgeClosest {
  float dist2;
  float s, t;    // closest points a0 + s (a1 - a0), b0 + t (b1 - b0)
  int category;  // uCate * 3 + vCate, EE_*
};

__host__ __device__ __forceinline__ int ee_param_category(float t) { return t <= 0.f ? EE_FIRST : (t >= 1.f ? EE_SECOND : EE_INTERIOR); }

__host__ __device__ __forceinline__ EdgeClosest ee_closest(const float (&a0)[3], const float (&a1)[3], const float (&b0)[3], const float (&b1)[3]) {
  EdgeClosest r;
  const float u[3] = {a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]}, v[3] = {b1[0] - b0[0], b1[1] - b0[1], b1[2] - b0[2]};
  const float w[3] = {a0[0] - b0[0], a0[1] - b0[1], a0[2] - b0[2]};
  const float n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const float nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  const float uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  bool interior = false;
  if (nn > EE_PARALLEL * uu * vv) {
    const float vw[3] = {v[1] * w[2] - v[2] * w[1], v[2] * w[0] - v[0] * w[2], v[0] * w[1] - v[1] * w[0]};
    const float uw[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const float s = (vw[0] * n[0] + vw[1] * n[1] + vw[2] * n[2]) / nn, t = (uw[0] * n[0] + uw[1] * n[1] + uw[2] * n[2]) / nn;
    if (s > 0.f && s < 1.f && t > 0.f && t < 1.f) {
      const float q[3] = {(w[0] + s * u[0]) - t * v[0], (w[1] + s * u[1]) - t * v[1], (w[2] + s * u[2]) - t * v[2]};
      r.dist2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
      r.s = s;
      r.t = t;
      r.category = EE_INTERIOR * 3 + EE_INTERIOR;
      interior = true;
    }
  }
  float p;
  float d = segment_dist2(a0, b0, b1, p);
  if (!interior || d < r.dist2) {
    r.dist2 = d; r.s = 0.f; r.t = p;
    r.category = EE_FIRST * 3 + ee_param_category(p);
  }
  d = segment_dist2(a1, b0, b1, p);
  if (d < r.dist2) {
    r.dist2 = d; r.s = 1.f; r.t = p;
    r.category = EE_SECOND * 3 + ee_param_category(p);
  }
  d = segment_dist2(b0, a0, a1, p);
  if (d < r.dist2) {
    r.dist2 = d; r.s = p; r.t = 0.f;
    r.category = ee_param_category(p) * 3 + EE_FIRST;
  }
  d = segment_dist2(b1, a0, a1, p);
  if (d < r.dist2) {
    r.dist2 = d; r.s = p; r.t = 1.f;
    r.category = ee_param_category(p) * 3 + EE_SECOND;
  }
  return r;
}

}  // namespace zsr
