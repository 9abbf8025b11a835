// levelset_device.hpp -- device side of zs::LevelSetBoundary<SparseGrid<3, f32, 8>> (the first member of GeneralBoundary,
// geometry/Collider.h:246-252) and of zs::Collider over it: a signed-distance field "sdf" (1 channel) and optionally a material velocity
// "v" (3 channels) on a sparse grid of 8^3 blocks -- a bht<int, 3, int, 16> keyed by block origins next to a TileVector<f32, 512> -- with
// the three level-set calls of geometry/SparseGrid.hpp:520-545:
//   getSignedDistance(x)   = linear-kernel sample of "sdf" over the 2^3 cells around worldToIndex(x); a cell of an absent block counts as
//                            the background value
//   getNormal(x)           = central differences of getSignedDistance at x +- eps e_i, eps = voxelSize / 4, then normalised (six samples)
//   getMaterialVelocity(x) = the same sample of the three "v" channels (background for absent cells, like every channel), 0 without "v"
// Plain struct = zs_rocm_levelset of the C ABI.  Cell values come through a FETCH functor `float f(chn, ix, iy, iz)`, so the per-point
// entry (one hash query per block change), the staged block kernels (zpc_amd/csrc/levelset.hip: values from LDS) and the C++ face form
// the same sums in the same order and give the same bits.  The normal is a float finite difference: compile translation units that use
// this header with -ffp-contract=off, like collider_device.hpp.
// Below the single level set: TransitionLevelSetView, the blend of two of them at a phase between two keyframes, and its collider.
#pragma once
#include <hip/hip_runtime.h>

#include "../zs_rocm.h"
#include "bht_device.hpp"
#include "collider_device.hpp"

namespace zsr {

constexpr int LS_SIDE = 8, LS_BLOCK = LS_SIDE * LS_SIDE * LS_SIDE;  // SparseGrid<3, f32, 8>: TileVector<f32, 512>

struct LevelSetView : zs_rocm_levelset {
  __host__ __device__ LevelSetView() = default;
  __host__ __device__ LevelSetView(const zs_rocm_levelset &l) : zs_rocm_levelset(l) {}

  __host__ __device__ __forceinline__ BhtDev table_dev() const {
    BhtDev t;
    t.keys = (int *)table.keys; t.indices = table.indices; t.status = table.status; t.activeKeys = (int *)table.activeKeys;
    t.cnt = table.cnt; t.success = table.success;
    t.tableSize = table.tableSize; t.numBuckets = table.numBuckets; t.bucket = (unsigned)BHT_BUCKET;
    t.hf[0] = table.hf0x; t.hf[1] = table.hf0y; t.hf[2] = table.hf1x; t.hf[3] = table.hf1y; t.hf[4] = table.hf2x; t.hf[5] = table.hf2y;
    return t;
  }
  // block number of the block with origin `org` (multiples of 8), -1 when absent; numbers the tiles do not hold count as absent
  __device__ __forceinline__ int block_of(const BhtDev &t, const int (&org)[3]) const {
    const int bno = bht_query<3>(t, org);
    return (bno >= 0 && (size_t)bno < numBlocks) ? bno : -1;
  }
  __device__ __forceinline__ float cell_value(int chn, int bno, int ix, int iy, int iz) const {
    if (bno < 0) return background;
    return tiles[((size_t)bno * numChannels + chn) * LS_BLOCK + (((ix & 7) * LS_SIDE + (iy & 7)) * LS_SIDE + (iz & 7))];
  }
  __host__ __device__ __forceinline__ void worldToIndex(const float (&x)[3], float (&X)[3]) const {
#pragma unroll
    for (int d = 0; d < 3; ++d) X[d] = (x[d] - origin[d]) / h;
  }

  // linear kernel at index-space X: base = floor(X), weights (1 - t, t) per axis, the 2^3 products (w0 w1) w2 times the cell value added
  // in the order first axis slowest (GridArena::isample).  N channels share one set of weights (iPack).  Eight equal values give that
  // value itself (the weights are a partition of unity; their rounded sum is not): a point whose stencil lies wholly outside the
  // stored blocks gets the background bit for bit, on every path, since the rule looks at the values only.
  template <int N, class Fetch> __device__ __forceinline__ void isample(const Fetch &f, int chn, const float (&X)[3], float (&out)[N]) const {
    int base[3];
    float w[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float fl = floorf(X[d]), t = X[d] - fl;
      base[d] = (int)fl;
      w[d][0] = 1.f - t;
      w[d][1] = t;
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
      float val[8];
      bool same = true;
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        val[o] = f(chn + c, base[0] + (o >> 2), base[1] + ((o >> 1) & 1), base[2] + (o & 1));
        same = same && val[o] == val[0];
      }
      float sum = 0.f;
#pragma unroll
      for (int o = 0; o < 8; ++o) sum += ((w[0][o >> 2] * w[1][(o >> 1) & 1]) * w[2][o & 1]) * val[o];
      out[c] = same ? val[0] : sum;
    }
  }
  template <class Fetch> __device__ __forceinline__ float getSignedDistance(const Fetch &f, const float (&x)[3]) const {
    float X[3], r[1];
    worldToIndex(x, X);
    isample<1>(f, sdfChannel, X, r);
    return r[0];
  }
  template <class Fetch> __device__ __forceinline__ void getNormal(const Fetch &f, const float (&x)[3], float (&n)[3]) const {
    const float eps = h / 4;
    float diff[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float v1[3] = {x[0], x[1], x[2]}, v2[3] = {x[0], x[1], x[2]};
      v1[i] = x[i] + eps;
      v2[i] = x[i] - eps;
      diff[i] = (getSignedDistance(f, v1) - getSignedDistance(f, v2)) / (eps + eps);
    }
    const float l = sqrtf(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]);
    n[0] = diff[0] / l; n[1] = diff[1] / l; n[2] = diff[2] / l;
  }
  // false (and vm = 0) when the grid has no "v"
  template <class Fetch> __device__ __forceinline__ bool getMaterialVelocity(const Fetch &f, const float (&x)[3], float (&vm)[3]) const {
    if (velChannel < 0) {
      vm[0] = vm[1] = vm[2] = 0.f;
      return false;
    }
    float X[3];
    worldToIndex(x, X);
    isample<3>(f, velChannel, X, vm);
    return true;
  }
};

// cell values straight from the grid: one hash query whenever the block changes (the 2^3 cells of a sample mostly share one)
struct LevelSetDirectFetch {
  const LevelSetView &ls;
  BhtDev t;
  mutable int org[3], bno;
  mutable bool have;
  __device__ __forceinline__ explicit LevelSetDirectFetch(const LevelSetView &l) : ls(l), t(l.table_dev()), bno(-1), have(false) {}
  __device__ __forceinline__ float operator()(int chn, int ix, int iy, int iz) const {
    const int o[3] = {ix & ~7, iy & ~7, iz & ~7};
    if (!have || o[0] != org[0] || o[1] != org[1] || o[2] != org[2]) {
      org[0] = o[0]; org[1] = o[1]; org[2] = o[2];
      bno = ls.block_of(t, o);
      have = true;
    }
    return ls.cell_value(chn, bno, ix, iy, iz);
  }
};

// the level set as the shape of ColliderDev::resolve_with
template <class Fetch> struct LevelSetShape {
  const LevelSetView &ls;
  const Fetch &f;
  __device__ __forceinline__ float signed_distance(const float (&X)[3]) const { return ls.getSignedDistance(f, X); }
  __device__ __forceinline__ void normal(const float (&X)[3], float (&n)[3]) const { ls.getNormal(f, X, n); }
  __device__ __forceinline__ bool material_velocity(const float (&X)[3], float (&vm)[3]) const { return ls.getMaterialVelocity(f, X, vm); }
};

// Collider<LevelSetBoundary<SparseGrid<3>>> (geometry/Collider.h:10-110): type and motion of a zs_rocm_collider (its geometry / param
// are not read) around a level set; transform and response are ColliderDev's
struct LevelSetColliderDev {
  ColliderDev motion;
  LevelSetView ls;
  template <class Fetch> __device__ __forceinline__ bool resolveCollision(const Fetch &f, const float (&x)[3], float (&v)[3], float erosion = 0.f) const {
    return motion.resolve_with(LevelSetShape<Fetch>{ls, f}, x, v, erosion);
  }
  __device__ __forceinline__ bool resolveCollision(const float (&x)[3], float (&v)[3], float erosion = 0.f) const {
    return resolveCollision(LevelSetDirectFetch(ls), x, v, erosion);
  }
};

// ---- keyframed level sets: the blend of two level sets `src` and `dst` a keyframe spacing stepDt apart, at the phase alpha in [0, 1]
// between them (the reference's TransitionLevelSetView over the two front entries of a keyframe queue, geometry/LevelSet.h).  At a point
// x of level-set world space every call first moves x along the mean material velocity, back to the time of src and on to the time of dst:
//   vs  = src.getMaterialVelocity(x)        vd = dst.getMaterialVelocity(x)        (0 for a level set without "v")
//   v_d = (vs_d + vd_d) * 0.5f
//   a0  = alpha * stepDt                    a1 = (1.f - alpha) * stepDt
//   x0_d = x_d - a0 * v_d                   x1_d = x_d + a1 * v_d
// and then blends the two level sets' own answers, component by component:
//   getSignedDistance(x)   = (1.f - alpha) * src.getSignedDistance(x0)   + alpha * dst.getSignedDistance(x1)
//   getNormal(x)           = (1.f - alpha) * src.getNormal(x0)           + alpha * dst.getNormal(x1)              (not renormalised)
//   getMaterialVelocity(x) = (1.f - alpha) * src.getMaterialVelocity(x0) + alpha * dst.getMaterialVelocity(x1)
// Every line is ONE float32 operation per operator as written, left to right, without contraction: the tests reproduce the chain up to
// x0 and x1 in numpy float32 (tests/ref64_transition.py), so every path -- the per-point entries, the staged block kernels, the C++
// face -- keeps this order.  Each level set reads its cells through its own fetch functor.  Where a level set's gradient vanishes (a
// stencil of equal values, as beyond its band) its normal is 0 / 0 and so is the blend, as in the reference: keep stepDt * speed inside
// the band (zpc_amd.levelset.LevelSetSequence.push checks it).
struct TransitionLevelSetView {
  LevelSetView src, dst;
  float stepDt, alpha;
  __host__ __device__ TransitionLevelSetView() = default;
  __host__ __device__ TransitionLevelSetView(const zs_rocm_levelset_transition &t) : src(t.src), dst(t.dst), stepDt(t.stepDt), alpha(t.alpha) {}

  __host__ __device__ __forceinline__ bool has_velocity() const { return src.velChannel >= 0 || dst.velChannel >= 0; }
  // the two displaced sample points of x
  template <class FS, class FD>
  __device__ __forceinline__ void displaced(const FS &fs, const FD &fd, const float (&x)[3], float (&x0)[3], float (&x1)[3]) const {
    float vs[3], vd[3];
    src.getMaterialVelocity(fs, x, vs);
    dst.getMaterialVelocity(fd, x, vd);
    const float a0 = alpha * stepDt, a1 = (1.f - alpha) * stepDt;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = (vs[d] + vd[d]) * 0.5f;
      x0[d] = x[d] - a0 * v;
      x1[d] = x[d] + a1 * v;
    }
  }
  // the blends at displaced points already formed
  template <class FS, class FD> __device__ __forceinline__ float sdf_at(const FS &fs, const FD &fd, const float (&x0)[3], const float (&x1)[3]) const {
    return (1.f - alpha) * src.getSignedDistance(fs, x0) + alpha * dst.getSignedDistance(fd, x1);
  }
  template <class FS, class FD>
  __device__ __forceinline__ void normal_at(const FS &fs, const FD &fd, const float (&x0)[3], const float (&x1)[3], float (&n)[3]) const {
    float ns[3], nd[3];
    src.getNormal(fs, x0, ns);
    dst.getNormal(fd, x1, nd);
#pragma unroll
    for (int d = 0; d < 3; ++d) n[d] = (1.f - alpha) * ns[d] + alpha * nd[d];
  }
  // false (and vm = 0) when neither level set has "v"
  template <class FS, class FD>
  __device__ __forceinline__ bool velocity_at(const FS &fs, const FD &fd, const float (&x0)[3], const float (&x1)[3], float (&vm)[3]) const {
    float vs[3], vd[3];
    src.getMaterialVelocity(fs, x0, vs);
    dst.getMaterialVelocity(fd, x1, vd);
#pragma unroll
    for (int d = 0; d < 3; ++d) vm[d] = (1.f - alpha) * vs[d] + alpha * vd[d];
    return has_velocity();
  }
  template <class FS, class FD> __device__ __forceinline__ float getSignedDistance(const FS &fs, const FD &fd, const float (&x)[3]) const {
    float x0[3], x1[3];
    displaced(fs, fd, x, x0, x1);
    return sdf_at(fs, fd, x0, x1);
  }
  template <class FS, class FD> __device__ __forceinline__ void getNormal(const FS &fs, const FD &fd, const float (&x)[3], float (&n)[3]) const {
    float x0[3], x1[3];
    displaced(fs, fd, x, x0, x1);
    normal_at(fs, fd, x0, x1, n);
  }
  template <class FS, class FD>
  __device__ __forceinline__ bool getMaterialVelocity(const FS &fs, const FD &fd, const float (&x)[3], float (&vm)[3]) const {
    float x0[3], x1[3];
    displaced(fs, fd, x, x0, x1);
    return velocity_at(fs, fd, x0, x1, vm);
  }
};

// the transition as the shape of ColliderDev::resolve_with.  The three calls of one resolveCollision come at the same X: the displaced
// points are formed at the first and kept (the same operations on the same inputs, so the same bits as forming them three times).
template <class FS, class FD> struct TransitionShape {
  const TransitionLevelSetView &tr;
  const FS &fs;
  const FD &fd;
  mutable float at[3], x0[3], x1[3];
  mutable bool have;
  __device__ __forceinline__ TransitionShape(const TransitionLevelSetView &t, const FS &s, const FD &d) : tr(t), fs(s), fd(d), have(false) {}
  __device__ __forceinline__ void move_to(const float (&X)[3]) const {
    if (have && X[0] == at[0] && X[1] == at[1] && X[2] == at[2]) return;
    tr.displaced(fs, fd, X, x0, x1);
    at[0] = X[0]; at[1] = X[1]; at[2] = X[2];
    have = true;
  }
  __device__ __forceinline__ float signed_distance(const float (&X)[3]) const { move_to(X); return tr.sdf_at(fs, fd, x0, x1); }
  __device__ __forceinline__ void normal(const float (&X)[3], float (&n)[3]) const { move_to(X); tr.normal_at(fs, fd, x0, x1, n); }
  __device__ __forceinline__ bool material_velocity(const float (&X)[3], float (&vm)[3]) const { move_to(X); return tr.velocity_at(fs, fd, x0, x1, vm); }
};

// Collider over the transition: type and motion of a zs_rocm_collider around the blended level set
struct TransitionColliderDev {
  ColliderDev motion;
  TransitionLevelSetView tr;
  template <class FS, class FD>
  __device__ __forceinline__ bool resolveCollision(const FS &fs, const FD &fd, const float (&x)[3], float (&v)[3], float erosion = 0.f) const {
    return motion.resolve_with(TransitionShape<FS, FD>(tr, fs, fd), x, v, erosion);
  }
  __device__ __forceinline__ bool resolveCollision(const float (&x)[3], float (&v)[3], float erosion = 0.f) const {
    return resolveCollision(LevelSetDirectFetch(tr.src), LevelSetDirectFetch(tr.dst), x, v, erosion);
  }
};

}  // namespace zsr
