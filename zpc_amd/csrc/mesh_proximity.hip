// mesh_proximity.hip -- the contact pairs of a triangle mesh with itself for gfx950: the vertex-triangle and edge-edge pairs closer than a
// contact distance dHat, topological neighbours removed, each with its squared distance and the feature pair it is realised on (the job
// of dist_pt_sqr / pt_category_and_dist2 / dist_ee_sqr / ee_category_and_dist2, geometry/SpatialQuery.hpp:19-500, on top of
// LBvhView::iter_neighbors / self_iter_neighbors, container/Bvh.hpp:644-728).  The tree walk and the exact test sit in one kernel; only
// real contacts are written.
//
//   PT   lane = vertex (in Morton order from 16384 vertices up, as the bulk queries); every lane walks the packed triangle tree with its
//        point's box dilated by dHat -- lbvh.hip's per-lane walk, one node per lane and step, the steps taken by the wave together.
//   EE   lane = leaf of the edge tree; the wave walks the union of its lanes' self-walks in pre-order (lbvh.hip's wave walk: the node is
//        fetched once per step), every leaf with its own box dilated by dHat, so a pair is met once, from the earlier leaf.
//   test At any step only a few lanes are at an overlapping leaf.  They do not run the exact test there: they append (owner lane,
//        candidate) to a queue of the wave in LDS (positions from a ballot: step-major, lane-minor).  Once 64 candidates wait, and at
//        the end, the wave runs the test with lane = candidate: topological exclusion, tri_closest / ee_closest, dist2 < dHat^2.
//   rank The hits of one batch are ranked per owner from the queue order (a ballot per distinct owner among the hits), on top of the
//        owner's running count -- no atomics: the position of every hit inside its owner's run is a function of the input alone.
//   cache The count pass remembers the first PROX_CACHE hit candidates of every owner (hit-major, as lbvh.hip's self-query), 4 bytes each.
//        The fill pass does not walk for owners whose hits all fit: the wave enumerates their cached hits with lane = hit, repeats the
//        exact test for the distance and the coordinates (the same arithmetic on the same input: the same bits) and writes them at
//        offset + rank.  Owners with more hits walk again.  The cache belongs to (mesh positions, dHat) of the last count pass; a fill
//        pass with another dHat, or after a refit, walks for everyone.
// Count pass -> exclusive scan by the caller -> fill pass (the same kernel with FILL): two calls give byte-identical lists.
// One wave per workgroup (as the self-query); LDS: 2 x 128 ints.  Built with -ffp-contract=off (zpc_amd/build.py).
#include <cfloat>
#include <cstring>

#include "mesh.hpp"

namespace zsr {

constexpr int PROX_BLOCK = 64, PROX_QUEUE = 128;  // a push adds at most 64 entries to fewer than 64 waiting ones
constexpr int PROX_CACHE = 32;                    // cached hit candidates per owner (128 bytes per vertex / edge)

__global__ __launch_bounds__(256) void prox_pack_kernel(LBvhDev bvh, MeshPackedNode *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bvh.numNodes) return;
  const AABB3 b = bvh.orderedBvs[i];
  MeshPackedNode n;
#pragma unroll
  for (int d = 0; d < 3; ++d) { n.lo[d] = b.lo[d]; n.hi[d] = b.hi[d]; }
  n.level = bvh.numNodes > 2 ? bvh.levels[i] : 0;  // (the small-tree form: every node is a leaf, its number the primitive's)
  n.aux = bvh.numNodes > 2 ? bvh.auxIndices[i] : i;
  if (bvh.numNodes > 2 && n.level != 0 && n.aux < 0) n.aux = bvh.numNodes;  // escape index behind the last subtree: one past the end
  out[i] = n;
}

__global__ __launch_bounds__(256) void prox_edge_box_kernel(const float *verts, const int *edges, int ne, float *boxes) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const int i = edges[2 * e], j = edges[2 * e + 1];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float a = verts[3 * (size_t)i + d], b = verts[3 * (size_t)j + d];
    boxes[6 * (size_t)e + d] = fminf(a, b);
    boxes[6 * (size_t)e + 3 + d] = fmaxf(a, b);
  }
}

__device__ __forceinline__ unsigned prox_expand_bits(unsigned v) {  // math/bit/Bits.h:84-90
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
// 30-bit Morton code of a vertex inside the root box (an ordering only)
__global__ __launch_bounds__(256) void prox_point_code_kernel(const MeshPackedNode *nodes, const float *pts, int n, unsigned *codes, int *ids) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const MeshPackedNode r = nodes[0];
  unsigned code = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float len = r.hi[d] - r.lo[d];
    float u = len > 0.f ? (pts[3 * (size_t)i + d] - r.lo[d]) / len : 0.f;
    u = u > 0.f ? (u > 0.999999f ? 0.999999f : u) : 0.f;  // (NaN -> 0)
    code |= prox_expand_bits((unsigned)(u * 1024.f)) << (2 - d);
  }
  codes[i] = code;
  ids[i] = i;
}

// ---------------------------------------------------------------------------------------------------------------- the wave's queue
// flagged lanes append (their lane, cand) behind the qn waiting entries, in lane order; qn is wave-uniform
__device__ __forceinline__ void prox_push(int *sOwner, int *sCand, int &qn, bool flag, int cand) {
  const unsigned long long m = __ballot(flag);
  if (flag) {
    const int pos = qn + __popcll(m & lanemask_lt());
    sOwner[pos] = lane_id();
    sCand[pos] = cand;
  }
  qn += __popcll(m);
}
// Takes the first min(qn, 64) entries, lane = entry, and moves the rest to the front.  exact(have, ownerLane, cand) -> hit is called by
// every lane (it may shuffle); emit(position) by the lanes with a hit: position = off of the owner + the owner's count so far + the rank
// of the hit among the batch's hits of the same owner, in queue order.  c: the running count, kept by the owner's lane.
template <class Exact, class Emit>
__device__ __forceinline__ void prox_flush(int *sOwner, int *sCand, int &qn, int &c, int off, Exact &&exact, Emit &&emit) {
  const int lane = lane_id();
  __syncthreads();  // (one wave per workgroup: orders the pushes before the reads)
  const int take = qn < 64 ? qn : 64;
  const bool have = lane < take, rest = lane + 64 < qn;
  const int owner = have ? sOwner[lane] : 0, cand = have ? sCand[lane] : 0;
  const int ro = rest ? sOwner[lane + 64] : 0, rc = rest ? sCand[lane + 64] : 0;
  __syncthreads();
  if (rest) {
    sOwner[lane] = ro;
    sCand[lane] = rc;
  }
  qn -= take;
  const bool hit = exact(have, owner, cand);
  unsigned long long rem = __ballot(hit);
  while (rem) {  // one round per distinct owner among the hits
    const int o = __shfl(owner, __ffsll((long long)rem) - 1, 64);
    const bool mine = hit && owner == o;
    const unsigned long long m = __ballot(mine);
    const int base = __shfl(off, o, 64) + __shfl(c, o, 64);
    if (mine) emit(base + __popcll(m & lanemask_lt()));
    if (lane == o) c += __popcll(m);
    rem &= ~m;
  }
}

// The fill pass of the owners whose hits the count pass cached: cc = the lane's cached hits (0: none, or too many to be cached).  The
// wave enumerates the hits of all its lanes, lane = hit: hit number pp belongs to the last lane whose exclusive prefix of cc is <= pp
// (lanes without hits share their successor's prefix).  cache[j * n + k0 + lane] = candidate of that lane's j-th hit.
template <class Exact, class Emit>
__device__ __forceinline__ void prox_replay(const int *__restrict__ cache, size_t n, int k0, int cc, int off, Exact &&exact, Emit &&emit) {
  const int lane = lane_id();
  int incl = cc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  const int pre = incl - cc, total = __shfl(incl, 63, 64);
  for (int p0 = 0; p0 < total; p0 += 64) {  // (wave-uniform trip count: the shuffles below need every lane)
    const int pp = p0 + lane;
    int lo = 0, hi = 63;
#pragma unroll
    for (int it = 0; it < 6; ++it) {
      const int mid = (lo + hi + 1) >> 1;
      if (__shfl(pre, mid, 64) <= pp) lo = mid;
      else hi = mid - 1;
    }
    const bool have = pp < total;
    const int j = pp - __shfl(pre, lo, 64), oOff = __shfl(off, lo, 64);
    const int cand = have ? cache[(size_t)j * n + (size_t)(k0 + lo)] : 0;
    if (exact(have, lo, cand)) emit(oOff + j);
  }
}

// ---------------------------------------------------------------------------------------------------------------- PT
template <bool FILL>
__global__ __launch_bounds__(PROX_BLOCK) void prox_pt_kernel(const MeshPackedNode *__restrict__ nodes, int numNodes, const float *__restrict__ verts,
                                                             const int *__restrict__ tris, int nv, float dHat, const int *__restrict__ perm,
                                                             int *counts, const int *offsets, int *pairs, float *dist2, int *feature,
                                                             float *bary, int *cache, int *cacheCounts) {
  __shared__ int sOwner[PROX_QUEUE], sCand[PROX_QUEUE];
  const int k0 = blockIdx.x * PROX_BLOCK, k = k0 + (int)threadIdx.x;
  const bool valid = k < nv;
  const int vi = valid ? (perm ? perm[k] : k) : 0;
  float lo[3], hi[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float x = verts[3 * (size_t)vi + d];
    lo[d] = x - dHat;
    hi[d] = x + dHat;
  }
  const float d2max = dHat * dHat;
  const int off = FILL && valid ? offsets[vi] : 0;
  int c = 0, qn = 0;
  TriClosest res;
  int resV = 0, resT = 0, resOwner = 0;
  auto exact = [&](bool have, int owner, int cand) -> bool {
    resV = __shfl(vi, owner, 64);
    resT = cand;
    resOwner = owner;
    if (!have) return false;
    const int i0 = tris[3 * (size_t)cand], i1 = tris[3 * (size_t)cand + 1], i2 = tris[3 * (size_t)cand + 2];
    if (i0 == resV || i1 == resV || i2 == resV) return false;  // the triangle contains the vertex
    float p[3], a[3], b[3], cc[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      p[d] = verts[3 * (size_t)resV + d];
      a[d] = verts[3 * (size_t)i0 + d];
      b[d] = verts[3 * (size_t)i1 + d];
      cc[d] = verts[3 * (size_t)i2 + d];
    }
    res = tri_closest(p, a, b, cc);
    return res.dist2 < d2max;
  };
  auto emit = [&](int pos) {
    if constexpr (FILL) {
      if (pairs) { pairs[2 * (size_t)pos] = resV; pairs[2 * (size_t)pos + 1] = resT; }
      if (dist2) dist2[pos] = res.dist2;
      if (feature) feature[pos] = res.feature;
      if (bary) { bary[3 * (size_t)pos] = res.bary[0]; bary[3 * (size_t)pos + 1] = res.bary[1]; bary[3 * (size_t)pos + 2] = res.bary[2]; }
    } else {  // (count pass: off = 0, pos = the rank of the hit at its owner)
      if (cache && pos < PROX_CACHE) cache[(size_t)pos * (size_t)nv + (size_t)(k0 + resOwner)] = resT;
    }
  };
  bool need = valid;
  if constexpr (FILL) {
    if (cache) {
      const int cc = valid ? cacheCounts[k] : 0;
      need = cc > PROX_CACHE;
      prox_replay(cache, (size_t)nv, k0, need ? 0 : cc, off, exact, emit);
    }
  }
  int node = need ? 0 : numNodes;
  while (__ballot(node < numNodes)) {
    bool push = false;
    int cand = 0;
    if (node < numNodes) {
      const MeshPackedNode n = nodes[node];
      bool ov = true;
#pragma unroll
      for (int d = 0; d < 3; ++d) ov = ov && !(lo[d] > n.hi[d] || hi[d] < n.lo[d]);
      if (n.level == 0) {
        push = ov;
        cand = n.aux;
        node++;
      } else
        node = ov ? node + 1 : n.aux;
    }
    prox_push(sOwner, sCand, qn, push, cand);
    if (qn >= 64) prox_flush(sOwner, sCand, qn, c, off, exact, emit);
  }
  if (qn > 0) prox_flush(sOwner, sCand, qn, c, off, exact, emit);
  if (!FILL && valid) {
    counts[vi] = c;
    if (cacheCounts) cacheCounts[k] = c;
  }
}

// ---------------------------------------------------------------------------------------------------------------- EE
// The walk is lbvh.hip's lbvh_self_query_wave_kernel (see there for why the next node of the wave needs no reduction); a leaf's own box is
// dilated by dHat and the leaf hits go to the queue.
template <bool FILL>
__global__ __launch_bounds__(PROX_BLOCK) void prox_ee_kernel(const MeshPackedNode *__restrict__ nodes, int numNodes, int numLeaves,
                                                             const int *__restrict__ leafInds, const float *__restrict__ verts,
                                                             const int *__restrict__ edges, float dHat, int *counts, const int *offsets, int *pairs,
                                                             float *dist2, int *category, float *st, int *cache, int *cacheCounts) {
  typedef int v8i __attribute__((ext_vector_type(8)));
  constexpr int NONE = 0x7fffffff;
  __shared__ int sOwner[PROX_QUEUE], sCand[PROX_QUEUE];
  const int k0 = blockIdx.x * PROX_BLOCK, k = k0 + (int)threadIdx.x;
  const bool valid = k < numLeaves;
  const int start = valid ? leafInds[k] : NONE;
  MeshPackedNode me{};
  if (valid) me = nodes[start];
  const int self = me.aux;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    me.lo[d] -= dHat;
    me.hi[d] += dHat;
  }
  const float d2max = dHat * dHat;
  const int off = FILL && valid ? offsets[k] : 0;
  int c = 0, qn = 0;
  EdgeClosest res;
  int resI = 0, resJ = 0, resOwner = 0, resCand = 0;
  auto exact = [&](bool have, int owner, int cand) -> bool {
    const int oe = __shfl(self, owner, 64);
    resOwner = owner;
    resCand = cand;
    resI = oe < cand ? oe : cand;
    resJ = oe < cand ? cand : oe;
    if (!have) return false;
    const int i0 = edges[2 * (size_t)resI], i1 = edges[2 * (size_t)resI + 1], j0 = edges[2 * (size_t)resJ], j1 = edges[2 * (size_t)resJ + 1];
    if (i0 == j0 || i0 == j1 || i1 == j0 || i1 == j1) return false;  // the edges share a vertex
    float a0[3], a1[3], b0[3], b1[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a0[d] = verts[3 * (size_t)i0 + d];
      a1[d] = verts[3 * (size_t)i1 + d];
      b0[d] = verts[3 * (size_t)j0 + d];
      b1[d] = verts[3 * (size_t)j1 + d];
    }
    res = ee_closest(a0, a1, b0, b1);
    return res.dist2 < d2max;
  };
  auto emit = [&](int pos) {
    if constexpr (FILL) {
      if (pairs) { pairs[2 * (size_t)pos] = resI; pairs[2 * (size_t)pos + 1] = resJ; }
      if (dist2) dist2[pos] = res.dist2;
      if (category) category[pos] = res.category;
      if (st) { st[2 * (size_t)pos] = res.s; st[2 * (size_t)pos + 1] = res.t; }
    } else {  // (count pass: off = 0, pos = the rank of the hit at its owner)
      if (cache && pos < PROX_CACHE) cache[(size_t)pos * (size_t)numLeaves + (size_t)(k0 + resOwner)] = resCand;
    }
  };
  bool need = valid;
  if constexpr (FILL) {
    if (cache) {
      const int cc = valid ? cacheCounts[k] : 0;
      need = cc > PROX_CACHE;
      prox_replay(cache, (size_t)numLeaves, k0, need ? 0 : cc, off, exact, emit);
    }
  }
  int next = need ? start : NONE;  // the walk starts AT the leaf, which reports itself first (skipped below)
  unsigned long long pending = __ballot(need);  // lanes that have not started yet, in lane (= leaf = node) order
  int nextStart = NONE;
  if (pending) nextStart = __builtin_amdgcn_readlane(start, __ffsll((long long)pending) - 1);
  int cur = nextStart;
  while (cur < numNodes) {
    if (cur == nextStart) {
      pending &= pending - 1;
      nextStart = NONE;
      if (pending) nextStart = __builtin_amdgcn_readlane(start, __ffsll((long long)pending) - 1);
    }
    const v8i raw = *reinterpret_cast<const v8i *>(reinterpret_cast<const char *>(nodes) + ((unsigned)cur << 5));
    const float nlo0 = __int_as_float(raw[0]), nlo1 = __int_as_float(raw[1]), nlo2 = __int_as_float(raw[2]);
    const float nhi0 = __int_as_float(raw[3]), nhi1 = __int_as_float(raw[4]), nhi2 = __int_as_float(raw[5]);
    const int level = raw[6], aux = raw[7];
    const bool active = next == cur;
    // the six interval tests as one compare (exact, see lbvh.hip)
    const float sep = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(me.lo[0] - nhi0, nlo0 - me.hi[0]), __builtin_fmaxf(me.lo[1] - nhi1, nlo1 - me.hi[1])),
                                      __builtin_fmaxf(me.lo[2] - nhi2, nlo2 - me.hi[2]));
    const bool ov = !(sep > 0.f);
    const unsigned long long downMask = __ballot(active) & __ballot(ov);
    if (__builtin_amdgcn_readfirstlane(level) == 0) {  // a leaf (wave-uniform branch): queue it, continue at cur + 1
      prox_push(sOwner, sCand, qn, active && ov && aux != self, aux);
      if (qn >= 64) prox_flush(sOwner, sCand, qn, c, off, exact, emit);
      if (active) next = cur + 1;
      cur = cur + 1;
    } else {  // a trunk node: descend on overlap, escape otherwise
      const bool down = active && ov;
      if (active) next = down ? cur + 1 : aux;
      if (downMask) cur = cur + 1;
      else cur = aux < nextStart ? aux : nextStart;
    }
  }
  if (qn > 0) prox_flush(sOwner, sCand, qn, c, off, exact, emit);
  if (!FILL && valid) {
    counts[k] = c;
    if (cacheCounts) cacheCounts[k] = c;
  }
}

static LBvhDev prox_tree(const zs_rocm_lbvh *b) {
  zs_rocm_lbvh_view v;
  zs_rocm_lbvh_get_view(b, &v);
  LBvhDev d;
  d.orderedBvs = (const AABB3 *)v.orderedBvs; d.parents = v.parents; d.levels = v.levels; d.leafInds = v.leafInds; d.auxIndices = v.auxIndices;
  d.numNodes = v.numNodes;
  return d;
}
// the packed nodes of a tree, refreshed after a build / refit (a mesh keeps its topology: the node count never changes)
static const MeshPackedNode *prox_packed(Launch &L, const LBvhDev &d, MeshPackedNode *&buf, bool &valid) {
  if (!buf) ZSR_CHECK(hipMalloc((void **)&buf, sizeof(MeshPackedNode) * (size_t)d.numNodes));
  if (!valid) {
    hipLaunchKernelGGL(prox_pack_kernel, dim3(ceil_div(d.numNodes, 256)), dim3(256), 0, L.stream, d, buf);
    valid = true;
  }
  return buf;
}
static void prox_edge_boxes(Launch &L, zs_rocm_mesh &m) {
  hipLaunchKernelGGL(prox_edge_box_kernel, dim3(ceil_div(m.ne, 256)), dim3(256), 0, L.stream, m.verts, m.edges, (int)m.ne, m.edgeBoxes);
}
// the edge tree, built by the first edge-edge query
static void prox_edge_tree(zs_rocm_policy *pol, zs_rocm_mesh &m) {
  if (m.edgeBvh || !m.ne) return;
  {
    Launch L(pol, "mesh_proximity (edge boxes)");
    ZSR_CHECK(hipMalloc((void **)&m.edgeBoxes, sizeof(float) * 6 * m.ne));
    prox_edge_boxes(L, m);
  }
  m.edgeBvh = zs_rocm_lbvh_create();
  zs_rocm_lbvh_build(pol, m.edgeBvh, m.edgeBoxes, m.ne, 1);
  m.edgePackedValid = false;
}

// the hit cache of a count pass: allocated on first use; without memory for it the passes run uncached
static void prox_cache(int *&cache, int *&cacheCounts, size_t n) {
  if (cache) return;
  if (hipMalloc((void **)&cache, sizeof(int) * n * PROX_CACHE) != hipSuccess || hipMalloc((void **)&cacheCounts, sizeof(int) * n) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(cache);
    cache = cacheCounts = nullptr;
  }
}
static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

int mesh_proximity_refit(zs_rocm_policy *pol, zs_rocm_mesh &m) {
  m.triPackedValid = false;
  m.ptCacheValid = m.eeCacheValid = false;
  if (!m.edgeBvh) return 0;
  {
    Launch L(pol, "mesh_refit (edge boxes)");
    prox_edge_boxes(L, m);
  }
  m.edgePackedValid = false;
  return zs_rocm_lbvh_refit(pol, m.edgeBvh, m.edgeBoxes, m.ne);
}

static bool prox_ok(zs_rocm_policy *pol, const zs_rocm_mesh *m, float dHat) { return pol && m && m->bvh && m->stats && dHat > 0.f && dHat <= FLT_MAX; }

template <bool FILL>
static int prox_pt(zs_rocm_policy *pol, const zs_rocm_mesh *m, float dHat, int *counts, const int *offsets, int *pairs, float *dist2, int *feature,
                   float *bary) {
  if (!prox_ok(pol, m, dHat) || (m->nv && !(FILL ? (const void *)offsets : (const void *)counts))) return -1;
  Launch L(pol, FILL ? "mesh_proximity_pt_fill" : "mesh_proximity_pt_count");
  if (!m->nv) return 0;
  if (!m->nt) {
    if (!FILL) ZSR_CHECK(hipMemsetAsync(counts, 0, sizeof(int) * m->nv, L.stream));
    return 0;
  }
  const LBvhDev d = prox_tree(m->bvh);
  const MeshPackedNode *nodes = prox_packed(L, d, m->triPacked, m->triPackedValid);
  const int *perm = nullptr;
  if (m->nv >= 16384 && d.numNodes > 2) {  // Morton order of the vertices inside the root box, as the bulk queries
    unsigned *codes = (unsigned *)L.temp(sizeof(unsigned) * m->nv), *sorted = (unsigned *)L.temp(sizeof(unsigned) * m->nv);
    int *ids = (int *)L.temp(sizeof(int) * m->nv), *p = (int *)L.temp(sizeof(int) * m->nv);
    hipLaunchKernelGGL(prox_point_code_kernel, dim3(ceil_div(m->nv, 256)), dim3(256), 0, L.stream, nodes, m->verts, (int)m->nv, codes, ids);
    radix_sort_pair_u32(L, codes, ids, sorted, p, m->nv, 0, 30);
    perm = p;
  }
  if (!FILL) {
    prox_cache(m->ptCache, m->ptCacheCounts, m->nv);
    m->ptCacheValid = m->ptCache != nullptr;
    m->ptCacheDHat = dHat;
  }
  const bool useCache = m->ptCacheValid && same_bits(m->ptCacheDHat, dHat);
  hipLaunchKernelGGL((prox_pt_kernel<FILL>), dim3(ceil_div(m->nv, PROX_BLOCK)), dim3(PROX_BLOCK), 0, L.stream, nodes, d.numNodes, m->verts, m->tris,
                     (int)m->nv, dHat, perm, counts, offsets, pairs, dist2, feature, bary, useCache ? m->ptCache : nullptr,
                     useCache ? m->ptCacheCounts : nullptr);
  return 0;
}

template <bool FILL>
static int prox_ee(zs_rocm_policy *pol, zs_rocm_mesh *m, float dHat, int *counts, const int *offsets, int *pairs, float *dist2, int *category,
                   float *st) {
  if (!prox_ok(pol, m, dHat) || (m->ne && !(FILL ? (const void *)offsets : (const void *)counts))) return -1;
  if (m->ne >= (1u << 26)) return -1;  // (the walk addresses nodes by a 32-bit byte offset, node << 5)
  if (!m->ne) return 0;
  prox_edge_tree(pol, *m);
  Launch L(pol, FILL ? "mesh_proximity_ee_fill" : "mesh_proximity_ee_count");
  const LBvhDev d = prox_tree(m->edgeBvh);
  const MeshPackedNode *nodes = prox_packed(L, d, m->edgePacked, m->edgePackedValid);
  if (!FILL) {
    prox_cache(m->eeCache, m->eeCacheCounts, m->ne);
    m->eeCacheValid = m->eeCache != nullptr;
    m->eeCacheDHat = dHat;
  }
  const bool useCache = m->eeCacheValid && same_bits(m->eeCacheDHat, dHat);
  hipLaunchKernelGGL((prox_ee_kernel<FILL>), dim3(ceil_div(m->ne, PROX_BLOCK)), dim3(PROX_BLOCK), 0, L.stream, nodes, d.numNodes, (int)m->ne, d.leafInds,
                     m->verts, m->edges, dHat, counts, offsets, pairs, dist2, category, st, useCache ? m->eeCache : nullptr,
                     useCache ? m->eeCacheCounts : nullptr);
  return 0;
}

}  // namespace zsr

using namespace zsr;

extern "C" {

size_t zs_rocm_mesh_num_edges(const zs_rocm_mesh *m) { return m ? m->ne : 0; }

int zs_rocm_mesh_edges(zs_rocm_policy *pol, const zs_rocm_mesh *m, int *edges) {
  if (!pol || !m || !m->stats || (m->ne && !edges)) return -1;
  Launch L(pol, "mesh_edges");
  if (m->ne) ZSR_CHECK(hipMemcpyAsync(edges, m->edges, sizeof(int) * 2 * m->ne, hipMemcpyDeviceToDevice, L.stream));
  return 0;
}

int zs_rocm_mesh_proximity_pt_count(zs_rocm_policy *pol, const zs_rocm_mesh *m, float dHat, int *counts) {
  return prox_pt<false>(pol, m, dHat, counts, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int zs_rocm_mesh_proximity_pt_fill(zs_rocm_policy *pol, const zs_rocm_mesh *m, float dHat, const int *offsets, int *pairs, float *dist2,
                                   int *feature, float *bary) {
  return prox_pt<true>(pol, m, dHat, nullptr, offsets, pairs, dist2, feature, bary);
}
int zs_rocm_mesh_proximity_ee_count(zs_rocm_policy *pol, zs_rocm_mesh *m, float dHat, int *counts) {
  return prox_ee<false>(pol, m, dHat, counts, nullptr, nullptr, nullptr, nullptr, nullptr);
}
int zs_rocm_mesh_proximity_ee_fill(zs_rocm_policy *pol, zs_rocm_mesh *m, float dHat, const int *offsets, int *pairs, float *dist2, int *category,
                                   float *st) {
  return prox_ee<true>(pol, m, dHat, nullptr, offsets, pairs, dist2, category, st);
}

}  // extern "C"
