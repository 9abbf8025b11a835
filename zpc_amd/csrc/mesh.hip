// mesh.hip -- triangle meshes as level-set colliders for gfx950: the mesh object (LBvh over the triangle boxes + face normals + vertex and
// edge pseudonormals), the bulk closest-point / signed-distance queries (LBvhView::find_nearest, container/Bvh.hpp:547-590, with the
// point-triangle distance of include/zensim_rocm/distance_device.hpp as the functor) and the conversion mesh -> SparseGrid<3, f32, 8>.
//
// Mesh -> level set, per candidate block (one workgroup of 512, lane = cell):
//   centre      lane 0 walks the tree from the block's centre c: d_c.  No cell of the block is nearer than d_c - r (r = 3.5 sqrt(3) voxel,
//               the half diagonal over the cell centres), so d_c - r > band rejects the block before anything else is done: most
//               candidates of a triangle's dilated box end here.
//   cull        every cell's nearest triangle lies within R = min(d_c + r, band + 7 sqrt(3) voxel) of the block's box (a kept block has a
//               cell nearer than band, so none of its cells is farther than the second bound).  The workgroup walks the tree breadth
//               first -- a frontier queue in LDS, one node per lane and round; the children of trunk node k are k + 1 and the escape index
//               of k + 1 (k + 2 after a leaf) -- and collects the triangles whose boxes are within R of the block's box.
//   stage       their vertices go to LDS, 48 bytes per triangle (9 floats, the triangle's number, 16-byte aligned).  Normals are NOT
//               staged: a lane needs the pseudonormal of one feature of one triangle, after the loop; staging 18 more floats per triangle
//               would cut the list to a third for values 511 of 512 lanes never read.
//   distance    every lane runs tri_closest over the list; all lanes read the same triangle, a same-address LDS broadcast.  Only (dist2,
//               triangle) is carried through the loop; the winner is evaluated once more for the closest point, sign and velocity.  Among
//               the listed triangles equal distances go to the smaller triangle number, so the result does not depend on the order the
//               atomics gave the list.  (The per-lane walk applies the rule among the leaves it visits only: on an exact tie the two
//               paths may name different triangles at the same distance.)
//   fallback    more than MESH_STAGE_TRIS survivors or a full queue: every lane walks the tree itself (TriMeshDev::nearest_triangle, the
//               bulk query's code).  A brute-force pass costs list length x 512; the per-lane walk visits a few dozen nodes, so meshes much
//               finer than the voxel belong here anyway.
// LDS: 640 x 48 B list + 2 x 4 KB queues + counters = 39 192 B: four workgroups fit in a CU's 160 KB, so LDS is not what limits residency;
// the kernel's 74 VGPRs are (6 waves per SIMD: three workgroups of 8 waves per CU).
// Built with -ffp-contract=off (zpc_amd/build.py).
#include <cfloat>

#include "common.hpp"
#include "bht.hpp"
#include "mesh.hpp"

namespace zsr {

void radix_sort_pair_u64(Launch &L, const unsigned long long *kin, const int *vin, unsigned long long *kout, int *vout, size_t n, int sbit,
                         int ebit);

constexpr int MESH_STAGE_TRIS = 640, MESH_STAGE_STRIDE = 12, MESH_QUEUE = 1024;
constexpr int MESH_LS_SIDE = 8, MESH_LS_BLOCK = 512;
constexpr unsigned MESH_LS_MAX_PER_TRI = 1u << 22;  // blocks under one triangle's dilated box; more: the call fails
enum { MESH_BOUNDARY = 0, MESH_NONMANIFOLD = 1, MESH_INCONSISTENT = 2, MESH_ZERO_AREA = 3, MESH_BAD_INDEX = 4 };

__global__ __launch_bounds__(256) void mesh_copy_tris_kernel(const int *in, size_t n3, int nv, int *out, int *stats) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  int v = in[i];
  if (v < 0 || v >= nv) {
    atomicAdd(stats + MESH_BAD_INDEX, 1);
    v = v < 0 ? 0 : nv - 1;
  }
  out[i] = v;
}

// boxes, unit face normals (0 for a zero-area triangle, by the test of tri_closest) and the three corner angles
__global__ __launch_bounds__(256) void mesh_face_kernel(const float *verts, const int *tris, int nt, float *boxes, float *faceN, float *angles,
                                                        int *stats) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  float a[3], b[3], c[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a[d] = verts[3 * tris[3 * t] + d];
    b[d] = verts[3 * tris[3 * t + 1] + d];
    c[d] = verts[3 * tris[3 * t + 2] + d];
    boxes[6 * t + d] = fminf(a[d], fminf(b[d], c[d]));
    boxes[6 * t + 3 + d] = fmaxf(a[d], fmaxf(b[d], c[d]));
  }
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
  const float n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
  const float nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  const float lab = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], lac = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
  if (!(nn > TRI_DEGENERATE * lab * lac)) {
    atomicAdd(stats + MESH_ZERO_AREA, 1);
#pragma unroll
    for (int d = 0; d < 3; ++d) faceN[3 * t + d] = angles[3 * t + d] = 0.f;
    return;
  }
  const float len = sqrtf(nn);
#pragma unroll
  for (int d = 0; d < 3; ++d) faceN[3 * t + d] = n[d] / len;
  angles[3 * t] = atan2f(len, ab[0] * ac[0] + ab[1] * ac[1] + ab[2] * ac[2]);
  angles[3 * t + 1] = atan2f(len, -(ab[0] * bc[0] + ab[1] * bc[1] + ab[2] * bc[2]));
  angles[3 * t + 2] = atan2f(len, ac[0] * bc[0] + ac[1] * bc[1] + ac[2] * bc[2]);
}

__global__ __launch_bounds__(256) void mesh_keys_kernel(const int *tris, size_t n3, unsigned long long *heKeys, unsigned *cornerKeys, int *vals) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  const size_t t = i / 3;
  const int e = (int)(i % 3);
  const unsigned u = (unsigned)tris[i], v = (unsigned)tris[3 * t + (e + 1) % 3];
  heKeys[i] = ((unsigned long long)(u < v ? u : v) << 32) | (u < v ? v : u);
  cornerKeys[i] = u;
  vals[i] = (int)i;
}

// one thread per run of equal half-edge keys: the edge pseudonormal = sum of the run's face normals, in sorted order (the sort is stable:
// by triangle number)
__global__ __launch_bounds__(256) void mesh_edge_kernel(const unsigned long long *keys, const int *vals, size_t n3, const int *tris,
                                                        const float *faceN, float *edgeN, int *stats, int countTopology) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  const unsigned long long k = keys[i];
  if (i > 0 && keys[i - 1] == k) return;
  size_t e = i + 1;
  while (e < n3 && keys[e] == k) ++e;
  float s[3] = {0.f, 0.f, 0.f};
  for (size_t j = i; j < e; ++j) {
    const int t = vals[j] / 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] += faceN[3 * t + d];
  }
  for (size_t j = i; j < e; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d) edgeN[3 * (size_t)vals[j] + d] = s[d];
  if (!countTopology) return;
  const size_t m = e - i;
  if (m == 1) atomicAdd(stats + MESH_BOUNDARY, 1);
  else if (m > 2) atomicAdd(stats + MESH_NONMANIFOLD, 1);
  else if ((unsigned)(k >> 32) != (unsigned)k) {  // two faces: they must run along the edge in opposite directions
    const int h0 = vals[i], h1 = vals[i + 1];
    const bool f0 = tris[h0] < tris[h0 / 3 * 3 + (h0 % 3 + 1) % 3], f1 = tris[h1] < tris[h1 / 3 * 3 + (h1 % 3 + 1) % 3];
    if (f0 == f1) atomicAdd(stats + MESH_INCONSISTENT, 1);
  }
}

// one thread per run of equal corner keys: the vertex pseudonormal = sum of angle x face normal over the run, in sorted order
__global__ __launch_bounds__(256) void mesh_vertex_kernel(const unsigned *keys, const int *vals, size_t n3, const float *faceN, const float *angles,
                                                          float *vertN) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  const unsigned k = keys[i];
  if (i > 0 && keys[i - 1] == k) return;
  float s[3] = {0.f, 0.f, 0.f};
  for (size_t j = i; j < n3 && keys[j] == k; ++j) {
    const int t = vals[j] / 3;
    const float w = angles[vals[j]];
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] += w * faceN[3 * t + d];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) vertN[3 * (size_t)k + d] = s[d];
}

__device__ __forceinline__ unsigned mesh_expand_bits(unsigned v) {  // math/bit/Bits.h:84-90
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}
// 30-bit Morton code of a point inside the root box (an ordering only)
__global__ __launch_bounds__(256) void mesh_point_code_kernel(const AABB3 *root, const float *pts, int nq, unsigned *codes, int *ids) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const AABB3 r = *root;
  unsigned code = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float len = r.hi[d] - r.lo[d];
    float u = len > 0.f ? (pts[3 * (size_t)i + d] - r.lo[d]) / len : 0.f;
    u = u > 0.f ? (u > 0.999999f ? 0.999999f : u) : 0.f;  // (NaN -> 0)
    code |= mesh_expand_bits((unsigned)(u * 1024.f)) << (2 - d);
  }
  codes[i] = code;
  ids[i] = i;
}

__global__ __launch_bounds__(256) void mesh_query_kernel(TriMeshDev m, const float *pts, size_t nq, float cap, const int *perm, float *dist,
                                                         int *tri, int *feature, float *bary, float *sdf, float *vel) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nq) return;
  const size_t i = perm ? (size_t)perm[k] : k;
  const float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  const MeshClosest r = m.closest_point(p, cap);
  if (dist) dist[i] = r.dist;
  if (tri) tri[i] = r.tri;
  if (feature) feature[i] = r.feature;
  if (bary) { bary[3 * i] = r.bary[0]; bary[3 * i + 1] = r.bary[1]; bary[3 * i + 2] = r.bary[2]; }
  if (sdf) sdf[i] = r.tri < 0 ? cap : m.sign_of(p, r) * r.dist;
  if (vel) {
    float v[3];
    m.velocity_of(r, v);
    vel[3 * i] = v[0]; vel[3 * i + 1] = v[1]; vel[3 * i + 2] = v[2];
  }
}

// ---------------------------------------------------------------------------------------------------------------- mesh -> level set
struct MeshLsFrame {
  float o[3], voxel, band;
};
// the blocks under a triangle's box dilated by band (+ one cell for the rounding of the index arithmetic)
__device__ __forceinline__ unsigned mesh_ls_block_range(const float *box, const MeshLsFrame &f, int (&blo)[3], int (&bn)[3]) {
  unsigned long long cnt = 1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    float lo = floorf((box[d] - f.o[d] - f.band) / f.voxel) - 1.f, hi = ceilf((box[3 + d] - f.o[d] + f.band) / f.voxel) + 1.f;
    if (!(lo > -1e9f && hi < 1e9f)) return 0xffffffffu;  // (also NaN)
    blo[d] = (int)lo >> 3;
    bn[d] = ((int)hi >> 3) - blo[d] + 1;
    cnt *= (unsigned long long)bn[d];
    if (cnt > MESH_LS_MAX_PER_TRI) return 0xffffffffu;
  }
  return (unsigned)cnt;
}
__global__ __launch_bounds__(256) void mesh_ls_count_kernel(const float *boxes, int nt, MeshLsFrame f, unsigned *counts, int *fail,
                                                            unsigned long long *sum) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned c = 0;
  if (t < nt) {
    int blo[3], bn[3];
    c = mesh_ls_block_range(boxes + 6 * (size_t)t, f, blo, bn);
    if (c == 0xffffffffu) {
      *fail = 1;
      c = 0;
    }
    counts[t] = c;
  }
  unsigned long long w = c;  // the 64-bit total (the scan below is 32-bit): one atomic per wave
#pragma unroll
  for (int d = 32; d; d >>= 1) w += shfl_down(w, d);
  if (lane_id() == 0 && w) atomicAdd(sum, w);
}
// one thread per (triangle, block) pair; offsets = exclusive scan of the counts
__global__ __launch_bounds__(256) void mesh_ls_insert_kernel(const float *boxes, int nt, MeshLsFrame f, const unsigned *offsets, unsigned total,
                                                             BhtDev tab) {
  __shared__ unsigned smem[2 + 256 / 64];
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = j < total;
  int key[3] = {0, 0, 0};
  if (valid) {
    int lo = 0, hi = nt - 1;  // the last triangle with offsets[t] <= j
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (offsets[mid] <= j) lo = mid;
      else hi = mid - 1;
    }
    int blo[3], bn[3];
    mesh_ls_block_range(boxes + 6 * (size_t)lo, f, blo, bn);
    const int r = (int)(j - offsets[lo]);
    key[0] = (blo[0] + r / (bn[1] * bn[2])) * MESH_LS_SIDE;
    key[1] = (blo[1] + r / bn[2] % bn[1]) * MESH_LS_SIDE;
    key[2] = (blo[2] + r % bn[2]) * MESH_LS_SIDE;
  }
  bht_insert_block<3>(tab, key, valid, smem);
}

__device__ __forceinline__ float mesh_box_gap2(const AABB3 &a, const float (&lo)[3], const float (&hi)[3]) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float g = fmaxf(0.f, fmaxf(a.lo[d] - hi[d], lo[d] - a.hi[d]));
    s += g * g;
  }
  return s;
}

__global__ __launch_bounds__(MESH_LS_BLOCK) void mesh_ls_block_kernel(TriMeshDev m, const int *keys, MeshLsFrame f, float *tiles, int numChannels,
                                                                      int *keep, unsigned *stats) {
  __shared__ __attribute__((aligned(16))) float s_tri[MESH_STAGE_TRIS * MESH_STAGE_STRIDE];
  __shared__ int s_q[2][MESH_QUEUE];
  __shared__ int s_n[4];  // [0], [1] queue lengths, [2] triangles, [3] overflow
  __shared__ float s_dc;
  const int tid = (int)threadIdx.x;
  const size_t blk = blockIdx.x;
  const int key[3] = {keys[3 * blk], keys[3 * blk + 1], keys[3 * blk + 2]};
  const int cc[3] = {tid >> 6, (tid >> 3) & 7, tid & 7};
  float p[3], lo[3], hi[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    p[d] = f.o[d] + f.voxel * (float)(key[d] + cc[d]);
    lo[d] = f.o[d] + f.voxel * (float)key[d];
    hi[d] = f.o[d] + f.voxel * (float)(key[d] + MESH_LS_SIDE - 1);
  }
  const float half = 6.0621778f * f.voxel;                          // 3.5 sqrt(3)
  const float rmax = (f.band + 12.124356f * f.voxel) * 1.00001f;    // band + 7 sqrt(3) voxel
  if (tid == 0) {
    const float c[3] = {0.5f * (lo[0] + hi[0]), 0.5f * (lo[1] + hi[1]), 0.5f * (lo[2] + hi[2])};
    const int t = m.nearest_triangle(c, rmax + half);
    s_dc = t < 0 ? 3.402823466e+38f : m.finish(c, t, rmax + half).dist;
    s_n[0] = 1; s_n[1] = 0; s_n[2] = 0; s_n[3] = 0;
    s_q[0][0] = 0;
  }
  __syncthreads();
  const float dc = s_dc;
  if (dc - half > f.band + 1e-4f * (f.band + half)) {  // no cell within band (the margin covers the rounding of dc)
    if (tid == 0) {
      keep[blk] = 0;
      if (stats) atomicAdd(stats + 0, 1u);
    }
    return;
  }
  const float R = fminf(dc + half, rmax) * 1.00001f + 1e-30f, R2 = R * R;
  const int numNodes = m.bvh.numNodes;
  int *s_id = (int *)s_tri;
  if (numNodes <= 2) {  // the small-tree form: every node is a leaf, its number the primitive's
    if (tid < numNodes) s_id[tid * MESH_STAGE_STRIDE + 9] = tid;
    if (tid == 0) s_n[2] = numNodes;
    __syncthreads();
  } else {
    for (int cur = 0;; cur ^= 1) {
      // the round's length and the overflow flag are latched by every wave BEFORE any wave of this round can write either (the barrier
      // below), so the exit decision is the same on every wave and all of them take the same barriers
      const int n = s_n[cur], over = s_n[3];
      __syncthreads();
      if (n == 0 || over) break;
      for (int i = tid; i < n; i += MESH_LS_BLOCK) {
        const int node = s_q[cur][i];
        if (mesh_box_gap2(m.bvh.orderedBvs[node], lo, hi) > R2) continue;
        if (m.bvh.levels[node] == 0) {
          const int slot = atomicAdd(&s_n[2], 1);
          if (slot < MESH_STAGE_TRIS) s_id[slot * MESH_STAGE_STRIDE + 9] = m.bvh.auxIndices[node];
          else s_n[3] = 1;
        } else {
          const int left = node + 1, right = m.bvh.levels[left] == 0 ? node + 2 : m.bvh.auxIndices[left];
          const int slot = atomicAdd(&s_n[cur ^ 1], 2);
          if (slot + 2 <= MESH_QUEUE) {
            s_q[cur ^ 1][slot] = left;
            s_q[cur ^ 1][slot + 1] = right;
          } else
            s_n[3] = 1;
        }
      }
      __syncthreads();
      if (tid == 0) s_n[cur] = 0;  // the queue after next: written before the next round's barrier, pushed to only after it
    }
  }
  const bool staged = s_n[3] == 0;
  int best = -1;
  if (staged) {
    const int ntri = s_n[2];
    for (int i = tid; i < ntri; i += MESH_LS_BLOCK) {
      float a[3], b[3], c[3];
      m.triangle(s_id[i * MESH_STAGE_STRIDE + 9], a, b, c);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        s_tri[i * MESH_STAGE_STRIDE + d] = a[d];
        s_tri[i * MESH_STAGE_STRIDE + 3 + d] = b[d];
        s_tri[i * MESH_STAGE_STRIDE + 6 + d] = c[d];
      }
    }
    __syncthreads();
    float best2 = 3.402823466e+38f;
    for (int i = 0; i < ntri; ++i) {
      const float *s = s_tri + i * MESH_STAGE_STRIDE;
      const float a[3] = {s[0], s[1], s[2]}, b[3] = {s[3], s[4], s[5]}, c[3] = {s[6], s[7], s[8]};
      const int id = s_id[i * MESH_STAGE_STRIDE + 9];
      const float d2 = tri_closest(p, a, b, c).dist2;
      if (d2 < best2 || (d2 == best2 && id < best)) {
        best2 = d2;
        best = id;
      }
    }
  } else
    best = m.nearest_triangle(p, rmax);
  const MeshClosest r = m.finish(p, best, rmax);
  const float sdf = r.tri < 0 ? rmax : m.sign_of(p, r) * r.dist;
  float *tile = tiles + blk * (size_t)numChannels * MESH_LS_BLOCK;
  tile[tid] = sdf;
  if (numChannels == 4) {
    float v[3];
    m.velocity_of(r, v);
#pragma unroll
    for (int d = 0; d < 3; ++d) tile[(1 + d) * MESH_LS_BLOCK + tid] = v[d];
  }
  const int kept = __syncthreads_or(fabsf(sdf) < f.band);
  if (tid == 0) {
    keep[blk] = kept ? 1 : 0;
    if (stats) {
      atomicAdd(stats + (staged ? 1 : 2), 1u);
      if (kept) atomicAdd(stats + 3, 1u);
    }
  }
}

__global__ __launch_bounds__(256) void mesh_ls_flags_kernel(const int *keep, size_t n, unsigned *flags) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] = keep[i] ? 1u : 0u;
}
__global__ __launch_bounds__(256) void mesh_ls_compact_kernel(const int *keys, const unsigned *flags, const unsigned *offsets, size_t n, int *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flags[i]) return;
#pragma unroll
  for (int d = 0; d < 3; ++d) out[3 * (size_t)offsets[i] + d] = keys[3 * i + d];
}
__global__ __launch_bounds__(256) void mesh_ls_gather_kernel(const int *keys, const int *keep, const float *src, BhtDev table, unsigned maxBlocks,
                                                             float *dst, int numChannels) {
  __shared__ int s_bno;
  const size_t blk = blockIdx.x;
  if (!keep[blk]) return;
  if (threadIdx.x == 0) {
    const int key[3] = {keys[3 * blk], keys[3 * blk + 1], keys[3 * blk + 2]};
    s_bno = bht_query<3>(table, key);
  }
  __syncthreads();
  const int bno = s_bno;
  if (bno < 0 || (unsigned)bno >= maxBlocks) return;
  const int n = numChannels * MESH_LS_BLOCK;
  for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) dst[(size_t)bno * n + i] = src[blk * (size_t)n + i];
}

// face normals, boxes and angles from the current vertices
static void mesh_faces(Launch &L, zs_rocm_mesh &m) {
  ZSR_CHECK(hipMemsetAsync(m.stats, 0, sizeof(int) * 4, L.stream));  // [4] (indices out of range) is a property of the topology
  if (m.nt)
    hipLaunchKernelGGL(mesh_face_kernel, dim3(ceil_div(m.nt, 256)), dim3(256), 0, L.stream, m.verts, m.tris, (int)m.nt, m.boxes, m.faceN, m.angles,
                       m.stats);
}
static void mesh_pseudonormals(Launch &L, zs_rocm_mesh &m) {
  ZSR_CHECK(hipMemsetAsync(m.vertN, 0, sizeof(float) * 3 * (m.nv ? m.nv : 1), L.stream));
  if (!m.nt) return;
  const size_t n3 = 3 * m.nt;
  hipLaunchKernelGGL(mesh_edge_kernel, dim3(ceil_div(n3, 256)), dim3(256), 0, L.stream, m.heKeys, m.heVals, n3, m.tris, m.faceN, m.edgeN, m.stats, 1);
  hipLaunchKernelGGL(mesh_vertex_kernel, dim3(ceil_div(n3, 256)), dim3(256), 0, L.stream, m.cornerKeys, m.cornerVals, n3, m.faceN, m.angles, m.vertN);
}

static bool mesh_ok(const zs_rocm_mesh *m) { return m && m->bvh && m->stats; }

// the unique edges from the sorted half-edge keys: the first key of every run, keys with min == max dropped; lexicographic order
__global__ __launch_bounds__(256) void mesh_edge_flags_kernel(const unsigned long long *keys, size_t n3, unsigned *flags) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n3) return;
  unsigned f = 0;
  if (i < n3) {
    const unsigned long long k = keys[i];
    f = (i == 0 || keys[i - 1] != k) && (unsigned)(k >> 32) != (unsigned)k ? 1u : 0u;
  }
  flags[i] = f;  // (flags[n3] = 0: the scan's last entry is the number of edges)
}
__global__ __launch_bounds__(256) void mesh_edge_compact_kernel(const unsigned long long *keys, size_t n3, const unsigned *flags,
                                                                const unsigned *offsets, int *edges) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3 || !flags[i]) return;
  const unsigned long long k = keys[i];
  edges[2 * (size_t)offsets[i]] = (int)(unsigned)(k >> 32);
  edges[2 * (size_t)offsets[i] + 1] = (int)(unsigned)k;
}
static void mesh_edges(Launch &L, zs_rocm_mesh &m) {
  const size_t n3 = 3 * m.nt;
  unsigned *flags = (unsigned *)L.temp(sizeof(unsigned) * (n3 + 1)), *offsets = (unsigned *)L.temp(sizeof(unsigned) * (n3 + 1));
  hipLaunchKernelGGL(mesh_edge_flags_kernel, dim3(ceil_div(n3 + 1, 256)), dim3(256), 0, L.stream, m.heKeys, n3, flags);
  exclusive_scan_u32(L, flags, n3 + 1, offsets);
  unsigned ne = 0;
  ZSR_CHECK(hipMemcpyAsync(&ne, offsets + n3, sizeof(unsigned), hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
  m.ne = ne;
  ZSR_CHECK(hipMalloc((void **)&m.edges, sizeof(int) * 2 * (ne ? ne : 1)));
  if (ne) hipLaunchKernelGGL(mesh_edge_compact_kernel, dim3(ceil_div(n3, 256)), dim3(256), 0, L.stream, m.heKeys, n3, flags, offsets, m.edges);
}


static MeshLsFrame ls_frame(const float *origin, float voxel, float band) {
  MeshLsFrame f;
  f.o[0] = origin[0]; f.o[1] = origin[1]; f.o[2] = origin[2];
  f.voxel = voxel;
  f.band = band;
  return f;
}
static bool ls_frame_ok(const float *origin, float voxel, float band) {
  return origin && voxel > 0.f && voxel <= 3.0e38f && band > 0.f && band <= 3.0e38f;
}
// counts and their exclusive scan (temporaries of L); returns the number of (triangle, block) pairs, (size_t)-1 if the lattice is too
// fine for the mesh (a triangle over more than 2^22 blocks, 2^31 pairs or more in all)
static size_t ls_pairs(Launch &L, const zs_rocm_mesh &m, const MeshLsFrame &f, unsigned **offsetsOut) {
  const size_t nt = m.nt;
  unsigned *counts = (unsigned *)L.temp(sizeof(unsigned) * nt), *offsets = (unsigned *)L.temp(sizeof(unsigned) * nt);
  int *fail = (int *)L.temp(sizeof(int));
  unsigned long long *sum = (unsigned long long *)L.temp(sizeof(unsigned long long));
  ZSR_CHECK(hipMemsetAsync(fail, 0, sizeof(int), L.stream));
  ZSR_CHECK(hipMemsetAsync(sum, 0, sizeof(unsigned long long), L.stream));
  hipLaunchKernelGGL(mesh_ls_count_kernel, dim3(ceil_div(nt, 256)), dim3(256), 0, L.stream, m.boxes, (int)nt, f, counts, fail, sum);
  exclusive_scan_u32(L, counts, nt, offsets);  // (meaningful only when the total below fits)
  unsigned long long total = 0;
  int failed = 0;
  ZSR_CHECK(hipMemcpyAsync(&total, sum, sizeof(total), hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipMemcpyAsync(&failed, fail, sizeof(int), hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
  if (offsetsOut) *offsetsOut = offsets;
  if (failed || total >= 0x80000000ull) return (size_t)-1;
  return (size_t)total;
}

}  // namespace zsr

using namespace zsr;

extern "C" {

zs_rocm_mesh *zs_rocm_mesh_create(zs_rocm_policy *pol, const float *verts, size_t nv, const int *tris, size_t nt, const float *vel) {
  if (!pol || (nv && !verts) || (nt && (!tris || !nv)) || nv > 0x7fffffffu || nt > 0x7fffffffu / 3) return nullptr;
  zs_rocm_mesh *m = new zs_rocm_mesh;
  m->nv = nv;
  m->nt = nt;
  m->hasVel = vel != nullptr;
  m->bvh = zs_rocm_lbvh_create();
  const size_t nv1 = nv ? nv : 1, nt1 = nt ? nt : 1;
  {
    Launch L(pol, "mesh_create (faces)");
    ZSR_CHECK(hipMalloc((void **)&m->verts, sizeof(float) * 3 * nv1));
    ZSR_CHECK(hipMalloc((void **)&m->vel, sizeof(float) * 3 * nv1));
    ZSR_CHECK(hipMalloc((void **)&m->vertN, sizeof(float) * 3 * nv1));
    ZSR_CHECK(hipMalloc((void **)&m->tris, sizeof(int) * 3 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->faceN, sizeof(float) * 3 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->angles, sizeof(float) * 3 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->edgeN, sizeof(float) * 9 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->boxes, sizeof(float) * 6 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->heKeys, sizeof(unsigned long long) * 3 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->heVals, sizeof(int) * 3 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->cornerKeys, sizeof(unsigned) * 3 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->cornerVals, sizeof(int) * 3 * nt1));
    ZSR_CHECK(hipMalloc((void **)&m->stats, sizeof(int) * ZS_ROCM_MESH_STAT_WORDS));
    ZSR_CHECK(hipMemsetAsync(m->stats, 0, sizeof(int) * ZS_ROCM_MESH_STAT_WORDS, L.stream));
    if (nv) ZSR_CHECK(hipMemcpyAsync(m->verts, verts, sizeof(float) * 3 * nv, hipMemcpyDeviceToDevice, L.stream));
    if (nv && vel) ZSR_CHECK(hipMemcpyAsync(m->vel, vel, sizeof(float) * 3 * nv, hipMemcpyDeviceToDevice, L.stream));
    if (nt) hipLaunchKernelGGL(mesh_copy_tris_kernel, dim3(ceil_div(3 * nt, 256)), dim3(256), 0, L.stream, tris, 3 * nt, (int)nv, m->tris, m->stats);
    mesh_faces(L, *m);
  }
  if (nt) zs_rocm_lbvh_build(pol, m->bvh, m->boxes, nt, 1);
  {
    Launch L(pol, "mesh_create (adjacency)");
    if (nt) {
      const size_t n3 = 3 * nt;
      unsigned long long *hk = (unsigned long long *)L.temp(sizeof(unsigned long long) * n3);
      unsigned *ck = (unsigned *)L.temp(sizeof(unsigned) * n3);
      int *ids = (int *)L.temp(sizeof(int) * n3);
      hipLaunchKernelGGL(mesh_keys_kernel, dim3(ceil_div(n3, 256)), dim3(256), 0, L.stream, m->tris, n3, hk, ck, ids);
      const int vb = key_bits(nv);
      radix_sort_pair_u64(L, hk, ids, m->heKeys, m->heVals, n3, 0, 32 + vb);
      radix_sort_pair_u32(L, ck, ids, m->cornerKeys, m->cornerVals, n3, 0, vb);
      mesh_edges(L, *m);
    }
    mesh_pseudonormals(L, *m);
  }
  return m;
}

void zs_rocm_mesh_destroy(zs_rocm_mesh *m) {
  if (!m) return;
  (void)hipFree(m->verts); (void)hipFree(m->vel); (void)hipFree(m->vertN); (void)hipFree(m->tris); (void)hipFree(m->faceN);
  (void)hipFree(m->angles); (void)hipFree(m->edgeN); (void)hipFree(m->boxes); (void)hipFree(m->heKeys); (void)hipFree(m->heVals);
  (void)hipFree(m->cornerKeys); (void)hipFree(m->cornerVals); (void)hipFree(m->stats);
  (void)hipFree(m->edges); (void)hipFree(m->edgeBoxes); (void)hipFree(m->triPacked); (void)hipFree(m->edgePacked);
  (void)hipFree(m->ptCache); (void)hipFree(m->ptCacheCounts); (void)hipFree(m->eeCache); (void)hipFree(m->eeCacheCounts);
  (void)hipFree(m->restLen2);
  (void)hipFree(m->hinges); (void)hipFree(m->hingeStarts); (void)hipFree(m->hingeEntries); (void)hipFree(m->cornerStarts);
  (void)hipFree(m->triRecord); (void)hipFree(m->hingeRecord); (void)hipFree(m->vertArea);
  zs_rocm_lbvh_destroy(m->bvh);
  if (m->edgeBvh) zs_rocm_lbvh_destroy(m->edgeBvh);
  delete m;
}

int zs_rocm_mesh_refit(zs_rocm_policy *pol, zs_rocm_mesh *m, const float *verts, const float *vel) {
  if (!pol || !mesh_ok(m) || (m->nv && !verts)) return -1;
  {
    Launch L(pol, "mesh_refit (faces)");
    if (m->nv) ZSR_CHECK(hipMemcpyAsync(m->verts, verts, sizeof(float) * 3 * m->nv, hipMemcpyDeviceToDevice, L.stream));
    if (m->nv && vel) {
      ZSR_CHECK(hipMemcpyAsync(m->vel, vel, sizeof(float) * 3 * m->nv, hipMemcpyDeviceToDevice, L.stream));
      m->hasVel = true;
    }
    mesh_faces(L, *m);
  }
  if (m->nt && zs_rocm_lbvh_refit(pol, m->bvh, m->boxes, m->nt) != 0) return -1;
  if (mesh_proximity_refit(pol, *m) != 0) return -1;
  Launch L(pol, "mesh_refit (pseudonormals)");
  mesh_pseudonormals(L, *m);
  return 0;
}

void zs_rocm_mesh_stats(zs_rocm_policy *pol, const zs_rocm_mesh *m, int *out) {
  if (!pol || !mesh_ok(m) || !out) return;
  Launch L(pol, "mesh_stats");
  ZSR_CHECK(hipMemcpyAsync(out, m->stats, sizeof(int) * ZS_ROCM_MESH_STAT_WORDS, hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
}

int zs_rocm_mesh_total_box(zs_rocm_policy *pol, const zs_rocm_mesh *m, float *box6) {
  if (!pol || !mesh_ok(m) || !box6 || !m->nt) return -1;
  float *dev = (float *)zs_rocm_policy_temporary(pol, sizeof(float) * 6);
  zs_rocm_lbvh_total_box(pol, m->bvh, dev);
  {
    Launch L(pol, "mesh_total_box");
    ZSR_CHECK(hipMemcpyAsync(box6, dev, sizeof(float) * 6, hipMemcpyDeviceToHost, L.stream));
    ZSR_CHECK(hipStreamSynchronize(L.stream));
  }
  zs_rocm_policy_temporary_free(pol, dev);
  return 0;
}

void zs_rocm_mesh_get_view(const zs_rocm_mesh *m, zs_rocm_mesh_view *v) {
  if (!v) return;
  if (!mesh_ok(m)) {
    *v = zs_rocm_mesh_view{};
    return;
  }
  v->verts = m->verts; v->tris = m->tris; v->vel = m->hasVel ? m->vel : nullptr;
  v->faceNormals = m->faceN; v->vertNormals = m->vertN; v->edgeNormals = m->edgeN;
  zs_rocm_lbvh_get_view(m->bvh, &v->bvh);
  v->numVerts = (int)m->nv; v->numTris = (int)m->nt;
}

static int mesh_query(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *points, size_t nq, float cap, float *dist, int *tri, int *feature,
                      float *bary, float *sdf, float *vel, const char *what) {
  if (!pol || !mesh_ok(m) || (nq && !points) || !(cap >= 0.f) || nq > 0x7fffffffu) return -1;
  Launch L(pol, what);
  if (!nq) return 0;
  const TriMeshDev d = m->dev();
  const int *perm = nullptr;
  if (nq >= 16384 && d.bvh.numNodes > 2) {  // Morton order of the points inside the root box, as lbvh_query_order
    unsigned *codes = (unsigned *)L.temp(sizeof(unsigned) * nq), *sorted = (unsigned *)L.temp(sizeof(unsigned) * nq);
    int *ids = (int *)L.temp(sizeof(int) * nq), *p = (int *)L.temp(sizeof(int) * nq);
    hipLaunchKernelGGL(mesh_point_code_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, L.stream, d.bvh.orderedBvs, points, (int)nq, codes, ids);
    radix_sort_pair_u32(L, codes, ids, sorted, p, nq, 0, 30);
    perm = p;
  }
  hipLaunchKernelGGL(mesh_query_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, L.stream, d, points, nq, cap, perm, dist, tri, feature, bary, sdf, vel);
  return 0;
}
int zs_rocm_mesh_closest_point(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *points, size_t nq, float cap, float *dist, int *tri,
                               int *feature, float *bary) {
  return mesh_query(pol, m, points, nq, cap, dist, tri, feature, bary, nullptr, nullptr, "LBvhView::find_nearest (triangles)");
}
int zs_rocm_mesh_signed_distance(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *points, size_t nq, float cap, float *sdf, float *vel) {
  return mesh_query(pol, m, points, nq, cap, nullptr, nullptr, nullptr, nullptr, sdf, vel, "mesh signed distance");
}

size_t zs_rocm_mesh_levelset_count(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *origin, float voxel, float band) {
  if (!pol || !mesh_ok(m) || !ls_frame_ok(origin, voxel, band)) return (size_t)-1;
  if (!m->nt) return 0;
  Launch L(pol, "mesh_levelset_count");
  return ls_pairs(L, *m, ls_frame(origin, voxel, band), nullptr);
}

int zs_rocm_mesh_levelset_candidates(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *origin, float voxel, float band,
                                     zs_rocm_bht_3 *cand) {
  if (!pol || !mesh_ok(m) || !ls_frame_ok(origin, voxel, band) || !cand || cand->t.dim != 3) return -1;
  if (!m->nt) return 0;
  Launch L(pol, "mesh_levelset_candidates");
  const MeshLsFrame f = ls_frame(origin, voxel, band);
  unsigned *offsets = nullptr;
  const size_t total = ls_pairs(L, *m, f, &offsets);
  if (total == (size_t)-1) return -1;
  if (total)
    hipLaunchKernelGGL(mesh_ls_insert_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, L.stream, m->boxes, (int)m->nt, f, offsets, (unsigned)total,
                       cand->t.dev());
  return 0;
}

int zs_rocm_mesh_levelset_blocks(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *origin, float voxel, float band, const zs_rocm_bht_3 *cand,
                                 size_t ncand, float *tiles, int numChannels, int *keep, unsigned *stats) {
  if (!pol || !mesh_ok(m) || !ls_frame_ok(origin, voxel, band) || !cand || cand->t.dim != 3 || ncand > cand->t.tableSize) return -1;
  if ((numChannels != 1 && numChannels != 4) || (ncand && (!tiles || !keep)) || ncand > 0x7fffffffu) return -1;
  Launch L(pol, "mesh_levelset_blocks");
  if (!ncand) return 0;
  hipLaunchKernelGGL(mesh_ls_block_kernel, dim3((unsigned)ncand), dim3(MESH_LS_BLOCK), 0, L.stream, m->dev(), (const int *)cand->t.activeKeys,
                     ls_frame(origin, voxel, band), tiles, numChannels, keep, stats);
  return 0;
}

size_t zs_rocm_mesh_levelset_select(zs_rocm_policy *pol, const zs_rocm_bht_3 *cand, size_t ncand, const int *keep, int *keptKeys) {
  if (!pol || !cand || cand->t.dim != 3 || ncand > cand->t.tableSize || (ncand && (!keep || !keptKeys))) return (size_t)-1;
  if (!ncand) return 0;
  Launch L(pol, "mesh_levelset_select");
  unsigned *flags = (unsigned *)L.temp(sizeof(unsigned) * (ncand + 1)), *offsets = (unsigned *)L.temp(sizeof(unsigned) * (ncand + 1));
  ZSR_CHECK(hipMemsetAsync(flags + ncand, 0, sizeof(unsigned), L.stream));
  hipLaunchKernelGGL(mesh_ls_flags_kernel, dim3(ceil_div(ncand, 256)), dim3(256), 0, L.stream, keep, ncand, flags);
  exclusive_scan_u32(L, flags, ncand + 1, offsets);
  hipLaunchKernelGGL(mesh_ls_compact_kernel, dim3(ceil_div(ncand, 256)), dim3(256), 0, L.stream, (const int *)cand->t.activeKeys, flags, offsets, ncand,
                     keptKeys);
  unsigned total = 0;
  ZSR_CHECK(hipMemcpyAsync(&total, offsets + ncand, sizeof(unsigned), hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
  return total;
}

int zs_rocm_mesh_levelset_gather(zs_rocm_policy *pol, const zs_rocm_bht_3 *cand, size_t ncand, const int *keep, const float *tiles,
                                 const zs_rocm_bht_3 *table, float *dstTiles, int numChannels) {
  if (!pol || !cand || !table || cand->t.dim != 3 || table->t.dim != 3 || ncand > cand->t.tableSize || ncand > 0x7fffffffu) return -1;
  if ((numChannels != 1 && numChannels != 4) || (ncand && (!keep || !tiles || !dstTiles))) return -1;
  Launch L(pol, "mesh_levelset_gather");
  if (!ncand) return 0;
  const unsigned maxBlocks = (unsigned)bht_size(table->t, L.stream);
  hipLaunchKernelGGL(mesh_ls_gather_kernel, dim3((unsigned)ncand), dim3(256), 0, L.stream, (const int *)cand->t.activeKeys, keep, tiles, table->t.dev(),
                     maxBlocks, dstTiles, numChannels);
  return 0;
}

}  // extern "C"
