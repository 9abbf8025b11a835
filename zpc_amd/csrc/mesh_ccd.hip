// mesh_ccd.hip -- the largest step along a direction that keeps the pairs of a proximity list free of contact, for gfx950: additive CCD per
// pair (include/zensim_rocm/ccd_device.hpp has the math and the float32 limits) over the PT and EE lists of mesh_proximity.hip, at the
// mesh's own or at trial positions, and the minimum over all pairs.  Bit-reproducible: no float atomics, and a pair's answer is a pure
// function of its eight rows, whichever lane and round computes it.
//
//   phase 1   lane = pair.  pair_corners resolves the four vertices (indices outside the mesh: the pair is inactive and gets tMax), the
//             lane gathers positions and directions and runs ccd_start: finiteness, the bound l_p on the relative speed, the distance at
//             t = 0, the first increment.  Most pairs of a candidate list end here (nothing moves relatively, or the first increment
//             already reaches tMax) and write their answer.
//   phase 2   the survivors of the workgroup are compacted through a ballot into an LDS queue of CcdRecord (pair number and the CcdState
//             between two evaluations: 24 bytes; the corners are gathered again from the pair number).  Lane k of the workgroup takes
//             queue entry k and runs up to CCD_ROUND evaluations of ccd_step; pairs that finish write their answer, the rest are
//             compacted again.  So the waves that still run are dense, a wave without work only passes the barriers, and the long tail of
//             a few slowly closing pairs occupies one wave, not four.  The loop ends when the queue is empty.
//   minimum   every lane keeps the smallest answer it wrote; one wave-level minimum and at most one integer atomicMin per wave on the bit
//             pattern (the answers are non-negative floats: the order of their bits is their order) against a word initialised to the
//             bits of tMax; a wave that cannot lower the word skips it.  A minimum has no order, so the word is the same on every call.
//   status    four integer counters: pairs at zero distance PT, EE, pairs stopped by maxIter PT, EE.
// Built with -ffp-contract=off (zpc_amd/build.py), as every translation unit behind tri_closest / ee_closest.
#include <cfloat>

#include "mesh.hpp"
#include "../../include/zensim_rocm/ccd_device.hpp"

namespace zsr {

constexpr int CCD_BLOCK = 256, CCD_WAVES = CCD_BLOCK / 64;
constexpr int CCD_ROUND = 4;  // evaluations between two compactions (profiles/mesh_ccd.md)

// one pair list of one kind and what the kernel reads and writes for it
struct CcdPairs {
  const float *verts, *dir;  // [nv][3] positions and direction
  const int *prims;          // tris [np][3] (PT) or edges [np][2] (EE)
  int nv, np;
  const int *pairs;  // [n][2]
  int n;
  float slack, tMax;
  int maxIter;
  float *toi;      // [n] or null
  unsigned *tMin;  // the bits of the running minimum
  int *status;     // [4]
};

struct CcdRecord {
  int pair;
  CcdState s;
};

template <bool EE>
__device__ __forceinline__ void ccd_finish(const CcdPairs &a, const CcdRecord &r, int status, float &best) {
  if (a.toi) a.toi[r.pair] = r.s.t;
  best = fminf(best, r.s.t);
  if (status == CCD_ZERO) atomicAdd(a.status + EE, 1);
  if (status == CCD_CAPPED) atomicAdd(a.status + 2 + EE, 1);
}

template <bool EE>
__global__ __launch_bounds__(CCD_BLOCK) void ccd_kernel(const CcdPairs a) {
  __shared__ CcdRecord queue[CCD_BLOCK];
  __shared__ int waveLive[CCD_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float best = a.tMax;
  CcdRecord r;
  bool live = false;
  {
    const int i = blockIdx.x * CCD_BLOCK + tid;
    if (i < a.n) {
      int idx[4], status = CCD_OK;
      r.pair = i;
      r.s.t = a.tMax;
      if (pair_corners<EE>(a.pairs, a.prims, a.nv, a.np, i, idx)) {
        float x[4][3], p[4][3];
        vertex_rows<4>(a.verts, idx, x);
        vertex_rows<4>(a.dir, idx, p);
        live = !ccd_start<EE>(x, p, a.slack, a.tMax, r.s, status);
      }
      if (!live) ccd_finish<EE>(a, r, status, best);
    }
  }
  for (;;) {
    const unsigned long long b = __ballot(live);
    if (lane == 0) waveLive[wave] = __popcll(b);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < CCD_WAVES; ++w) {
      const int c = waveLive[w];
      base += w < wave ? c : 0;
      total += c;
    }
    if (total == 0) break;  // the same for every lane of the workgroup
    if (live) queue[base + __popcll(b & ((1ull << lane) - 1ull))] = r;  // base + rank < total <= CCD_BLOCK
    __syncthreads();
    live = tid < total;
    if (live) {
      r = queue[tid];
      int idx[4], status = CCD_OK;
      pair_corners<EE>(a.pairs, a.prims, a.nv, a.np, r.pair, idx);  // an active pair: it passed this test in phase 1
      float x[4][3], p[4][3];
      vertex_rows<4>(a.verts, idx, x);
      vertex_rows<4>(a.dir, idx, p);
      bool done = false;
#pragma unroll 1
      for (int k = 0; k < CCD_ROUND && !done; ++k) done = ccd_step<EE>(x, p, a.tMax, a.maxIter, r.s, status);
      if (done) {
        ccd_finish<EE>(a, r, status, best);
        live = false;
      }
    }
    __syncthreads();  // queue and waveLive are read; the next round overwrites them
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = fminf(best, __shfl_xor(best, o));
  // the word only falls, so a wave whose minimum is not below what it reads there (a value the word held at some time, never below its
  // final one) cannot change it: it skips the atomic.  3.3 M atomics on one address: 38.1 -> 9.1 ms on a 213 M-pair list
  if (lane == 0 && __float_as_uint(best) < __hip_atomic_load(a.tMin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMin(a.tMin, __float_as_uint(best));
}

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_mesh_ccd(zs_rocm_policy *pol, const zs_rocm_mesh *m, const float *verts, const float *dir, const int *ptPairs, size_t npt,
                     const int *eePairs, size_t nee, float slack, float tMax, int maxIter, float *ptToi, float *eeToi, float *tMin,
                     int *status) {
  if (!pol || !m || !m->stats || !dir || !tMin) return -1;
  if (!(slack > 0.f && slack < 1.f) || !(tMax > 0.f && tMax <= FLT_MAX) || maxIter < 1) return -1;
  if (!barrier_counts_ok(npt, nee) || (npt && !ptPairs) || (nee && !eePairs)) return -1;
  Launch L(pol, "mesh_ccd");
  int *st = status ? status : (int *)L.temp(sizeof(int) * 4);
  ZSR_CHECK(hipMemsetAsync(st, 0, sizeof(int) * 4, L.stream));
  ZSR_CHECK(hipMemsetD32Async((hipDeviceptr_t)tMin, (int)__builtin_bit_cast(unsigned, tMax), 1, L.stream));
  const CcdPairs pt = {verts ? verts : m->verts, dir, m->tris, (int)m->nv, (int)m->nt, ptPairs, (int)npt, slack, tMax, maxIter, ptToi,
                       (unsigned *)tMin, st};
  CcdPairs ee = pt;
  ee.prims = m->edges, ee.np = (int)m->ne, ee.pairs = eePairs, ee.n = (int)nee, ee.toi = eeToi;
  if (pt.n) hipLaunchKernelGGL((ccd_kernel<false>), dim3(ceil_div(pt.n, CCD_BLOCK)), dim3(CCD_BLOCK), 0, L.stream, pt);
  if (ee.n) hipLaunchKernelGGL((ccd_kernel<true>), dim3(ceil_div(ee.n, CCD_BLOCK)), dim3(CCD_BLOCK), 0, L.stream, ee);
  return 0;
}

}  // extern "C"
