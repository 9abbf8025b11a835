// mesh_solve.hip -- the linear system of one Newton iteration on a mesh for gfx950: A = diag(mass) + scale (H+_elastic + H+_barrier +
// H_friction) on [nv][3] float32 vectors, its 3 x 3 diagonal blocks, the operator in one gather, and a block-Jacobi preconditioned
// conjugate-gradient solve whose scalars never leave the device (include/zensim_rocm/solve_device.hpp has the block arithmetic; the terms
// are the products of mesh_elastic.hip and mesh_barrier.hip, launched here through mesh.hpp / mesh_pairs.hpp).  Bit-reproducible: no float
// atomics anywhere.
//
//   blocks    lane = triangle / hinge / pair.  The element's own corner block at corner c is, column j, the rows of corner c of the
//             product's own device function at the unit direction e_{c,j}: one call per (corner, column) in a loop, whose
//             position-dependent part (closest point, barrier derivatives, strain, tangent) does not depend on the direction.  The six
//             entries (i <= j) of every corner go to scratch once; an idle element writes zeros.  An element any of whose calls reports an
//             overflow / a zero distance is counted once.  (A degenerate element that has one vertex on two corners gets the two corners'
//             own blocks and not their cross terms.)  A gather with six accumulators per vertex sums the runs the products' gather sums:
//             triangle run then hinge run; the pair run.  A last kernel combines the three with scale and mass and inverts.
//   multiply  the element kernels of the three products write their [corners][3] terms to one scratch array (elastic, barrier, friction),
//             then solve_gather_kernel, lane = vertex, sums up to four runs into one accumulator triple: elastic triangle, elastic hinge,
//             barrier, friction; a run that is absent has a null pointer.  q = mass x + scale acc, zero at a fixed vertex.
//   dot       d = sum_v ((a0 b0 + a1 b1) + a2 b2), every product exact in float64 (24 x 24 bits), the three added left to right in float64;
//             workgroup g holds the vertices [256 g, 256 g + 256), thread t vertex 256 g + t (0.0 beyond nv and at a fixed vertex), an LDS
//             tree (h = 128, 64, .., 1: s[t] += s[t + h]) gives the partial of g; a single workgroup then has thread t add the partials
//             t, t + 256, .. front to back and runs the same tree.
//   solve     r = b - A x, z = D^-1 r, p = z, rz = r . z; res = (float) sqrt(rz), history[0] = res, localTol = min(relTol res, tol);
//             converged at once if res <= localTol, else maxIters == 0 ends with flag 2.  Iteration k:
//                 q = A p and the partials of p . q            (element kernels, solve_gather_kernel<true>)
//                 pq: not finite -> flag 4; not positive -> flag 3; else alpha = (float) (rz / pq)          (solve_scalar_kernel)
//                 x += alpha p, r -= alpha q, z = D^-1 r, the partials of r . z                             (solve_update_kernel)
//                 rz': not finite or negative -> flag 4; else beta = (float) (rz' / rz), rz = rz', iters = k + 1,
//                     res = (float) sqrt(rz'), history[k + 1] = res; res <= localTol -> flag 1, else iters == maxIters -> flag 2
//                 p = z + beta p                                                                             (solve_direction_kernel)
//             Every solver kernel reads the flag first and returns if it is set, so x, iters and the history are frozen from then on
//             whatever else is enqueued (the products' element kernels still run: they write scratch only).  The host enqueues
//             checkEvery iterations, copies the flag back and waits: ceil(iters / checkEvery) read-backs per solve and nothing else.
// Built with -ffp-contract=off (zpc_amd/build.py): tests/ref64_solve.py replays blocks, operator and solve operation by operation.
#include <cfloat>

#include "mesh_system.hpp"
#include "../../include/zensim_rocm/elastic_device.hpp"
#include "../../include/zensim_rocm/solve_device.hpp"

namespace zsr {

constexpr int SOLVE_BLOCK = TERM_BLOCK;
enum { SOLVE_RUNNING = 0, SOLVE_CONVERGED = 1, SOLVE_MAX_ITERS = 2, SOLVE_BREAKDOWN = 3, SOLVE_NOT_FINITE = 4 };
enum { SOLVE_STAGE_INIT, SOLVE_STAGE_ALPHA, SOLVE_STAGE_BETA };

// ---------------------------------------------------------------------------------------------------------------- element blocks
// column j of the corner block at corner c from the product's terms h at the unit direction e_{c,j}: entries (i, j), i <= j
template <int N>
__device__ __forceinline__ void block_store_column(float *out, int c, int j, const float (&h)[N][3]) {
  float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (k == c) r0 = h[k][0], r1 = h[k][1], r2 = h[k][2];
  float *o = out + 6 * c;
  if (j == 0) {
    o[0] = r0;
  } else if (j == 1) {
    o[1] = r0, o[3] = r1;
  } else {
    o[2] = r0, o[4] = r1, o[5] = r2;
  }
}
template <int N>
__device__ __forceinline__ void block_unit(float (&z)[N][3], int c, int j) {
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) z[k][d] = (k == c && d == j) ? 1.f : 0.f;
}
template <int N>
__device__ __forceinline__ void block_zero(float *out) {
#pragma unroll
  for (int k = 0; k < 6 * N; ++k) out[k] = 0.f;
}

struct BlockElems {
  const float *verts;
  const int *elems;  // tris [n][3] or hinges [n][4]
  int nv, n;
  const float *record;  // [n][4]
  float mu, lam, kb;
  float *blocks;  // [n][3 or 4][6]
  int *status;    // one overflow count
};

template <bool HINGE>
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_elem_block_kernel(const BlockElems a) {
  const int i = blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  constexpr int N = HINGE ? 4 : 3;
  float *out = a.blocks + 6 * N * (size_t)i;
  int idx[N];
  if (!elastic_indices<N>(a.elems, (size_t)i, a.nv, idx)) return block_zero<N>(out);
  const float4 r = reinterpret_cast<const float4 *>(a.record)[i];
  const float rec[4] = {r.x, r.y, r.z, r.w};
  [[maybe_unused]] float x[N][3];
  if constexpr (!HINGE) vertex_rows<N>(a.verts, idx, x);
  bool overflow = false;
#pragma unroll 1
  for (int cj = 0; cj < 3 * N; ++cj) {
    const int c = cj / 3, j = cj - 3 * c;
    float z[N][3], h[N][3];
    block_unit<N>(z, c, j);
    int status;
    if constexpr (HINGE)
      status = elastic_hinge_product(rec, z, a.kb, h);
    else
      status = elastic_tri_product<true>(rec, x, z, a.mu, a.lam, h);
    overflow = overflow || status == ELASTIC_OVERFLOW;
    block_store_column<N>(out, c, j, h);
  }
  if (overflow) atomicAdd(a.status, 1);
}

enum { BLOCK_PT, BLOCK_EE, BLOCK_FRICTION_PT, BLOCK_FRICTION_EE };

// a.contrib: the [n][4][6] blocks; a.verts: positions (barrier) or the displacement (friction)
template <int KIND>
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_pair_block_kernel(const BarrierPairs a) {
  const int i = blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  constexpr bool EE = KIND == BLOCK_EE || KIND == BLOCK_FRICTION_EE, FRICTION = KIND == BLOCK_FRICTION_PT || KIND == BLOCK_FRICTION_EE;
  float *out = a.contrib + 24 * (size_t)i;
  int idx[4];
  float eps;
  if (!barrier_corners<EE>(a, i, idx, eps)) return block_zero<4>(out);
  float p[4][3];
  vertex_rows<4>(a.verts, idx, p);
  [[maybe_unused]] FrictionRecord rec = friction_record_zero();
  if constexpr (FRICTION) rec = friction_load(a.record, (size_t)i);
  bool zero = false;
#pragma unroll 1
  for (int cj = 0; cj < 12; ++cj) {
    const int c = cj / 3, j = cj - 3 * c;
    float z[4][3], h[4][3];
    block_unit<4>(z, c, j);
    int status;
    if constexpr (FRICTION)
      status = friction_product(rec, p, z, a.mu, a.epsv, h);
    else if constexpr (EE)
      status = barrier_ee_hvp<true>(p[0], p[1], p[2], p[3], z, a.dHat2, a.kappa, eps, h);
    else
      status = barrier_pt_hvp<true>(p[0], p[1], p[2], p[3], z, a.dHat2, a.kappa, h);
    zero = zero || status == BARRIER_ZERO;
    block_store_column<4>(out, c, j, h);
  }
  if (zero) atomicAdd(a.status + EE, 1);
}

// the six-float rows of one run of vertex v, front to back
__device__ __forceinline__ void block_add_run(const int *__restrict__ starts, const int *__restrict__ entries, const float *__restrict__ blocks, int v,
                                              float (&s)[6]) {
  for (int i = starts[v]; i < starts[v + 1]; ++i) {
    const float *g = blocks + 6 * (size_t)entries[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += g[k];
  }
}
template <int NRUNS>
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_block_gather_kernel(const int *__restrict__ starts0, const int *__restrict__ entries0,
                                                                         const float *__restrict__ blocks0, const int *__restrict__ starts1,
                                                                         const int *__restrict__ entries1, const float *__restrict__ blocks1,
                                                                         int nv, float *__restrict__ out) {
  const int v = blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  if (v >= nv) return;
  float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  block_add_run(starts0, entries0, blocks0, v, s);
  if constexpr (NRUNS == 2) block_add_run(starts1, entries1, blocks1, v, s);
#pragma unroll
  for (int k = 0; k < 6; ++k) out[6 * (size_t)v + k] = s[k];
}

__device__ __forceinline__ bool solve_fixed(const float *__restrict__ mass, const unsigned char *__restrict__ fixed, int v) {
  return (fixed && fixed[v]) || !solve_mass_ok(mass[v]);
}

// status[0]: inverse fallbacks, status[1]: masses treated as fixed
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_block_combine_kernel(const float *__restrict__ el, const float *__restrict__ ba,
                                                                          const float *__restrict__ fr, const float *__restrict__ mass,
                                                                          const unsigned char *__restrict__ fixed, float scale, int nv,
                                                                          float *__restrict__ combined, float *__restrict__ inverse, int *status) {
  const int v = blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  if (v >= nv) return;
  float e[6], b[6], f[6], D[6], inv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 6; ++k) e[k] = el[6 * (size_t)v + k], b[k] = ba[6 * (size_t)v + k], f[k] = fr[6 * (size_t)v + k];
  const float m = mass[v];
  block_combine(e, b, f, scale, m, D);
  if (!solve_mass_ok(m)) atomicAdd(status + 1, 1);
  if (!solve_fixed(mass, fixed, v) && block_inverse(D, m, inv)) atomicAdd(status, 1);
#pragma unroll
  for (int k = 0; k < 6; ++k) combined[6 * (size_t)v + k] = D[k], inverse[6 * (size_t)v + k] = inv[k];
}

// ---------------------------------------------------------------------------------------------------------------- the device record
// what the solver kernels hand to each other; the caller's record (iters, flag, history) is separate
struct SolveState {
  double rz;
  float alpha, beta, localTol;
  int pad;
};

__device__ __forceinline__ double solve_block_sum(double s) {
  __shared__ double sm[SOLVE_BLOCK];
  sm[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int h = SOLVE_BLOCK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  return sm[0];
}
__device__ __forceinline__ double solve_dot3(const float (&a)[3], const float (&b)[3]) {
  return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
}
__device__ __forceinline__ void solve_load3(const float *__restrict__ a, int v, float (&o)[3]) {
  o[0] = a[3 * (size_t)v], o[1] = a[3 * (size_t)v + 1], o[2] = a[3 * (size_t)v + 2];
}
__device__ __forceinline__ void solve_store3(float *__restrict__ a, int v, const float (&o)[3]) {
  a[3 * (size_t)v] = o[0], a[3 * (size_t)v + 1] = o[1], a[3 * (size_t)v + 2] = o[2];
}
__device__ __forceinline__ bool solve_double_finite(double x) { return fabs(x) <= DBL_MAX; }

// ---------------------------------------------------------------------------------------------------------------- the operator
// the up to four runs of the fused gather; a run with starts == nullptr is absent.  (Plain pointers in the kernel's argument list, as in
// terms_gather_kernel.)  DOT: the solver's variant, which returns once the flag is set and writes the partial of x . q of its workgroup
template <bool DOT>
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_gather_kernel(const int *__restrict__ starts0, const int *__restrict__ entries0,
                                                                   const float *__restrict__ terms0, const int *__restrict__ starts1,
                                                                   const int *__restrict__ entries1, const float *__restrict__ terms1,
                                                                   const int *__restrict__ starts2, const int *__restrict__ entries2,
                                                                   const float *__restrict__ terms2, const int *__restrict__ starts3,
                                                                   const int *__restrict__ entries3, const float *__restrict__ terms3,
                                                                   const float *__restrict__ mass, const unsigned char *__restrict__ fixed,
                                                                   float scale, int nv, const float *__restrict__ x, float *__restrict__ q,
                                                                   double *__restrict__ partial, const int *__restrict__ flag) {
  if constexpr (DOT)
    if (*flag != SOLVE_RUNNING) return;
  const int v = blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  double d = 0.0;
  if (v < nv) {
    float out[3] = {0.f, 0.f, 0.f}, xv[3];
    solve_load3(x, v, xv);
    if (!solve_fixed(mass, fixed, v)) {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      if (starts0) terms_add_run(starts0, entries0, terms0, v, s0, s1, s2);
      if (starts1) terms_add_run(starts1, entries1, terms1, v, s0, s1, s2);
      if (starts2) terms_add_run(starts2, entries2, terms2, v, s0, s1, s2);
      if (starts3) terms_add_run(starts3, entries3, terms3, v, s0, s1, s2);
      const float m = mass[v];
      out[0] = m * xv[0] + scale * s0;
      out[1] = m * xv[1] + scale * s1;
      out[2] = m * xv[2] + scale * s2;
      if constexpr (DOT) d = solve_dot3(xv, out);
    }
    solve_store3(q, v, out);
  }
  if constexpr (DOT) {
    d = solve_block_sum(d);
    if (threadIdx.x == 0) partial[blockIdx.x] = d;
  }
}

// ---------------------------------------------------------------------------------------------------------------- the solver kernels
// r = b - q, z = D^-1 r, p = z and the partial of r . z
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_init_kernel(const float *__restrict__ b, const float *__restrict__ q,
                                                                 const float *__restrict__ inverse, int nv, float *__restrict__ r,
                                                                 float *__restrict__ z, float *__restrict__ p, double *__restrict__ partial) {
  const int v = blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  double d = 0.0;
  if (v < nv) {
    float bv[3], qv[3], rv[3], zv[3], B[6];
    solve_load3(b, v, bv);
    solve_load3(q, v, qv);
#pragma unroll
    for (int k = 0; k < 6; ++k) B[k] = inverse[6 * (size_t)v + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) rv[k] = bv[k] - qv[k];
    block_apply(B, rv, zv);
    solve_store3(r, v, rv);
    solve_store3(z, v, zv);
    solve_store3(p, v, zv);
    d = solve_dot3(rv, zv);
  }
  d = solve_block_sum(d);
  if (threadIdx.x == 0) partial[blockIdx.x] = d;
}

// one workgroup: the partials into the scalar of the stage, the record and the flag
template <int STAGE>
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_scalar_kernel(const double *__restrict__ partial, int parts, SolveState *state, int *record,
                                                                   int maxIters, float tol, float relTol) {
  int *iters = record, *flag = record + 1;
  float *history = reinterpret_cast<float *>(record + 2);
  if (*flag != SOLVE_RUNNING) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < parts; i += SOLVE_BLOCK) s += partial[i];
  s = solve_block_sum(s);
  if (threadIdx.x != 0) return;
  if constexpr (STAGE == SOLVE_STAGE_ALPHA) {
    if (!solve_double_finite(s)) *flag = SOLVE_NOT_FINITE;
    else if (!(s > 0.0)) *flag = SOLVE_BREAKDOWN;
    else state->alpha = (float)(state->rz / s);
  } else {
    if (!solve_double_finite(s) || s < 0.0) {
      *flag = SOLVE_NOT_FINITE;
      return;
    }
    const float res = (float)sqrt(s);
    int k = 0;
    if constexpr (STAGE == SOLVE_STAGE_INIT) {
      state->localTol = fminf(relTol * res, tol);
    } else {
      state->beta = (float)(s / state->rz);
      k = *iters + 1;
      *iters = k;
    }
    state->rz = s;
    history[k] = res;
    if (res <= state->localTol) *flag = SOLVE_CONVERGED;
    else if (k == maxIters) *flag = SOLVE_MAX_ITERS;
  }
}

// x += alpha p, r -= alpha q, z = D^-1 r and the partial of r . z
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_update_kernel(const float *__restrict__ p, const float *__restrict__ q,
                                                                   const float *__restrict__ inverse, const SolveState *__restrict__ state,
                                                                   const int *__restrict__ flag, int nv, float *__restrict__ x,
                                                                   float *__restrict__ r, float *__restrict__ z, double *__restrict__ partial) {
  if (*flag != SOLVE_RUNNING) return;
  const int v = blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  const float alpha = state->alpha;
  double d = 0.0;
  if (v < nv) {
    float pv[3], qv[3], xv[3], rv[3], zv[3], B[6];
    solve_load3(p, v, pv);
    solve_load3(q, v, qv);
    solve_load3(x, v, xv);
    solve_load3(r, v, rv);
#pragma unroll
    for (int k = 0; k < 6; ++k) B[k] = inverse[6 * (size_t)v + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) xv[k] = xv[k] + alpha * pv[k], rv[k] = rv[k] - alpha * qv[k];
    block_apply(B, rv, zv);
    solve_store3(x, v, xv);
    solve_store3(r, v, rv);
    solve_store3(z, v, zv);
    d = solve_dot3(rv, zv);
  }
  d = solve_block_sum(d);
  if (threadIdx.x == 0) partial[blockIdx.x] = d;
}

// p = z + beta p
__global__ __launch_bounds__(SOLVE_BLOCK) void solve_direction_kernel(const float *__restrict__ z, const SolveState *__restrict__ state,
                                                                      const int *__restrict__ flag, size_t n3, float *__restrict__ p) {
  if (*flag != SOLVE_RUNNING) return;
  const size_t i = (size_t)blockIdx.x * SOLVE_BLOCK + threadIdx.x;
  if (i < n3) p[i] = z[i] + state->beta * p[i];
}

// ---------------------------------------------------------------------------------------------------------------- host
// (SystemLayout, system_layout and system_ok: mesh_system.hpp, shared with mesh_potential.hip)

// the element kernels of the three products for the direction dir into scratch; st: six zeroed counts (elastic, barrier, friction)
static void system_launch_terms(Launch &L, const zs_rocm_mesh *m, const zs_rocm_mesh_system &s, const SystemLayout &l, const float *dir,
                                float *scratch, int *st) {
  if (s.elastic) elastic_launch_status(L, m, s.verts, s.mu, s.lam, s.kb, ELASTIC_OP_PRODUCT_PSD, dir, nullptr, nullptr, scratch + l.elastic, st);
  BarrierPairs pt, ee;
  if (s.barrier) {
    barrier_pair_args(m, s.verts, s.ptPairs, s.npt, s.eePairs, s.nee, s.dHat, s.kappa, s.mollify, dir, nullptr, nullptr, scratch + l.barrier, 12,
                      st + 2, {}, pt, ee);
    barrier_launch_args(L, BARRIER_OP_PRODUCT_PSD, pt, ee);
  }
  if (s.friction) {
    barrier_pair_args(m, s.u, s.fPtPairs, s.fNpt, s.fEePairs, s.fNee, 0.f, 0.f, 0, dir, nullptr, nullptr, scratch + l.friction, 12, st + 4,
                      {const_cast<float *>(s.record), s.fmu, s.epsv}, pt, ee);
    barrier_launch_args(L, BARRIER_OP_FRICTION_PRODUCT, pt, ee);
  }
}

template <bool DOT>
static void system_launch_gather(Launch &L, const zs_rocm_mesh *m, const zs_rocm_mesh_system &s, const SystemLayout &l, const float *scratch,
                                 const float *x, float *q, double *partial, const int *flag) {
  if (!m->nv) return;
  const TermRun none = {};
  const TermRun tri = s.elastic ? TermRun{m->cornerStarts, m->cornerVals, scratch + l.elastic} : none;
  const TermRun hinge = s.elastic ? TermRun{m->hingeStarts, m->hingeEntries, scratch + l.elastic + 9 * m->nt} : none;
  const TermRun bar = s.barrier ? TermRun{s.starts, s.entries, scratch + l.barrier} : none;
  const TermRun fr = s.friction ? TermRun{s.fStarts, s.fEntries, scratch + l.friction} : none;
  hipLaunchKernelGGL(solve_gather_kernel<DOT>, dim3(ceil_div(m->nv, SOLVE_BLOCK)), dim3(SOLVE_BLOCK), 0, L.stream, tri.starts, tri.entries, tri.terms,
                     hinge.starts, hinge.entries, hinge.terms, bar.starts, bar.entries, bar.terms, fr.starts, fr.entries, fr.terms, s.mass, s.fixed,
                     s.scale, (int)m->nv, x, q, partial, flag);
}

static int *system_status(Launch &L, int n) {
  int *st = (int *)L.temp(sizeof(int) * n);
  ZSR_CHECK(hipMemsetAsync(st, 0, sizeof(int) * n, L.stream));
  return st;
}

template <int NRUNS>
static void system_block_gather(Launch &L, const TermRun &a, const TermRun &b, size_t nv, float *out) {
  hipLaunchKernelGGL(solve_block_gather_kernel<NRUNS>, dim3(ceil_div(nv, SOLVE_BLOCK)), dim3(SOLVE_BLOCK), 0, L.stream, a.starts, a.entries, a.terms,
                     b.starts, b.entries, b.terms, (int)nv, out);
}

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_mesh_system_sizes(const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, size_t *sizes) {
  if (!m || !s || !sizes || (s->elastic && !m->hasRestShape) || (s->barrier && !barrier_counts_ok(s->npt, s->nee)) ||
      (s->friction && !barrier_counts_ok(s->fNpt, s->fNee)))
    return -1;
  sizes[0] = system_layout(m, *s, 3).total;
  sizes[1] = system_layout(m, *s, 6).total;
  sizes[2] = m->nv;
  return 0;
}

int zs_rocm_mesh_system_blocks(zs_rocm_policy *pol, const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, float *scratch, float *elastic,
                               float *barrier, float *friction, float *combined, float *inverse, int *status) {
  if (!system_ok(pol, m, s)) return -1;
  const SystemLayout l = system_layout(m, *s, 6);
  if ((l.total && !scratch) || (m->nv && (!elastic || !barrier || !friction || !combined || !inverse))) return -1;
  Launch L(pol, "mesh_system_blocks");
  int *st = status ? status : (int *)L.temp(sizeof(int) * 8);
  ZSR_CHECK(hipMemsetAsync(st, 0, sizeof(int) * 8, L.stream));
  const size_t nv = m->nv;
  const dim3 block(SOLVE_BLOCK);
  if (!nv) return 0;
  if (s->elastic) {
    float *tb = scratch + l.elastic, *hb = tb + 18 * m->nt;
    const bool membrane = s->mu > 0.f || s->lam > 0.f, bending = s->kb > 0.f;  // a kind that is skipped gets zero bytes, as in elastic_launch
    const BlockElems tri = {s->verts ? s->verts : m->verts, m->tris, (int)nv, (int)m->nt, m->triRecord, s->mu, s->lam, s->kb, tb, st};
    BlockElems hinge = tri;
    hinge.elems = m->hinges, hinge.n = (int)m->nh, hinge.record = m->hingeRecord, hinge.blocks = hb, hinge.status = st + 1;
    if (m->nt && membrane) {
      hipLaunchKernelGGL(solve_elem_block_kernel<false>, dim3(ceil_div(m->nt, SOLVE_BLOCK)), block, 0, L.stream, tri);
    } else if (m->nt) {
      ZSR_CHECK(hipMemsetAsync(tb, 0, sizeof(float) * 18 * m->nt, L.stream));
    }
    if (m->nh && bending) {
      hipLaunchKernelGGL(solve_elem_block_kernel<true>, dim3(ceil_div(m->nh, SOLVE_BLOCK)), block, 0, L.stream, hinge);
    } else if (m->nh) {
      ZSR_CHECK(hipMemsetAsync(hb, 0, sizeof(float) * 24 * m->nh, L.stream));
    }
    system_block_gather<2>(L, {m->cornerStarts, m->cornerVals, tb}, {m->hingeStarts, m->hingeEntries, hb}, nv, elastic);
  } else {
    ZSR_CHECK(hipMemsetAsync(elastic, 0, sizeof(float) * 6 * nv, L.stream));
  }
  BarrierPairs pt, ee;
  if (s->barrier) {
    barrier_pair_args(m, s->verts, s->ptPairs, s->npt, s->eePairs, s->nee, s->dHat, s->kappa, s->mollify, nullptr, nullptr, nullptr,
                      scratch + l.barrier, 24, st + 2, {}, pt, ee);
    if (pt.n) hipLaunchKernelGGL(solve_pair_block_kernel<BLOCK_PT>, dim3(ceil_div(pt.n, SOLVE_BLOCK)), block, 0, L.stream, pt);
    if (ee.n) hipLaunchKernelGGL(solve_pair_block_kernel<BLOCK_EE>, dim3(ceil_div(ee.n, SOLVE_BLOCK)), block, 0, L.stream, ee);
    system_block_gather<1>(L, {s->starts, s->entries, scratch + l.barrier}, {}, nv, barrier);
  } else {
    ZSR_CHECK(hipMemsetAsync(barrier, 0, sizeof(float) * 6 * nv, L.stream));
  }
  if (s->friction) {
    barrier_pair_args(m, s->u, s->fPtPairs, s->fNpt, s->fEePairs, s->fNee, 0.f, 0.f, 0, nullptr, nullptr, nullptr, scratch + l.friction, 24, st + 4,
                      {const_cast<float *>(s->record), s->fmu, s->epsv}, pt, ee);
    if (pt.n) hipLaunchKernelGGL(solve_pair_block_kernel<BLOCK_FRICTION_PT>, dim3(ceil_div(pt.n, SOLVE_BLOCK)), block, 0, L.stream, pt);
    if (ee.n) hipLaunchKernelGGL(solve_pair_block_kernel<BLOCK_FRICTION_EE>, dim3(ceil_div(ee.n, SOLVE_BLOCK)), block, 0, L.stream, ee);
    system_block_gather<1>(L, {s->fStarts, s->fEntries, scratch + l.friction}, {}, nv, friction);
  } else {
    ZSR_CHECK(hipMemsetAsync(friction, 0, sizeof(float) * 6 * nv, L.stream));
  }
  hipLaunchKernelGGL(solve_block_combine_kernel, dim3(ceil_div(nv, SOLVE_BLOCK)), block, 0, L.stream, elastic, barrier, friction, s->mass, s->fixed,
                     s->scale, (int)nv, combined, inverse, st + 6);
  return 0;
}

int zs_rocm_mesh_system_multiply(zs_rocm_policy *pol, const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, float *scratch, const float *x,
                                 float *q) {
  if (!system_ok(pol, m, s)) return -1;
  const SystemLayout l = system_layout(m, *s, 3);
  if ((l.total && !scratch) || (m->nv && (!x || !q))) return -1;
  Launch L(pol, "mesh_system_multiply");
  system_launch_terms(L, m, *s, l, x, scratch, system_status(L, 6));
  system_launch_gather<false>(L, m, *s, l, scratch, x, q, nullptr, nullptr);
  return 0;
}

int zs_rocm_mesh_system_solve(zs_rocm_policy *pol, const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, float *scratch, const float *inverse,
                              const float *b, float *x, int maxIters, float tol, float relTol, int checkEvery, void *record) {
  if (!system_ok(pol, m, s) || maxIters < 0 || checkEvery < 1 || !record) return -1;
  const SystemLayout l = system_layout(m, *s, 3);
  if ((l.total && !scratch) || (m->nv && (!inverse || !b || !x || b == x))) return -1;
  Launch L(pol, "mesh_system_solve");
  const size_t nv = m->nv, n3 = 3 * nv, n3p = (n3 + 63) & ~(size_t)63;
  int *rec = (int *)record;
  ZSR_CHECK(hipMemsetAsync(rec, 0, sizeof(int) * (3 + (size_t)maxIters), L.stream));
  // work vectors r, z, p, q, the partial sums and the scalars, all from the stream's temporary arena, once
  const unsigned parts = nv ? ceil_div(nv, SOLVE_BLOCK) : 0u;
  float *work = (float *)L.temp(sizeof(float) * 4 * (n3p + 64));
  float *r = work, *z = work + n3p, *p = work + 2 * n3p, *q = work + 3 * n3p;
  double *partial = (double *)L.temp(sizeof(double) * (parts + 1));
  SolveState *state = (SolveState *)L.temp(sizeof(SolveState));
  ZSR_CHECK(hipMemsetAsync(state, 0, sizeof(SolveState), L.stream));
  int *st = system_status(L, 6), *flag = rec + 1;
  const dim3 block(SOLVE_BLOCK), grid(parts);
  system_launch_terms(L, m, *s, l, x, scratch, st);
  system_launch_gather<false>(L, m, *s, l, scratch, x, q, nullptr, nullptr);
  if (nv) hipLaunchKernelGGL(solve_init_kernel, grid, block, 0, L.stream, b, (const float *)q, inverse, (int)nv, r, z, p, partial);
  hipLaunchKernelGGL(solve_scalar_kernel<SOLVE_STAGE_INIT>, dim3(1), block, 0, L.stream, (const double *)partial, (int)parts, state, rec, maxIters, tol,
                     relTol);
  for (int done = 0; done < maxIters;) {
    const int batch = maxIters - done < checkEvery ? maxIters - done : checkEvery;
    for (int k = 0; k < batch; ++k) {
      system_launch_terms(L, m, *s, l, p, scratch, st);
      system_launch_gather<true>(L, m, *s, l, scratch, p, q, partial, flag);
      hipLaunchKernelGGL(solve_scalar_kernel<SOLVE_STAGE_ALPHA>, dim3(1), block, 0, L.stream, (const double *)partial, (int)parts, state, rec, maxIters,
                         tol, relTol);
      if (nv) {
        hipLaunchKernelGGL(solve_update_kernel, grid, block, 0, L.stream, (const float *)p, (const float *)q, inverse, (const SolveState *)state,
                           (const int *)flag, (int)nv, x, r, z, partial);
      }
      hipLaunchKernelGGL(solve_scalar_kernel<SOLVE_STAGE_BETA>, dim3(1), block, 0, L.stream, (const double *)partial, (int)parts, state, rec, maxIters,
                         tol, relTol);
      if (nv) {
        hipLaunchKernelGGL(solve_direction_kernel, dim3(ceil_div(n3, SOLVE_BLOCK)), block, 0, L.stream, (const float *)z, (const SolveState *)state,
                           (const int *)flag, n3, p);
      }
    }
    done += batch;
    int f = SOLVE_RUNNING;  // the one read-back of the batch: a copy on the stream, then wait for it
    ZSR_CHECK(hipMemcpyAsync(&f, flag, sizeof(int), hipMemcpyDeviceToHost, L.stream));
    ZSR_CHECK(hipStreamSynchronize(L.stream));
    if (f != SOLVE_RUNNING) break;
  }
  return 0;
}

}  // extern "C"
