// mesh_potential.hip -- the incremental potential of an implicit cloth / shell step on a mesh for gfx950,
//
//     E(x) = 1/2 (x - xt)^T M (x - xt) + scale (Psi_elastic(x) + B(x) + D(x - start)),
//
// as one fused evaluation of energy and gradient and as a backtracking line search whose decisions stay on the device
// (include/zensim_rocm/potential_device.hpp has the arithmetic; the terms are those of mesh_elastic.hip and mesh_barrier.hip, launched here
// through mesh.hpp / mesh_pairs.hpp; the descriptor, its scratch layout and its checks are the Newton system's, mesh_system.hpp).
// Bit-reproducible: no float atomics anywhere.
//
//   energies  one float32 array, a part behind the other: the inertia energy of every vertex, then what the element kernels write -- triangles,
//             hinges; barrier PT, EE; friction PT, EE (a term that is absent has no room).
//   evaluate  the gradient operations of the element kernels write their energies there and their [corners][3] terms to the scratch array
//             (laid out as for the system's multiply); potential_gather_kernel, lane = vertex, sums the elastic triangle run, the elastic
//             hinge run, the barrier run and the friction run into one accumulator triple (an absent run has a null pointer), computes the
//             inertia energy and g = mass d + scale acc.  Energy only: the energy operations and potential_inertia_kernel, no gather.
//   totals    every part in the order of terms_total (mesh_terms.hip): potential_partial_kernel, one workgroup per chunk of 4096 energies of
//             one part, thread t the elements t, t + 256, .., an LDS tree; then potential_total_kernel, one workgroup, has thread t add a
//             part's partials t, t + 256, .. front to back and runs the same tree, part after part, and composes E.  Two launches for
//             the four totals, so parts[1..3] equal the energies of the public calls bit for bit.
//   slope     g . p as the solve's dot: every product exact in float64, the three added left to right, 256 vertices per workgroup (in the
//             gather kernel), an LDS tree, one workgroup over the partials (in the total kernel).
//   search    E_0, g, slope as above, then per trial: potential_trial_kernel (x_k = x + t_k p, u_k = x_k - start, the inertia energies at
//             x_k; t_k from the record), the energy operations at x_k / u_k, potential_partial_kernel, potential_total_kernel<TRIAL> (the
//             history entry, t, trials, the flag).  Every kernel of this file in the loop reads the flag first and returns if it is set, so
//             x, t, energy and the history are frozen from then on whatever else is enqueued (the element kernels still run: they write
//             scratch only).  The host enqueues checkEvery trials, copies the flag back and waits.
// Plain launches only.  Built with -ffp-contract=off (zpc_amd/build.py): tests/ref64_potential.py replays it operation by operation.
#include <cfloat>

#include "mesh_system.hpp"
#include "../../include/zensim_rocm/elastic_device.hpp"
#include "../../include/zensim_rocm/potential_device.hpp"

namespace zsr {

constexpr int POT_BLOCK = TERM_BLOCK;
constexpr int POT_CHUNK = 4096;  // RED_CHUNK of mesh_terms.hip
enum { POT_STAGE_EVAL, POT_STAGE_INIT, POT_STAGE_TRIAL };

// the four parts of the energy array (inertia, elastic, barrier, friction): floats before each, their lengths, and the chunks of POT_CHUNK
// before each (chunk[4]: all)
struct PotentialParts {
  size_t off[4], n[4];
  unsigned chunk[5];
};

// (a trailing barrier: the kernel that totals four parts calls this four times)
__device__ __forceinline__ double potential_block_sum(double s) {
  __shared__ double sm[POT_BLOCK];
  sm[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int h = POT_BLOCK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ void potential_load3(const float *__restrict__ a, int v, float (&o)[3]) {
  o[0] = a[3 * (size_t)v], o[1] = a[3 * (size_t)v + 1], o[2] = a[3 * (size_t)v + 2];
}
__device__ __forceinline__ void potential_store3(float *__restrict__ a, int v, const float (&o)[3]) {
  a[3 * (size_t)v] = o[0], a[3 * (size_t)v + 1] = o[1], a[3 * (size_t)v + 2] = o[2];
}

// ---------------------------------------------------------------------------------------------------------------- per vertex
// u = x - start, every component
__global__ __launch_bounds__(POT_BLOCK) void potential_displacement_kernel(const float *__restrict__ x, const float *__restrict__ start, size_t n3,
                                                                           float *__restrict__ u) {
  const size_t i = (size_t)blockIdx.x * POT_BLOCK + threadIdx.x;
  if (i < n3) u[i] = x[i] - start[i];
}

__global__ __launch_bounds__(POT_BLOCK) void potential_inertia_kernel(const float *__restrict__ x, const float *__restrict__ target,
                                                                      const float *__restrict__ mass, const unsigned char *__restrict__ fixed, int nv,
                                                                      float *__restrict__ inertia) {
  const int v = blockIdx.x * POT_BLOCK + threadIdx.x;
  if (v >= nv) return;
  float e = 0.f;
  if (!potential_fixed(mass, fixed, v)) {
    float xv[3], tv[3], d[3];
    potential_load3(x, v, xv);
    potential_load3(target, v, tv);
    e = potential_inertia(xv, tv, mass[v], d);
  }
  inertia[v] = e;
}

// the up to four runs of the fused gather (a run with starts == nullptr is absent; plain pointers, as in solve_gather_kernel), the inertia
// energy and g = mass d + scale acc.  DOT: the partial of g . p of the workgroup as well
template <bool DOT>
__global__ __launch_bounds__(POT_BLOCK) void potential_gather_kernel(const int *__restrict__ starts0, const int *__restrict__ entries0,
                                                                     const float *__restrict__ terms0, const int *__restrict__ starts1,
                                                                     const int *__restrict__ entries1, const float *__restrict__ terms1,
                                                                     const int *__restrict__ starts2, const int *__restrict__ entries2,
                                                                     const float *__restrict__ terms2, const int *__restrict__ starts3,
                                                                     const int *__restrict__ entries3, const float *__restrict__ terms3,
                                                                     const float *__restrict__ mass, const unsigned char *__restrict__ fixed,
                                                                     float scale, int nv, const float *__restrict__ x,
                                                                     const float *__restrict__ target, const float *__restrict__ p,
                                                                     float *__restrict__ g, float *__restrict__ inertia,
                                                                     double *__restrict__ partial) {
  const int v = blockIdx.x * POT_BLOCK + threadIdx.x;
  double d = 0.0;
  if (v < nv) {
    float out[3] = {0.f, 0.f, 0.f}, e = 0.f;
    if (!potential_fixed(mass, fixed, v)) {
      float acc[3] = {0.f, 0.f, 0.f}, xv[3], tv[3], dv[3];
      if (starts0) terms_add_run(starts0, entries0, terms0, v, acc[0], acc[1], acc[2]);
      if (starts1) terms_add_run(starts1, entries1, terms1, v, acc[0], acc[1], acc[2]);
      if (starts2) terms_add_run(starts2, entries2, terms2, v, acc[0], acc[1], acc[2]);
      if (starts3) terms_add_run(starts3, entries3, terms3, v, acc[0], acc[1], acc[2]);
      potential_load3(x, v, xv);
      potential_load3(target, v, tv);
      const float m = mass[v];
      e = potential_inertia(xv, tv, m, dv);
      potential_gradient(m, dv, scale, acc, out);
      if constexpr (DOT) {
        float pv[3];
        potential_load3(p, v, pv);
        d = ((double)out[0] * (double)pv[0] + (double)out[1] * (double)pv[1]) + (double)out[2] * (double)pv[2];
      }
    }
    potential_store3(g, v, out);
    inertia[v] = e;
  }
  if constexpr (DOT) {
    d = potential_block_sum(d);
    if (threadIdx.x == 0) partial[blockIdx.x] = d;
  }
}

// trial k of the search: x_k = x + t_k p (x at a fixed vertex), u_k = x_k - start (start == nullptr: no friction), the inertia energies
__global__ __launch_bounds__(POT_BLOCK) void potential_trial_kernel(const float *__restrict__ x, const float *__restrict__ p,
                                                                    const float *__restrict__ start, const float *__restrict__ target,
                                                                    const float *__restrict__ mass, const unsigned char *__restrict__ fixed, int nv,
                                                                    const PotentialRecord *__restrict__ rec, float *__restrict__ xk,
                                                                    float *__restrict__ uk, float *__restrict__ inertia) {
  if (rec->flag != POTENTIAL_RUNNING) return;
  const int v = blockIdx.x * POT_BLOCK + threadIdx.x;
  if (v >= nv) return;
  const float t = rec->tNext;
  const bool fx = potential_fixed(mass, fixed, v);
  float xv[3], pv[3], y[3];
  potential_load3(x, v, xv);
  potential_load3(p, v, pv);
  potential_trial(xv, pv, t, fx, y);
  potential_store3(xk, v, y);
  if (start) {
    float sv[3], u[3];
    potential_load3(start, v, sv);
    potential_displacement(y, sv, u);
    potential_store3(uk, v, u);
  }
  float e = 0.f;
  if (!fx) {
    float tv[3], d[3];
    potential_load3(target, v, tv);
    e = potential_inertia(y, tv, mass[v], d);
  }
  inertia[v] = e;
}

// ---------------------------------------------------------------------------------------------------------------- totals and decisions
// workgroup b: one chunk of one part (flag == nullptr: an evaluation)
__global__ __launch_bounds__(POT_BLOCK) void potential_partial_kernel(const float *__restrict__ energy, const PotentialParts a,
                                                                      double *__restrict__ partial, const int *__restrict__ flag) {
  if (flag && *flag != POTENTIAL_RUNNING) return;
  const unsigned b = blockIdx.x;
  int k = 0;
  while (k < 3 && b >= a.chunk[k + 1]) ++k;
  const size_t lo = (size_t)(b - a.chunk[k]) * POT_CHUNK, n = a.n[k];
  const size_t hi = lo + POT_CHUNK < n ? lo + POT_CHUNK : n;
  const float *e = energy + a.off[k];
  double s = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += POT_BLOCK) s += (double)e[i];
  s = potential_block_sum(s);
  if (threadIdx.x == 0) partial[b] = s;
}

// one workgroup: the four totals, E and what the stage does with it -- EVAL: out[0..3] = the parts, out[4] = E; INIT: the slope from the
// partials of g . p, the start of the record; TRIAL: the decision
template <int STAGE>
__global__ __launch_bounds__(POT_BLOCK) void potential_total_kernel(const double *__restrict__ partial, const PotentialParts a,
                                                                    const double *__restrict__ dotPartial, int ndot, float scale, double *out,
                                                                    PotentialRecord *rec, float tMax, const float *__restrict__ tMaxDev, float c1,
                                                                    float shrink, int maxTrials) {
  if constexpr (STAGE != POT_STAGE_EVAL)
    if (rec->flag != POTENTIAL_RUNNING) return;
  double parts[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double s = 0.0;
    for (unsigned i = a.chunk[k] + threadIdx.x; i < a.chunk[k + 1]; i += POT_BLOCK) s += partial[i];
    parts[k] = potential_block_sum(s);
  }
  [[maybe_unused]] double slope = 0.0;
  if constexpr (STAGE == POT_STAGE_INIT) {
    for (int i = threadIdx.x; i < ndot; i += POT_BLOCK) slope += dotPartial[i];
    slope = potential_block_sum(slope);
  }
  if (threadIdx.x != 0) return;
  const double e = potential_energy(parts, scale);
  if constexpr (STAGE == POT_STAGE_EVAL) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = parts[k];
    out[4] = e;
  } else {
    double *history = reinterpret_cast<double *>(rec + 1);
    PotentialRecord r = *rec;
    if constexpr (STAGE == POT_STAGE_INIT)
      potential_begin(r, history, e, slope, tMaxDev ? *tMaxDev : tMax);
    else
      potential_decide(r, history, e, c1, shrink, maxTrials);
    *rec = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct PotentialPlan {
  SystemLayout l;       // the terms in scratch, three floats per corner
  PotentialParts parts;
  size_t energies;      // floats of the energy array
};
static PotentialPlan potential_plan(const zs_rocm_mesh *m, const zs_rocm_mesh_system &s) {
  PotentialPlan p;
  p.l = system_layout(m, s, 3);
  const size_t n[4] = {m->nv, s.elastic ? m->nt + m->nh : 0, s.barrier ? s.npt + s.nee : 0, s.friction ? s.fNpt + s.fNee : 0};
  size_t off = 0;
  unsigned chunk = 0;
  for (int k = 0; k < 4; ++k) {
    p.parts.off[k] = off, p.parts.n[k] = n[k], p.parts.chunk[k] = chunk;
    off += n[k], chunk += (unsigned)((n[k] + POT_CHUNK - 1) / POT_CHUNK);
  }
  p.parts.chunk[4] = chunk, p.energies = off;
  return p;
}

static bool potential_counts_ok(const zs_rocm_mesh *m, const zs_rocm_mesh_system *s) {
  return !(s->elastic && !m->hasRestShape) && !(s->barrier && !barrier_counts_ok(s->npt, s->nee)) &&
         !(s->friction && !barrier_counts_ok(s->fNpt, s->fNee));
}

// the system's checks with the positions and the start of the step in the places of its trial positions and its displacement (friction
// needs start), and the two arrays every entry reads
static bool potential_ok(const zs_rocm_policy *pol, const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, const float *target, const float *start,
                         const float *verts) {
  if (!s) return false;
  zs_rocm_mesh_system c = *s;
  c.verts = verts, c.u = start;
  if (!system_ok(pol, m, &c) || !potential_counts_ok(m, s)) return false;
  return !(m->nv && (!target || !verts));
}

// the element kernels of the three terms at verts / u: the gradient operations (energies and terms) or the energy operations; st: six
// zeroed counts (elastic, barrier, friction)
static void potential_launch_terms(Launch &L, const zs_rocm_mesh *m, const zs_rocm_mesh_system &s, const PotentialPlan &p, bool gradient,
                                   const float *verts, const float *u, float *energy, float *scratch, int *st) {
  if (s.elastic) {
    float *e = energy + p.parts.off[1];
    elastic_launch_status(L, m, verts, s.mu, s.lam, s.kb, gradient ? ELASTIC_OP_GRADIENT : ELASTIC_OP_ENERGY, nullptr, e, e + m->nt,
                          gradient ? scratch + p.l.elastic : nullptr, st);
  }
  BarrierPairs pt, ee;
  if (s.barrier) {
    float *e = energy + p.parts.off[2];
    barrier_pair_args(m, verts, s.ptPairs, s.npt, s.eePairs, s.nee, s.dHat, s.kappa, s.mollify, nullptr, e, e + s.npt,
                      gradient ? scratch + p.l.barrier : nullptr, 12, st + 2, {}, pt, ee);
    barrier_launch_args(L, gradient ? BARRIER_OP_GRADIENT : BARRIER_OP_ENERGY, pt, ee);
  }
  if (s.friction) {
    float *e = energy + p.parts.off[3];
    barrier_pair_args(m, u, s.fPtPairs, s.fNpt, s.fEePairs, s.fNee, 0.f, 0.f, 0, nullptr, e, e + s.fNpt, gradient ? scratch + p.l.friction : nullptr,
                      12, st + 4, {const_cast<float *>(s.record), s.fmu, s.epsv}, pt, ee);
    barrier_launch_args(L, gradient ? BARRIER_OP_FRICTION_GRADIENT : BARRIER_OP_FRICTION_ENERGY, pt, ee);
  }
}

template <bool DOT>
static void potential_launch_gather(Launch &L, const zs_rocm_mesh *m, const zs_rocm_mesh_system &s, const PotentialPlan &p, const float *scratch,
                                    const float *x, const float *target, const float *dir, float *g, float *inertia, double *partial) {
  if (!m->nv) return;
  const TermRun none = {};
  const TermRun tri = s.elastic ? TermRun{m->cornerStarts, m->cornerVals, scratch + p.l.elastic} : none;
  const TermRun hinge = s.elastic ? TermRun{m->hingeStarts, m->hingeEntries, scratch + p.l.elastic + 9 * m->nt} : none;
  const TermRun bar = s.barrier ? TermRun{s.starts, s.entries, scratch + p.l.barrier} : none;
  const TermRun fr = s.friction ? TermRun{s.fStarts, s.fEntries, scratch + p.l.friction} : none;
  hipLaunchKernelGGL(potential_gather_kernel<DOT>, dim3(ceil_div(m->nv, POT_BLOCK)), dim3(POT_BLOCK), 0, L.stream, tri.starts, tri.entries, tri.terms,
                     hinge.starts, hinge.entries, hinge.terms, bar.starts, bar.entries, bar.terms, fr.starts, fr.entries, fr.terms, s.mass, s.fixed,
                     s.scale, (int)m->nv, x, target, dir, g, inertia, partial);
}

// the partials of the four parts, then the stage's total kernel
template <int STAGE>
static void potential_launch_totals(Launch &L, const PotentialPlan &p, const float *energy, double *partial, const double *dotPartial, int ndot,
                                    float scale, double *out, PotentialRecord *rec, float tMax, const float *tMaxDev, float c1, float shrink,
                                    int maxTrials) {
  const int *flag = STAGE == POT_STAGE_TRIAL ? &rec->flag : nullptr;
  if (p.parts.chunk[4])
    hipLaunchKernelGGL(potential_partial_kernel, dim3(p.parts.chunk[4]), dim3(POT_BLOCK), 0, L.stream, energy, p.parts, partial, flag);
  hipLaunchKernelGGL(potential_total_kernel<STAGE>, dim3(1), dim3(POT_BLOCK), 0, L.stream, (const double *)partial, p.parts, dotPartial, ndot, scale,
                     out, rec, tMax, tMaxDev, c1, shrink, maxTrials);
}

static int *potential_status(Launch &L, int *status) {
  int *st = status ? status : (int *)L.temp(sizeof(int) * 6);
  ZSR_CHECK(hipMemsetAsync(st, 0, sizeof(int) * 6, L.stream));
  return st;
}

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_mesh_potential_sizes(const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, size_t *sizes) {
  if (!m || !s || !sizes || !potential_counts_ok(m, s)) return -1;
  const PotentialPlan p = potential_plan(m, *s);
  sizes[0] = p.l.total;
  sizes[1] = p.energies;
  sizes[2] = m->nv;
  return 0;
}

int zs_rocm_mesh_potential_evaluate(zs_rocm_policy *pol, const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, const float *target,
                                    const float *start, const float *verts, float *scratch, float *energies, double *parts, float *grad,
                                    int *status) {
  if (!potential_ok(pol, m, s, target, start, verts) || !parts) return -1;
  const PotentialPlan p = potential_plan(m, *s);
  if ((p.energies && !energies) || (grad && p.l.total && !scratch)) return -1;
  Launch L(pol, "mesh_potential_evaluate");
  const size_t nv = m->nv, n3 = 3 * nv;
  int *st = potential_status(L, status);
  float *u = nullptr;
  if (s->friction && nv) {
    u = (float *)L.temp(sizeof(float) * n3);
    hipLaunchKernelGGL(potential_displacement_kernel, dim3(ceil_div(n3, POT_BLOCK)), dim3(POT_BLOCK), 0, L.stream, verts, start, n3, u);
  }
  double *partial = (double *)L.temp(sizeof(double) * ((size_t)p.parts.chunk[4] + 1));
  potential_launch_terms(L, m, *s, p, grad != nullptr, verts, u, energies, scratch, st);
  if (grad) {
    potential_launch_gather<false>(L, m, *s, p, scratch, verts, target, nullptr, grad, energies, nullptr);
  } else if (nv) {
    hipLaunchKernelGGL(potential_inertia_kernel, dim3(ceil_div(nv, POT_BLOCK)), dim3(POT_BLOCK), 0, L.stream, verts, target, s->mass, s->fixed, (int)nv,
                       energies);
  }
  potential_launch_totals<POT_STAGE_EVAL>(L, p, energies, partial, nullptr, 0, s->scale, parts, nullptr, 0.f, nullptr, 0.f, 0.f, 0);
  return 0;
}

int zs_rocm_mesh_potential_line_search(zs_rocm_policy *pol, const zs_rocm_mesh *m, const zs_rocm_mesh_system *s, const float *target,
                                       const float *start, const float *verts, const float *dir, float tMax, const float *tMaxDev, float c1,
                                       float shrink, int maxTrials, int checkEvery, float *scratch, float *energies, float *x, void *record) {
  if (!potential_ok(pol, m, s, target, start, verts) || !record || maxTrials < 1 || checkEvery < 1) return -1;
  if (!(c1 >= 0.f && c1 <= FLT_MAX) || !(shrink > 0.f && shrink < 1.f)) return -1;
  const PotentialPlan p = potential_plan(m, *s);
  if ((p.energies && !energies) || (p.l.total && !scratch) || (m->nv && (!dir || !x || x == verts || x == dir))) return -1;
  Launch L(pol, "mesh_potential_line_search");
  const size_t nv = m->nv, n3 = 3 * nv;
  PotentialRecord *rec = (PotentialRecord *)record;
  ZSR_CHECK(hipMemsetAsync(rec, 0, sizeof(PotentialRecord) + sizeof(double) * ((size_t)maxTrials + 1), L.stream));
  int *st = potential_status(L, nullptr);
  const dim3 block(POT_BLOCK), grid(nv ? ceil_div(nv, POT_BLOCK) : 0u);
  const int ndot = (int)grid.x;
  // the gradient, the displacement, the partial sums: all from the stream's temporary arena, once
  float *g = (float *)L.temp(sizeof(float) * (n3 + 64));
  float *u = s->friction ? (float *)L.temp(sizeof(float) * (n3 + 64)) : nullptr;
  double *partial = (double *)L.temp(sizeof(double) * ((size_t)p.parts.chunk[4] + 1));
  double *dotPartial = (double *)L.temp(sizeof(double) * ((size_t)ndot + 1));
  if (u && nv) hipLaunchKernelGGL(potential_displacement_kernel, dim3(ceil_div(n3, POT_BLOCK)), block, 0, L.stream, verts, start, n3, u);
  potential_launch_terms(L, m, *s, p, true, verts, u, energies, scratch, st);
  potential_launch_gather<true>(L, m, *s, p, scratch, verts, target, dir, g, energies, dotPartial);
  potential_launch_totals<POT_STAGE_INIT>(L, p, energies, partial, dotPartial, ndot, s->scale, nullptr, rec, tMax, tMaxDev, c1, shrink, maxTrials);
  int f = POTENTIAL_RUNNING;
  for (int done = 0; done < maxTrials;) {
    const int batch = maxTrials - done < checkEvery ? maxTrials - done : checkEvery;
    for (int k = 0; k < batch; ++k) {
      if (nv) {
        hipLaunchKernelGGL(potential_trial_kernel, grid, block, 0, L.stream, verts, dir, u ? start : nullptr, target, s->mass, s->fixed, (int)nv,
                           (const PotentialRecord *)rec, x, u, energies);
      }
      potential_launch_terms(L, m, *s, p, false, x, u, energies, nullptr, st);
      potential_launch_totals<POT_STAGE_TRIAL>(L, p, energies, partial, nullptr, 0, s->scale, nullptr, rec, tMax, tMaxDev, c1, shrink, maxTrials);
    }
    done += batch;
    f = POTENTIAL_RUNNING;  // the one read-back of the batch: a copy on the stream, then wait for it
    ZSR_CHECK(hipMemcpyAsync(&f, &rec->flag, sizeof(int), hipMemcpyDeviceToHost, L.stream));
    ZSR_CHECK(hipStreamSynchronize(L.stream));
    if (f != POTENTIAL_RUNNING) break;
  }
  // no trial accepted: x is where the search started
  if (f != POTENTIAL_ACCEPTED && nv) ZSR_CHECK(hipMemcpyAsync(x, verts, sizeof(float) * n3, hipMemcpyDeviceToDevice, L.stream));
  return 0;
}

}  // extern "C"
