// mesh_terms.hip -- what the terms of a mesh share behind their per-element kernels, for gfx950 (mesh.hpp declares it; mesh_barrier.hip:
// barrier and friction on the pairs of a proximity list, mesh_elastic.hip: membrane and bending on triangles and hinges).  An element
// kernel writes one float32 energy per element and its [corners][3] terms to a scratch array, once.  Bit-reproducible: no float atomics.
//
//   incidence built once per element list, independent of the positions: the (vertex, corners * element + corner) entries stably sorted by
//             vertex with radix_sort_pair_u32, so a vertex's run is in element order; run starts = exclusive scan of the per-vertex counts
//             (integer atomics: a count has no order).  The entry kernel is the caller's (incidence_kernel of mesh.hpp over its own rule).
//   gather    lane = vertex: sums the scratch terms of its runs, one run after the other, each front to back.  The order is the lists', so
//             two calls give the same bytes.  A long run (a hub vertex) costs its lane that many loads and nothing else.
//   total     float64 sum of the float32 energies of two arrays, one behind the other, in a fixed order: workgroup g sums elements
//             [g, g + 1) x RED_CHUNK, thread t the elements t, t + 256, .. of the chunk, then an LDS tree; one workgroup sums the partials
//             the same way.
// Built with -ffp-contract=off (zpc_amd/build.py) like the translation units it serves.
#include "mesh.hpp"

namespace zsr {

constexpr int RED_CHUNK = 4096;

// ---------------------------------------------------------------------------------------------------------------- incidence
IncidenceKeys incidence_begin(Launch &L, size_t n, size_t nv) {
  IncidenceKeys k = {nullptr, nullptr, (unsigned *)L.temp(sizeof(unsigned) * (nv + 1))};
  ZSR_CHECK(hipMemsetAsync(k.counts, 0, sizeof(unsigned) * (nv + 1), L.stream));
  if (n) k.keys = (unsigned *)L.temp(sizeof(unsigned) * n), k.vals = (int *)L.temp(sizeof(int) * n);
  return k;
}

void incidence_end(Launch &L, const IncidenceKeys &k, size_t n, size_t nv, int *starts, int *entries) {
  if (n) radix_sort_pair_u32(L, k.keys, k.vals, (unsigned *)L.temp(sizeof(unsigned) * n), entries, n, 0, key_bits(nv + 1));  // keys 0 .. nv
  exclusive_scan_u32(L, k.counts, nv + 1, (unsigned *)starts);
}

// ---------------------------------------------------------------------------------------------------------------- gather
// (plain pointer arguments, not the TermRun structs: the compiler then loads every kernel argument ahead of the first run)
template <int NRUNS>
__global__ __launch_bounds__(TERM_BLOCK) void terms_gather_kernel(const int *__restrict__ starts0, const int *__restrict__ entries0,
                                                                  const float *__restrict__ terms0, const int *__restrict__ starts1,
                                                                  const int *__restrict__ entries1, const float *__restrict__ terms1, int nv,
                                                                  float *__restrict__ out) {
  const int v = blockIdx.x * TERM_BLOCK + threadIdx.x;
  if (v >= nv) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  terms_add_run(starts0, entries0, terms0, v, s0, s1, s2);
  if constexpr (NRUNS == 2) terms_add_run(starts1, entries1, terms1, v, s0, s1, s2);
  out[3 * (size_t)v] = s0;
  out[3 * (size_t)v + 1] = s1;
  out[3 * (size_t)v + 2] = s2;
}

void terms_gather(Launch &L, const TermRun *runs, int nruns, size_t nv, float *out) {
  if (!nv) return;
  const TermRun a = runs[0], b = nruns == 2 ? runs[1] : TermRun{};
  hipLaunchKernelGGL(nruns == 2 ? terms_gather_kernel<2> : terms_gather_kernel<1>, dim3(ceil_div(nv, TERM_BLOCK)), dim3(TERM_BLOCK), 0, L.stream,
                     a.starts, a.entries, a.terms, b.starts, b.entries, b.terms, (int)nv, out);
}

// ---------------------------------------------------------------------------------------------------------------- the float64 total
__device__ __forceinline__ double terms_block_sum(double s) {
  __shared__ double sm[TERM_BLOCK];
  sm[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int h = TERM_BLOCK / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  return sm[0];
}
__global__ __launch_bounds__(TERM_BLOCK) void terms_partial_kernel(const float *__restrict__ a, size_t na, const float *__restrict__ b, size_t nb,
                                                                   double *partial) {
  const size_t lo = (size_t)blockIdx.x * RED_CHUNK, n = na + nb;
  const size_t hi = lo + RED_CHUNK < n ? lo + RED_CHUNK : n;
  double s = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += TERM_BLOCK) s += (double)(i < na ? a[i] : b[i - na]);
  s = terms_block_sum(s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(TERM_BLOCK) void terms_total_kernel(const double *__restrict__ partial, size_t n, double *total) {
  double s = 0.0;
  for (size_t i = threadIdx.x; i < n; i += TERM_BLOCK) s += partial[i];
  s = terms_block_sum(s);
  if (threadIdx.x == 0) *total = s;
}

void terms_total(Launch &L, const float *a, size_t na, const float *b, size_t nb, double *total) {
  const size_t n = na + nb, parts = (n + RED_CHUNK - 1) / RED_CHUNK;
  double *partial = parts ? (double *)L.temp(sizeof(double) * parts) : nullptr;
  if (parts) hipLaunchKernelGGL(terms_partial_kernel, dim3((unsigned)parts), dim3(TERM_BLOCK), 0, L.stream, a, na, b, nb, partial);
  hipLaunchKernelGGL(terms_total_kernel, dim3(1), dim3(TERM_BLOCK), 0, L.stream, partial, parts, total);
}

int *terms_status(Launch &L, int *status) {
  int *st = status ? status : (int *)L.temp(sizeof(int) * 2);
  ZSR_CHECK(hipMemsetAsync(st, 0, sizeof(int) * 2, L.stream));
  return st;
}

}  // namespace zsr
