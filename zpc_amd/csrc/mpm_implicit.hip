// mpm_implicit.hip -- the implicit-MPM system: zs_rocm_mpm_implicit_force (G2P2GTransfer, kernels: mpm_implicit_kernels.hpp),
// _multiply / _precondition (ImplicitMPMSystem, simulation/mpm/ImplicitMPM.hpp:11-157; _project lives in mpm_implicit_project.hip, which
// is built without FP contraction like collider.hip), the dof-vector operators (math/linear/LinearOperators.hpp:14-72) and
// zs_rocm_mpm_implicit_solve (ConjugateGradient::solve, math/linear/ConjugateGradient.hpp:60-162).
//
// The solve runs the reference's operation sequence; its debug prints (checkVector, the per-iteration fmt::print) and the getchar()
// of ConjugateGradient.hpp:158 are left out.
#include "mpm_implicit_kernels.hpp"

namespace zsr {
// mpm_implicit_project.hip
void implicit_project_enqueue(hipStream_t stream, const zs_rocm_mpm_params *p, const int *activeKeys, const float *grid, size_t nblocks,
                              const zs_rocm_collider *collider, float *inout);

// ---- entry-wise kernels on dof vectors (bandwidth-trivial)
enum { DOF_PLUS = 0, DOF_MULTIPLIES = 1, DOF_MINUS = 2, DOF_DIVIDES = 3 };
template <int OP> static __global__ __launch_bounds__(256) void dof_compwise_kernel(const float *a, const float *b, float *c, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = a[i], y = b[i];
  c[i] = OP == DOF_PLUS ? x + y : OP == DOF_MULTIPLIES ? x * y : OP == DOF_MINUS ? x - y : x / y;
}
static __global__ __launch_bounds__(256) void dof_fill_kernel(float *a, float v, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}
// c = m a + n b (LinearCombineOp)
static __global__ __launch_bounds__(256) void dof_linear_combine_kernel(float m, const float *a, float nn, const float *b, float *c, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) c[i] = m * a[i] + nn * b[i];
}

// a . b in two levels, the shape of the library's float reduce (grid-stride partial sums per workgroup, one workgroup adds them), with the
// product formed in the load.  It is a kernel pair of its own and not a call into reduce because that one (primitives.hip) is a
// file-static template over an iterator Port of ONE input: giving it a second input or a load functor means changing the existing
// reduce kernels, which carry the scan / sort paths' tuning.
constexpr int DOT_BLOCK = 256, DOT_MAX_BLOCKS = 1024;
__device__ __forceinline__ float dot_block_reduce(float v) {
  __shared__ float part[DOT_BLOCK / 64];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += shfl_down(v, d);
  if (lane_id() == 0) part[wave_id()] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0)
    for (int k = 0; k < DOT_BLOCK / 64; ++k) s += part[k];
  return s;
}
static __global__ __launch_bounds__(DOT_BLOCK) void dof_dot_partial_kernel(const float *a, const float *b, size_t n, float *partials) {
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * DOT_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * DOT_BLOCK) acc = fmaf(a[i], b[i], acc);
  acc = dot_block_reduce(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}
static __global__ __launch_bounds__(DOT_BLOCK) void dof_dot_final_kernel(const float *partials, int np, float *out) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < np; i += DOT_BLOCK) acc += partials[i];
  acc = dot_block_reduce(acc);
  if (threadIdx.x == 0) *out = acc;
}

// ForceDtSqrPlusMass (ImplicitMPM.hpp:16-31), as written: entry-wise (f dt dt + m) v on nodes with mass; the contraction of
// (f dt) dt + m that the compiler would pick anyway is spelled out, so the entry has three roundings in every build
template <int SIDE> static __global__ __launch_bounds__(256) void implicit_mass_kernel(const float *grid, const float *vIn, float *out, size_t nEntries, float dt) {
  constexpr int NC = SIDE * SIDE * SIDE;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nEntries) return;
  const size_t node = i / 3;
  const float mass = grid[(node / NC) * 7 * NC + node % NC];
  if (mass > 0.f) out[i] = fmaf(out[i] * dt, dt, mass) * vIn[i];
}
// DivPernodeMass (ImplicitMPM.hpp:126-137): IEEE division, one rounding
template <int SIDE> static __global__ __launch_bounds__(256) void implicit_precondition_kernel(const float *grid, const float *in, float *out, size_t nEntries) {
  constexpr int NC = SIDE * SIDE * SIDE;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nEntries) return;
  const size_t node = i / 3;
  const float mass = grid[(node / NC) * 7 * NC + node % NC];
  if (mass > 0.f) out[i] = in[i] / mass;
}

// ---- host side, on a Launch that the caller holds (the solve keeps one Launch, and with it its temporaries, for all its iterations)
static void dof_fill(Launch &L, float *a, float v, size_t n) {
  if (n) hipLaunchKernelGGL(dof_fill_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, a, v, n);
}
static void dof_assign(Launch &L, const float *a, float *b, size_t n) {
  if (n && a != b) ZSR_CHECK(hipMemcpyAsync(b, a, n * sizeof(float), hipMemcpyDeviceToDevice, L.stream));
}
static void dof_compwise(Launch &L, int op, const float *a, const float *b, float *c, size_t n) {
  if (!n) return;
  const dim3 g(ceil_div(n, 256)), bl(256);
  switch (op) {
    case DOF_PLUS: hipLaunchKernelGGL((dof_compwise_kernel<DOF_PLUS>), g, bl, 0, L.stream, a, b, c, n); break;
    case DOF_MULTIPLIES: hipLaunchKernelGGL((dof_compwise_kernel<DOF_MULTIPLIES>), g, bl, 0, L.stream, a, b, c, n); break;
    case DOF_MINUS: hipLaunchKernelGGL((dof_compwise_kernel<DOF_MINUS>), g, bl, 0, L.stream, a, b, c, n); break;
    default: hipLaunchKernelGGL((dof_compwise_kernel<DOF_DIVIDES>), g, bl, 0, L.stream, a, b, c, n); break;
  }
}
static void dof_linear_combine(Launch &L, float m, const float *a, float nn, const float *b, float *c, size_t n) {
  if (n) hipLaunchKernelGGL(dof_linear_combine_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, L.stream, m, a, nn, b, c, n);
}
// partials: DOT_MAX_BLOCKS floats
static void dof_dot(Launch &L, const float *a, const float *b, size_t n, float *partials, float *out) {
  const unsigned nb = n ? (ceil_div(n, DOT_BLOCK * 4) < (unsigned)DOT_MAX_BLOCKS ? (ceil_div(n, DOT_BLOCK * 4) ? ceil_div(n, DOT_BLOCK * 4) : 1u) : (unsigned)DOT_MAX_BLOCKS) : 1u;
  hipLaunchKernelGGL(dof_dot_partial_kernel, dim3(nb), dim3(DOT_BLOCK), 0, L.stream, a, b, n, partials);
  hipLaunchKernelGGL(dof_dot_final_kernel, dim3(1), dim3(DOT_BLOCK), 0, L.stream, (const float *)partials, (int)nb, out);
}
static float read_back(Launch &L, const float *dev) {  // like bht::size(): a copy on the stream, then wait for it
  float v = 0.f;
  ZSR_CHECK(hipMemcpyAsync(&v, dev, sizeof(float), hipMemcpyDeviceToHost, L.stream));
  ZSR_CHECK(hipStreamSynchronize(L.stream));
  return v;
}

struct ImplicitArgs {
  const zs_rocm_mpm_params *p;
  zs_rocm_particles ps;
  const zs_rocm_bht_3 *tab;
  const float *grid;
  size_t nblocks;
  const int *binStart;
  const unsigned *cellCount;
  const int *nbr;
  bool binned() const { return binStart && cellCount && nbr; }
  size_t entries() const { return nblocks * (size_t)p->side * p->side * p->side * 3; }
};
// everything the kernels will dereference, checked before anything is touched
static bool implicit_args_ok(const ImplicitArgs &a, bool needGrid) {
  if (!a.p || !a.tab) return false;
  if (a.p->side != 4 && a.p->side != 8) return false;
  if (a.p->model < ZS_MPM_FIXED_COROTATED || a.p->model > ZS_MPM_EQUATION_OF_STATE) return false;
  if (!(a.p->dx > 0.f)) return false;
  if (needGrid && !a.grid) return false;
  if (a.ps.n && (!a.ps.pos.base || !a.ps.F.base)) return false;
  if (a.ps.n && model_uses_logjp(a.p->model) && !a.ps.logJp.base) return false;
  if (a.ps.n > (size_t)0x7fffff00) return false;  // particle indices are ints in the bins
  if ((a.binStart || a.cellCount || a.nbr) && !a.binned()) return false;  // the three arrays of the binned path come together
  return true;
}

// stale: ints for ps.n + 64 (binned path only)
static void implicit_force(Launch &L, const ImplicitArgs &a, const float *vIn, float *fOut, float *trial, int *stale) {
  if (!a.ps.n || !a.nblocks) return;
  MpmDev mp = make_dev(a.p);
  ParticlesDev pd = make_particles(a.ps);
  BhtDev t = a.tab->t.dev();
  const zs_rocm_particles &ps = a.ps;
  const int model = a.p->model;
  if (a.binned()) {
    int *staleCount = stale + ps.n + 32;
    ZSR_CHECK(hipMemsetAsync(staleCount, 0, sizeof(int), L.stream));
    // (mass, vel, C are not read: the layout check looks at the attributes the kernel loads)
    zs_rocm_particles used = ps;
    used.mass = used.vel = used.C = ps.pos;
    const int lw = uniform_lane_width(used, model_uses_logjp(model), false);
    const unsigned nb = (unsigned)a.nblocks;
    const int *binStart = a.binStart, *nbr = a.nbr;
    const unsigned *cellCount = a.cellCount;
#define CALL_IMPL_BLOCK3(S, M, LWv)                                                                                                      \
  do {                                                                                                                                   \
    hipLaunchKernelGGL((implicit_block_kernel<S, M, LWv>), dim3(nb), dim3(S == 8 ? 256 : 64), 0, L.stream, mp, pd, t, vIn, fOut, trial,  \
                       binStart, cellCount, nbr, stale, staleCount);                                                                     \
    hipLaunchKernelGGL((implicit_stale_kernel<S, M>), dim3(STALE_BLOCKS), dim3(256), 0, L.stream, mp, pd, t, vIn, fOut, trial,           \
                       (const int *)stale, (const int *)staleCount);                                                                     \
  } while (0)
#define CALL_IMPL_BLOCK(S, M) ZSR_DISPATCH_LW(lw, CALL_IMPL_BLOCK3, S, M)
    ZSR_DISPATCH_SIDE_PURE(a.p->side, model, CALL_IMPL_BLOCK);
  } else {
#define CALL_IMPL_GLOBAL(S, M) \
  hipLaunchKernelGGL((implicit_global_kernel<S, M>), dim3(ceil_div(ps.n, 256)), dim3(256), 0, L.stream, mp, pd, t, vIn, fOut, trial)
    ZSR_DISPATCH_SIDE_PURE(a.p->side, model, CALL_IMPL_GLOBAL);
  }
}

static void implicit_multiply(Launch &L, const ImplicitArgs &a, const float *vIn, float *out, int *stale) {
  const size_t ne = a.entries();
  if (!ne) return;
  ZSR_CHECK(hipMemsetAsync(out, 0, ne * sizeof(float), L.stream));  // DofFill{out, 0} (ImplicitMPM.hpp:47)
  implicit_force(L, a, vIn, out, nullptr, stale);
  if (a.p->side == 4) hipLaunchKernelGGL((implicit_mass_kernel<4>), dim3(ceil_div(ne, 256)), dim3(256), 0, L.stream, a.grid, vIn, out, ne, a.p->dt);
  else hipLaunchKernelGGL((implicit_mass_kernel<8>), dim3(ceil_div(ne, 256)), dim3(256), 0, L.stream, a.grid, vIn, out, ne, a.p->dt);
}
static void implicit_precondition(Launch &L, const float *grid, size_t nblocks, int side, const float *in, float *out) {
  const size_t ne = nblocks * (size_t)side * side * side * 3;
  if (!ne) return;
  if (side == 4) hipLaunchKernelGGL((implicit_precondition_kernel<4>), dim3(ceil_div(ne, 256)), dim3(256), 0, L.stream, grid, in, out, ne);
  else hipLaunchKernelGGL((implicit_precondition_kernel<8>), dim3(ceil_div(ne, 256)), dim3(256), 0, L.stream, grid, in, out, ne);
}
// the shape of the projection's collider: none (the collider's own analytic shape), a level set, or a transition between two
struct BoundaryShape {
  const zs_rocm_levelset *levelset = nullptr;
  const zs_rocm_levelset_transition *transition = nullptr;
  explicit operator bool() const { return levelset || transition; }
};
// shape set: `collider` gives type and motion only (the grid is only read there too)
// false: the transition kernel could not be launched
static bool implicit_project(Launch &L, const ImplicitArgs &a, const zs_rocm_collider *collider, const BoundaryShape &shape, float *inout) {
  const int *keys = (const int *)a.tab->t.dev().activeKeys;
  const zs_rocm_levelset *levelset = shape.levelset;
  if (shape.transition) return transition_blocks_enqueue(L.stream, a.p, keys, const_cast<float *>(a.grid), a.nblocks, collider, shape.transition, inout);
  if (levelset) levelset_blocks_enqueue(L.stream, a.p, keys, const_cast<float *>(a.grid), a.nblocks, collider, levelset, inout);
  else implicit_project_enqueue(L.stream, a.p, keys, a.grid, a.nblocks, collider, inout);
  return true;
}
// a level set or a transition comes with a collider (type and motion); neither: no boundary
static bool boundary_ok(const zs_rocm_collider *collider, const BoundaryShape &shape) {
  if (shape.transition) return transition_collider_ok(collider, shape.transition);
  return shape.levelset ? levelset_collider_ok(collider, shape.levelset) : true;
}

}  // namespace zsr

using namespace zsr;

extern "C" {

int zs_rocm_mpm_implicit_force(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, zs_rocm_particles ps, const zs_rocm_bht_3 *tab, size_t nblocks,
                               const int *binStart, const unsigned *cellCount, const int *nbr, const float *vIn, float *fOut, float *trial) {
  const ImplicitArgs a{p, ps, tab, nullptr, nblocks, binStart, cellCount, nbr};
  if (!pol || !implicit_args_ok(a, false) || !vIn || !fOut) return -1;
  Launch L(pol, "G2P2GTransfer");
  int *stale = a.binned() && ps.n && nblocks ? (int *)L.temp(sizeof(int) * (ps.n + 64)) : nullptr;
  implicit_force(L, a, vIn, fOut, trial, stale);
  return 0;
}

int zs_rocm_mpm_implicit_multiply(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, zs_rocm_particles ps, const zs_rocm_bht_3 *tab,
                                  const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount, const int *nbr,
                                  const float *vIn, float *out) {
  const ImplicitArgs a{p, ps, tab, grid, nblocks, binStart, cellCount, nbr};
  if (!pol || !implicit_args_ok(a, true) || !vIn || !out || vIn == out) return -1;
  Launch L(pol, "ImplicitMPMSystem::multiply");
  int *stale = a.binned() && ps.n && nblocks ? (int *)L.temp(sizeof(int) * (ps.n + 64)) : nullptr;
  implicit_multiply(L, a, vIn, out, stale);
  return 0;
}

static int implicit_project_entry(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, const zs_rocm_bht_3 *tab, const float *grid, size_t nblocks,
                                  const zs_rocm_collider *collider, const BoundaryShape &levelset, float *inout) {
  if (!pol || !p || !tab || !grid || !inout || (p->side != 4 && p->side != 8) || !(p->dx > 0.f)) return -1;
  if (!boundary_ok(collider, levelset) || nblocks > (size_t)0x7fffffff) return -1;
  Launch L(pol, "ImplicitMPMSystem::project");
  const ImplicitArgs a{p, zs_rocm_particles{}, tab, grid, nblocks, nullptr, nullptr, nullptr};
  return implicit_project(L, a, collider, levelset, inout) ? 0 : -1;
}
int zs_rocm_mpm_implicit_project(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, const zs_rocm_bht_3 *tab, const float *grid, size_t nblocks,
                                 const zs_rocm_collider *collider, float *inout) {
  return implicit_project_entry(pol, p, tab, grid, nblocks, collider, BoundaryShape{}, inout);
}
int zs_rocm_mpm_implicit_project_levelset(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, const zs_rocm_bht_3 *tab, const float *grid,
                                          size_t nblocks, const zs_rocm_collider *collider, const zs_rocm_levelset *levelset, float *inout) {
  if (!levelset && collider) return -1;  // (a collider alone is zs_rocm_mpm_implicit_project's)
  return implicit_project_entry(pol, p, tab, grid, nblocks, collider, BoundaryShape{levelset, nullptr}, inout);
}
int zs_rocm_mpm_implicit_project_transition(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, const zs_rocm_bht_3 *tab, const float *grid,
                                            size_t nblocks, const zs_rocm_collider *collider, const zs_rocm_levelset_transition *transition,
                                            float *inout) {
  if (!transition) return -1;
  return implicit_project_entry(pol, p, tab, grid, nblocks, collider, BoundaryShape{nullptr, transition}, inout);
}

int zs_rocm_mpm_implicit_precondition(zs_rocm_policy *pol, const float *grid, size_t nblocks, int side, const float *in, float *out) {
  if (!pol || !grid || !in || !out || (side != 4 && side != 8)) return -1;
  Launch L(pol, "ImplicitMPMSystem::precondition");
  implicit_precondition(L, grid, nblocks, side, in, out);
  return 0;
}

// (the void dof calls cannot report a refusal: with a NULL policy or vector they return without touching anything)
void zs_rocm_dof_assign(zs_rocm_policy *pol, const float *a, float *b, size_t n) {
  if (!pol || !a || !b) return;
  Launch L(pol, "DofAssign");
  dof_assign(L, a, b, n);
}
void zs_rocm_dof_fill(zs_rocm_policy *pol, float *a, float v, size_t n) {
  if (!pol || !a) return;
  Launch L(pol, "DofFill");
  dof_fill(L, a, v, n);
}
int zs_rocm_dof_compwise(zs_rocm_policy *pol, int op, const float *a, const float *b, float *c, size_t n) {
  if (!pol || !a || !b || !c || op < DOF_PLUS || op > DOF_DIVIDES) return -1;
  Launch L(pol, "DofCompwiseOp");
  dof_compwise(L, op, a, b, c, n);
  return 0;
}
void zs_rocm_dof_linear_combine(zs_rocm_policy *pol, float m, const float *a, float n_, const float *b, float *c, size_t n) {
  if (!pol || !a || !b || !c) return;
  Launch L(pol, "LinearCombineOp");
  dof_linear_combine(L, m, a, n_, b, c, n);
}
void zs_rocm_dof_dot(zs_rocm_policy *pol, const float *a, const float *b, size_t n, float *out) {
  if (!pol || !a || !b || !out) return;
  Launch L(pol, "dotProduct");
  float *partials = (float *)L.temp(sizeof(float) * DOT_MAX_BLOCKS);
  dof_dot(L, a, b, n, partials, out);
}

// the CG driver of both solve entries
static int implicit_solve(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, zs_rocm_particles ps, const zs_rocm_bht_3 *tab, const float *grid,
                          size_t nblocks, const int *binStart, const unsigned *cellCount, const int *nbr, const zs_rocm_collider *collider,
                          const BoundaryShape &levelset, const float *b, float *x, int maxIters, float tol, float relTol, int *iters) {
  const ImplicitArgs a{p, ps, tab, grid, nblocks, binStart, cellCount, nbr};
  if (!pol || !implicit_args_ok(a, true) || !b || !x || b == x || maxIters < 0) return -1;
  if (!boundary_ok(collider, levelset) || nblocks > (size_t)0x7fffffff) return -1;
  if (iters) *iters = 0;
  const size_t ne = a.entries();
  if (!ne || maxIters == 0) return 0;  // the reference's loop does not run either and x = xinout comes back as it went in
  Launch L(pol, "ConjugateGradient::solve");
  // work vectors r, p, q, temp + the dot product's partial sums and two scalars, all from the stream's temporary arena, once
  const size_t nev = (ne + 63) & ~(size_t)63;
  float *work = (float *)L.temp(sizeof(float) * (4 * nev + DOT_MAX_BLOCKS + 64));
  float *r = work, *pv = work + nev, *q = work + 2 * nev, *temp = work + 3 * nev, *partials = work + 4 * nev, *scalar = partials + DOT_MAX_BLOCKS;
  int *stale = a.binned() && ps.n ? (int *)L.temp(sizeof(int) * (ps.n + 64)) : nullptr;
  // (the reference copies xinout into a member x_ first and back at the end, :77,160: x is updated in place here)
  implicit_multiply(L, a, x, temp, stale);
  dof_compwise(L, DOF_MINUS, b, temp, r, ne);  // r = b - A x
  if (!implicit_project(L, a, collider, levelset, r)) return -1;
  dof_assign(L, r, q, ne);                     // (entries without mass: q keeps r there, which the projection has zeroed)
  implicit_precondition(L, grid, nblocks, p->side, r, q);
  dof_assign(L, q, pv, ne);
  dof_dot(L, r, q, ne, partials, scalar);
  float zTrk = read_back(L, scalar);
  float resNorm = sqrtf(zTrk);
  const float localTol = fminf(relTol * resNorm, tol);
  int iter = 0;
  for (; iter != maxIters; ++iter) {
    if (resNorm <= localTol) break;
    implicit_multiply(L, a, pv, temp, stale);
    if (!implicit_project(L, a, collider, levelset, temp)) return -1;
    dof_dot(L, temp, pv, ne, partials, scalar);
    const float alpha = zTrk / read_back(L, scalar);
    dof_linear_combine(L, alpha, pv, 1.f, x, x, ne);      // x = x + alpha p
    dof_linear_combine(L, -alpha, temp, 1.f, r, r, ne);   // r = r - alpha temp
    implicit_precondition(L, grid, nblocks, p->side, r, q);
    const float zTrkLast = zTrk;
    dof_dot(L, q, r, ne, partials, scalar);
    zTrk = read_back(L, scalar);
    const float beta = zTrk / zTrkLast;
    dof_linear_combine(L, beta, pv, 1.f, q, pv, ne);      // p = q + beta p
    resNorm = sqrtf(zTrk);
  }
  if (iters) *iters = iter;
  return 0;
}
int zs_rocm_mpm_implicit_solve(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, zs_rocm_particles ps, const zs_rocm_bht_3 *tab,
                               const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount, const int *nbr,
                               const zs_rocm_collider *collider, const float *b, float *x, int maxIters, float tol, float relTol, int *iters) {
  return implicit_solve(pol, p, ps, tab, grid, nblocks, binStart, cellCount, nbr, collider, BoundaryShape{}, b, x, maxIters, tol, relTol, iters);
}
int zs_rocm_mpm_implicit_solve_levelset(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, zs_rocm_particles ps, const zs_rocm_bht_3 *tab,
                                        const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount, const int *nbr,
                                        const zs_rocm_collider *collider, const zs_rocm_levelset *levelset, const float *b, float *x,
                                        int maxIters, float tol, float relTol, int *iters) {
  if (!levelset && collider) return -1;  // (a collider alone is zs_rocm_mpm_implicit_solve's)
  return implicit_solve(pol, p, ps, tab, grid, nblocks, binStart, cellCount, nbr, collider, BoundaryShape{levelset, nullptr}, b, x, maxIters, tol,
                        relTol, iters);
}
int zs_rocm_mpm_implicit_solve_transition(zs_rocm_policy *pol, const zs_rocm_mpm_params *p, zs_rocm_particles ps, const zs_rocm_bht_3 *tab,
                                          const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount, const int *nbr,
                                          const zs_rocm_collider *collider, const zs_rocm_levelset_transition *transition, const float *b,
                                          float *x, int maxIters, float tol, float relTol, int *iters) {
  if (!transition) return -1;
  return implicit_solve(pol, p, ps, tab, grid, nblocks, binStart, cellCount, nbr, collider, BoundaryShape{nullptr, transition}, b, x, maxIters,
                        tol, relTol, iters);
}

}  // extern "C"
