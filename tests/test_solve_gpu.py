"""The mesh Newton system on the device (zpc_amd/mesh_solve.py, zpc_amd/csrc/mesh_solve.hip) against the existing public products, the
float32 replay and the float64 reference of tests/ref64_solve.py.

Scenes: ref64_proximity.SCENES, the strips with nv = 255, 256, 258 and 3 nv = 4095, 4098 (the 256-lane boundaries of the vertex kernels and
the 4096-entry boundary of a vector), `fan` for the long hub run.  Trial positions: displaced(.., 1e-1) and compressed(.., 0.5), so that
the psd projection acts; u is a small displacement.

1  per-term blocks == hx[v] of the public *_hessian_product(.., psd=True) at x = e_{v,j}, value for value (every vertex under 300
   vertices, 64 sampled ones with the ends on the strips);
2  combined blocks, inverse and the fallback / fixed-mass counts bit for bit with the float32 replay;
3  multiply bit for bit with the replay -- ref64_terms.gather over the elem_terms / pair_terms of the public product calls plus the epilogue
   -- for every subset of terms, with fixed vertices and a non-positive mass;
4  solve: x, iters, flag and the residual history bit for bit with the replay, the same bytes for check_every 1, 3, 8 and on a second
   call; max_iters = 0 returns x0; a negative scale reaches the breakdown flag;
5  against truth on tiny2 and sheets5 at rel_tol = 1e-2: the true preconditioned residual of the device's x against the dense float64
   matrix is at most twice that of the float64 PCG.  Measured on an MI355X: see the test's docstring;
6  descent on sheets: g . d < 0 and the composed float64 energy decreases at the largest t = 2^-k under max_step;
7  the argument checks.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import ref64_elastic as rl
import ref64_proximity as rp
import ref64_solve as rs
import ref64_terms as rt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STRIPS = ("strip14x16", "strip1x127", "strip1x128", "strip14x90", "strip1x682")
NAMES = rp.SCENES + STRIPS
POSITIONS = ("displaced", "compressed")
TERMS = ("elastic", "barrier", "friction")


def _np(x):
    return None if x is None else x.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _scene(name):
    v, t, dhat = rs.scene(name)
    return v, np.asarray(t, np.int32).reshape(-1, 3), dhat


@functools.lru_cache(maxsize=None)
def _position(name, which):
    v, t, _ = _scene(name)
    return rl.displaced(v, t, 1, 1e-1) if which == "displaced" else rl.compressed(v, 0.5)


class Case:
    """a mesh with rest shape, rest lengths, proximity lists and lagged friction at the rest positions, masses from the vertex areas, and
    the element vertex lists with their incidences for the replay; built once per scene"""

    def __init__(self, pol, name):
        from zpc_amd.mesh import TriMesh
        self.name = name
        self.v, self.t, self.dhat = _scene(name)
        self.nv = len(self.v)
        self.mesh = mesh = TriMesh(pol, self.v, self.t)
        mesh.set_rest()
        mesh.set_rest_shape()
        self.prox = mesh.proximity(self.dhat)
        self.lag = mesh.friction_lag(self.prox, self.dhat, rs.KAPPA)
        _, hinges, _, area = mesh.rest_shape()
        self.mass = (np.float32(rs.DENSITY) * _np(area)).astype(np.float32)
        self.u = rs.small_displacement(self.nv)
        t64, e = self.t.astype(np.int64), _np(mesh.edges()).astype(np.int64)
        pt, ee = _np(self.prox.pt_pairs).astype(np.int64), _np(self.prox.ee_pairs).astype(np.int64)
        self.pt, self.ee = pt, ee
        vert = np.concatenate([np.concatenate([pt[:, :1], t64[pt[:, 1]]], axis=1), np.concatenate([e[ee[:, 0]], e[ee[:, 1]]], axis=1)]).reshape(-1, 4)
        self.inc = dict(tri=rt.incidence(t64, self.nv), hinge=rt.incidence(_np(hinges).astype(np.int64).reshape(-1, 4), self.nv),
                        pair=rt.incidence(vert, self.nv))

    def system(self, terms=TERMS, mass=None, fixed=None, scale=rs.SCALE):
        from zpc_amd.mesh_solve import MeshSystem
        return MeshSystem(self.mesh, self.mass if mass is None else mass, scale, elastic=(rs.MU, rs.LAM, rs.KB) if "elastic" in terms else None,
                          barrier=(self.prox, self.dhat, rs.KAPPA) if "barrier" in terms else None,
                          friction=(self.lag, rs.FRICTION_MU, rs.EPS_V) if "friction" in terms else None, fixed=fixed)

    def products(self, x, verts, terms=TERMS):
        """the three public product calls (psd) for the direction x at verts: dict term -> result"""
        m, out = self.mesh, {}
        if "elastic" in terms:
            out["elastic"] = m.elastic_hessian_product(rs.MU, rs.LAM, rs.KB, x, verts=verts, psd=True)
        if "barrier" in terms:
            out["barrier"] = m.barrier_hessian_product(self.prox, self.dhat, rs.KAPPA, x, verts=verts, psd=True)
        if "friction" in terms:
            out["friction"] = m.friction_hessian_product(self.lag, self.u, rs.FRICTION_MU, rs.EPS_V, x)
        return out

    def runs(self, verts, terms=TERMS):
        """x -> the runs of the replay's gather, from the per-element terms the public product calls leave on the device"""
        def of(x):
            r, out = self.products(np.asarray(x, np.float32), verts, terms), []
            if "elastic" in terms:
                out += [self.inc["tri"] + (_np(r["elastic"].tri_terms).reshape(-1, 3),), self.inc["hinge"] + (_np(r["elastic"].hinge_terms).reshape(-1, 3),)]
            for k in ("barrier", "friction"):
                if k in terms:
                    out.append(self.inc["pair"] + (_np(r[k].pair_terms).reshape(-1, 3),))
            return out
        return of


_cases = {}


def _case(pol, name):
    if name not in _cases:
        _cases[name] = Case(pol, name)
    return _cases[name]


def _sample(case):
    if not case.name.startswith("strip"):
        return np.arange(case.nv)
    pick = np.random.default_rng(7).choice(case.nv, 62, replace=False)
    return np.unique(np.concatenate([[0, case.nv - 1], pick]))


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("which", POSITIONS)
@pytest.mark.parametrize("name", NAMES)
def test_per_term_blocks_equal_the_public_products_at_unit_directions(pol, name, which):
    c = _case(pol, name)
    verts = _position(name, which)
    S = c.system()
    S.linearize(verts, c.u)
    B = S.blocks()
    sample = _sample(c)
    x = torch.zeros(c.nv, 3, dtype=torch.float32, device="cuda")
    want = {k: [] for k in TERMS}
    for v in sample.tolist():
        for j in range(3):
            x[v, j] = 1
            r = c.products(x, verts)
            for k in TERMS:
                want[k].append(r[k].hx[v].clone())
            x[v, j] = 0
    for k in TERMS:
        hx = torch.stack(want[k]).cpu().numpy().reshape(len(sample), 3, 3)      # [vertex, j, i]
        ref = np.stack([hx[:, j, i] for i, j in rs.SLOT], axis=1)
        got = _np(getattr(B, k))[sample]
        assert np.array_equal(got, ref), (k, np.abs(got - ref).max())
    if name in ("sheets", "fan", "stack", "strip14x16"):
        assert all(np.abs(_np(getattr(B, k))).max() > 0 for k in TERMS)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("which", POSITIONS)
@pytest.mark.parametrize("name", NAMES)
def test_combined_blocks_and_inverse_bit_for_bit_with_the_replay(pol, name, which):
    c = _case(pol, name)
    fixed = np.zeros(c.nv, np.uint8)
    fixed[::5] = 1
    mass = c.mass.copy()
    mass[1::7] = (0, -1, np.nan, np.inf)[len(name) % 4]
    for scale, m, fx in ((rs.SCALE, c.mass, None), (rs.SCALE, mass, fixed), (1e12, c.mass, None)):
        S = c.system(mass=m, fixed=fx, scale=scale)
        counts = S.linearize(_position(name, which), c.u)
        B = S.blocks()
        D = rs.combine(_np(B.elastic), _np(B.barrier), _np(B.friction), scale, m, np.float32)
        inv, fallbacks, bad = rs.precondition(D, m, fx, np.float32)
        assert _same(_np(B.combined), D) and _same(_np(B.inverse), inv)
        assert (counts.inverse_fallbacks, counts.fixed_masses) == (fallbacks, bad)
        if scale == 1e12 and name == "sheets":
            assert fallbacks > 0
        if fx is not None:
            assert bad >= len(mass[1::7]) and not _np(B.inverse)[::5].any()      # (a vertex without a triangle has no mass either)


# ------------------------------------------------------------------------------------------------ 3
def _multiply_replay(c, verts, terms, mass, fixed, scale=rs.SCALE):
    return rs.operator(c.runs(verts, terms), mass, scale, fixed, np.float32)


@pytest.mark.parametrize("which", POSITIONS)
@pytest.mark.parametrize("name", NAMES)
def test_multiply_bit_for_bit_with_the_replay_for_every_subset_of_terms(pol, name, which):
    c = _case(pol, name)
    verts = _position(name, which)
    x = np.random.default_rng(77).standard_normal((c.nv, 3)).astype(np.float32)
    fixed = np.zeros(c.nv, np.uint8)
    fixed[2::5] = 1
    mass = c.mass.copy()
    mass[::9] = 0
    for n in range(4):
        for terms in itertools.combinations(TERMS, n):
            for m, fx in ((c.mass, None), (mass, fixed)):
                S = c.system(terms, mass=m, fixed=fx)
                S.linearize(verts, c.u)
                q = _np(S.multiply(x))
                assert _same(q, _multiply_replay(c, verts, terms, m, fx)(x)), terms
                if fx is not None:
                    assert not q[2::5].any() and not q[::9].any()


def test_the_friction_lists_may_differ_from_the_barrier_lists(pol):
    c = _case(pol, "sheets")
    from zpc_amd.mesh_solve import MeshSystem
    near = c.mesh.proximity(0.6 * c.dhat)
    assert 0 < len(near.pt_pairs) < len(c.prox.pt_pairs)
    verts = _position("sheets", "displaced")
    S = MeshSystem(c.mesh, c.mass, rs.SCALE, barrier=(near, c.dhat, rs.KAPPA), friction=dict(lag=c.lag, mu=rs.FRICTION_MU, eps_v=rs.EPS_V))
    S.linearize(verts, c.u)
    x = np.random.default_rng(78).standard_normal((c.nv, 3)).astype(np.float32)
    hb = c.mesh.barrier_hessian_product(near, c.dhat, rs.KAPPA, x, verts=verts, psd=True).hx
    hf = c.mesh.friction_hessian_product(c.lag, c.u, rs.FRICTION_MU, rs.EPS_V, x).hx
    want = torch.from_numpy(c.mass).cuda()[:, None] * torch.from_numpy(x).cuda() + np.float32(rs.SCALE) * (hb + hf)
    got = S.multiply(x)
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("which", POSITIONS)
@pytest.mark.parametrize("name", NAMES)
def test_solve_bit_for_bit_with_the_replay_whatever_check_every(pol, name, which):
    c = _case(pol, name)
    verts = _position(name, which)
    fixed = np.zeros(c.nv, np.uint8)
    fixed[3::11] = 1
    S = c.system(fixed=fixed)
    S.linearize(verts, c.u)
    g = np.random.default_rng(79)
    b, x0 = g.standard_normal((c.nv, 3)).astype(np.float32), (1e-3 * g.standard_normal((c.nv, 3))).astype(np.float32)
    kw = dict(max_iters=10, rel_tol=1e-3)
    want = rs.pcg(_multiply_replay(c, verts, TERMS, c.mass, fixed), _np(S.blocks().inverse), b, x0, dtype=np.float32, **kw)
    first = None
    for check_every in (1, 3, 8, 8):
        r = S.solve(b, x0, check_every=check_every, **kw)
        got = (_np(r.x), r.iters, r.flag, r.residuals)
        assert _same(got[0], want["x"]) and got[1:3] == (want["iters"], want["flag"]) and _same(got[3], want["residuals"]), check_every
        assert len(r.residuals) == r.iters + 1 and np.array_equal(got[0][3::11], x0[3::11])
        first = first or got
        assert _same(got[0], first[0]) and _same(got[3], first[3])
    r = S.solve(b, x0, max_iters=0)
    # (max_iters unless the start is the solution already: a scene without triangles has no mass, every vertex is fixed and res0 = 0)
    none = rs.pcg(_multiply_replay(c, verts, TERMS, c.mass, fixed), _np(S.blocks().inverse), b, x0, 0, rel_tol=1e-3, dtype=np.float32)
    assert _same(_np(r.x), x0) and r.iters == 0 and _same(r.residuals, none["residuals"]) and len(r.residuals) == 1
    assert r.flag == none["flag"] == ("converged" if name == "tiny0" else "max_iters")


def test_solve_converges_and_a_negative_scale_breaks_down(pol):
    c = _case(pol, "sheets")
    verts = _position("sheets", "displaced")
    b = np.random.default_rng(80).standard_normal((c.nv, 3)).astype(np.float32)
    S = c.system()
    S.linearize(verts, c.u)
    r = S.solve(b, max_iters=400, rel_tol=1e-4)
    assert r.flag == "converged" and 0 < r.iters < 400 and r.residuals[-1] <= 1e-4 * r.residuals[0]
    want = rs.pcg(_multiply_replay(c, verts, TERMS, c.mass, None), _np(S.blocks().inverse), b, None, 400, rel_tol=1e-4, dtype=np.float32)
    assert _same(_np(r.x), want["x"]) and r.iters == want["iters"] and _same(r.residuals, want["residuals"])
    N = c.system(scale=-1e3 * rs.SCALE)
    N.linearize(verts, c.u)
    r = N.solve(b, max_iters=50)
    want = rs.pcg(_multiply_replay(c, verts, TERMS, c.mass, None, -1e3 * rs.SCALE), _np(N.blocks().inverse), b, None, 50, dtype=np.float32)
    assert r.flag == "breakdown" == want["flag"] and r.iters == want["iters"] and _same(_np(r.x), want["x"])


# ------------------------------------------------------------------------------------------------ 5
def _reference64(c, verts):
    """the float64 system on the device's own lists and records"""
    rest2 = _np(c.mesh.rest())
    S = rs.System(c.v, c.t, c.mass, rs.SCALE, elastic=(rs.MU, rs.LAM, rs.KB), barrier=dict(pt=c.pt, ee=c.ee, dhat=c.dhat, kappa=rs.KAPPA, rest2=rest2),
                  friction=dict(pt=c.pt, ee=c.ee, record=_np(c.lag.record), mu=rs.FRICTION_MU, eps_v=rs.EPS_V), dtype=np.float64)
    S.linearize(verts, c.u)
    return S


@pytest.mark.parametrize("name", rs.SMALL)
def test_the_true_residual_against_the_float64_matrix(pol, name):
    """MI355X: tiny2 device 2.4696e-03 (11 iterations) / float64 2.4694e-03 (11 iterations) of res0 7.1188e-01; sheets5 device 1.2490e-02 (15
    iterations) / float64 1.2501e-02 (15 iterations) of res0 1.7427e+00: the float32 recurrence drifts by 1e-4 to 1e-3 of the residual at
    this tolerance, far below the factor of 2"""
    c = _case(pol, name)
    verts = _position(name, "displaced")
    R = _reference64(c, verts)
    A = R.dense()
    assert np.abs(A - A.T).max() <= 1e-8 * np.abs(A).max() and np.linalg.eigvalsh(0.5 * (A + A.T))[0] > 0
    inv64 = R.blocks()["inverse"]
    b = np.random.default_rng(81).standard_normal((c.nv, 3)).astype(np.float32)

    def true_residual(x):
        r = b.astype(np.float64) - (A @ np.asarray(x, np.float64).reshape(-1)).reshape(-1, 3)
        return float(np.sqrt((r * rs.apply_block(inv64, r)).sum()))
    S = c.system()
    S.linearize(verts, c.u)
    dev = S.solve(b, max_iters=400, rel_tol=1e-2)
    ref = rs.pcg(R.multiply, inv64, b, None, 400, rel_tol=1e-2, dtype=np.float64)
    res_dev, res_ref = true_residual(_np(dev.x)), true_residual(ref["x"])
    print("%s: true preconditioned residual device %.4e (%d iterations) / float64 %.4e (%d iterations) of res0 %.4e"
          % (name, res_dev, dev.iters, res_ref, ref["iters"], true_residual(np.zeros_like(b))))
    assert dev.flag == "converged" and ref["flag"] == "converged"
    assert res_dev <= 2 * res_ref


# ------------------------------------------------------------------------------------------------ 6
def test_the_newton_direction_descends_on_sheets(pol):
    c = _case(pol, "sheets")
    m, verts = c.mesh, _position("sheets", "displaced")
    ge = m.elastic(rs.MU, rs.LAM, rs.KB, verts=verts).grad
    gb = m.barrier(c.prox, c.dhat, rs.KAPPA, verts=verts).grad
    gf = m.friction(c.lag, c.u, rs.FRICTION_MU, rs.EPS_V).grad
    g = np.float32(rs.SCALE) * (ge + gb + gf)
    S = c.system()
    S.linearize(verts, c.u)
    r = S.solve(-g, max_iters=400, rel_tol=1e-3)
    assert r.flag == "converged"
    d, g64 = _np(r.x).astype(np.float64), _np(g).astype(np.float64)
    assert (g64 * d).sum() < 0
    bound = float(m.max_step(c.prox, r.x, verts=verts).t.item())
    assert bound > 0
    t = 1.0
    while t >= bound:
        t *= 0.5
    R = _reference64(c, verts)
    mass = c.mass.astype(np.float64)

    def energy(s):
        # the incremental potential about verts: the inertia term is zero there, h^2 times the three potentials
        step = s * d
        return 0.5 * float((mass[:, None] * step * step).sum()) + rs.SCALE * R.energy(verts.astype(np.float64) + step, c.u.astype(np.float64) + step)
    e0, e1 = energy(0.0), energy(t)
    print("sheets: g . d = %.4e, t = %g (max_step %.4g), energy %.9e -> %.9e" % ((g64 * d).sum(), t, bound, e0, e1))
    assert e1 < e0


# ------------------------------------------------------------------------------------------------ 7
def test_the_argument_checks(pol, hiplib):
    from zpc_amd._lib import MeshSystemDesc
    from zpc_amd.mesh import TriMesh
    from zpc_amd.mesh_solve import MeshSystem
    c = _case(pol, "tiny2")
    ok = dict(elastic=(rs.MU, rs.LAM, rs.KB), barrier=(c.prox, c.dhat, rs.KAPPA), friction=(c.lag, rs.FRICTION_MU, rs.EPS_V))
    for bad in (dict(mass=c.mass[:-1]), dict(scale=float("nan")), dict(fixed=np.zeros(c.nv + 1, np.uint8)), dict(elastic=(-1.0, 0.0, 0.0)),
                dict(elastic=(1.0, 2.0)), dict(barrier=(c.prox, -1.0, 1.0)), dict(barrier=(c.lag, c.dhat, 1.0)), dict(friction=(c.prox, 0.3, 1e-3)),
                dict(friction=(c.lag, -0.1, 1e-3)), dict(friction=(c.lag, 0.3, 0.0)), dict(friction=dict(lag=c.lag, mu=0.3))):
        kw = dict(dict(mass=c.mass, scale=rs.SCALE), **ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            MeshSystem(c.mesh, kw.pop("mass"), kw.pop("scale"), **kw)
    bare = TriMesh(pol, c.v, c.t)
    with pytest.raises(ValueError):
        MeshSystem(bare, c.mass, rs.SCALE, elastic=ok["elastic"])      # no rest shape
    S = c.system()
    x = np.zeros((c.nv, 3), np.float32)
    for call in (S.blocks, lambda: S.multiply(x), lambda: S.solve(x)):
        with pytest.raises(ValueError):
            call()                                                     # before linearize
    with pytest.raises(ValueError):
        S.linearize(c.v)                                               # friction needs u
    with pytest.raises(ValueError):
        S.linearize(c.v[:-1], c.u)
    S.linearize(c.v, c.u)
    for bad in (x[:-1], np.zeros((c.nv, 2), np.float32)):
        with pytest.raises(ValueError):
            S.multiply(bad)
        with pytest.raises(ValueError):
            S.solve(bad)
    for kw in (dict(max_iters=-1), dict(check_every=0), dict(tol=-1.0), dict(rel_tol=-1.0), dict(x0=x[:-1])):
        with pytest.raises(ValueError):
            S.solve(x, **kw)
    assert S.multiply(np.zeros((c.nv, 3), np.float64)).dtype == torch.float32      # other float types are converted
    # lists that changed since the incidence was built
    other = _case(pol, "sheets5")
    prox = c.mesh.proximity(c.dhat)
    lag = c.mesh.friction_lag(prox, c.dhat, rs.KAPPA)
    T = MeshSystem(c.mesh, c.mass, rs.SCALE, barrier=(prox, c.dhat, rs.KAPPA), friction=(lag, rs.FRICTION_MU, rs.EPS_V))
    T.linearize(c.v, c.u)
    kept = prox.pt_pairs
    prox.pt_pairs = other.prox.pt_pairs
    for call in (lambda: T.linearize(c.v, c.u), T.blocks, lambda: T.multiply(x), lambda: T.solve(x)):
        with pytest.raises(ValueError):
            call()
    prox.pt_pairs = kept
    T.multiply(x)
    # the C entries: -1 and nothing written
    d = MeshSystemDesc()
    C.memmove(C.byref(d), C.byref(S._desc), C.sizeof(d))
    h, mh, by = pol.handle, c.mesh.handle, C.byref
    sizes = (C.c_size_t * 3)()
    assert hiplib.zs_rocm_mesh_system_sizes(mh, by(d), sizes) == 0 and sizes[2] == c.nv and sizes[1] >= sizes[0] > 0
    assert hiplib.zs_rocm_mesh_system_sizes(None, by(d), sizes) == -1 and hiplib.zs_rocm_mesh_system_sizes(mh, None, sizes) == -1
    assert hiplib.zs_rocm_mesh_system_sizes(mh, by(d), None) == -1
    f32 = dict(dtype=torch.float32, device="cuda")
    scratch = torch.zeros(int(sizes[1]), **f32)
    blk = [torch.full((c.nv, 6), 7.0, **f32) for _ in range(5)]
    q = torch.full((c.nv, 3), 7.0, **f32)
    xd, bd = torch.zeros(c.nv, 3, **f32), torch.ones(c.nv, 3, **f32)
    rec = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    blocks = lambda pol_, m_, d_, s_, outs: hiplib.zs_rocm_mesh_system_blocks(pol_, m_, d_, s_, *outs, None)
    outs = [p(t) for t in blk]
    assert blocks(None, mh, by(d), p(scratch), outs) == -1 and blocks(h, None, by(d), p(scratch), outs) == -1
    assert blocks(h, mh, None, p(scratch), outs) == -1 and blocks(h, mh, by(d), None, outs) == -1
    for k in range(5):
        assert blocks(h, mh, by(d), p(scratch), outs[:k] + [None] + outs[k + 1:]) == -1
    mul = hiplib.zs_rocm_mesh_system_multiply
    assert mul(None, mh, by(d), p(scratch), p(xd), p(q)) == -1 and mul(h, mh, by(d), None, p(xd), p(q)) == -1
    assert mul(h, mh, by(d), p(scratch), None, p(q)) == -1 and mul(h, mh, by(d), p(scratch), p(xd), None) == -1
    order = ("pol", "mesh", "d", "scratch", "inv", "b", "x", "max_iters", "tol", "rel_tol", "check_every", "rec")
    good = dict(pol=h, mesh=mh, d=by(d), scratch=p(scratch), inv=p(S.blocks().inverse), b=p(bd), x=p(xd), max_iters=4, tol=1.0, rel_tol=1e-3,
                check_every=2, rec=p(rec))
    solve = lambda **kw: hiplib.zs_rocm_mesh_system_solve(*[dict(good, **kw)[k] for k in order])
    for kw in (dict(pol=None), dict(mesh=None), dict(d=None), dict(scratch=None), dict(inv=None), dict(b=None), dict(x=None), dict(x=p(bd)),
               dict(max_iters=-1), dict(check_every=0), dict(rec=None)):
        assert solve(**kw) == -1, kw

    def broken(**fields):
        e = MeshSystemDesc()
        C.memmove(C.byref(e), C.byref(d), C.sizeof(e))
        for k, v in fields.items():
            setattr(e, k, v)
        return by(e)
    for fields in (dict(mass=None), dict(scale=float("inf")), dict(mu=-1.0), dict(kb=float("nan")), dict(dHat=0.0), dict(kappa=-1.0), dict(ptPairs=None),
                   dict(starts=None), dict(entries=None), dict(u=None), dict(record=None), dict(fStarts=None), dict(fEntries=None), dict(epsv=0.0),
                   dict(fmu=-1.0), dict(fEePairs=None)):
        assert mul(h, mh, broken(**fields), p(scratch), p(xd), p(q)) == -1, fields
        assert blocks(h, mh, broken(**fields), p(scratch), outs) == -1, fields
    pol.syncCtx()
    assert all(float(t.min()) == 7.0 == float(t.max()) for t in blk + [q]) and int(rec.min()) == 7 == int(rec.max()) and not xd.any()
    assert solve() == 0
    pol.syncCtx()
    assert int(rec[1]) in (1, 2)
