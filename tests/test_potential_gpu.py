"""The mesh incremental potential on the device (zpc_amd/mesh_potential.py, zpc_amd/csrc/mesh_potential.hip) against the existing public
calls, the float32 replay and the float64 reference of tests/ref64_potential.py.

Scenes: ref64_proximity.SCENES, the strips with nv = 255, 256, 258 (the 256-lane boundary of the vertex kernels and of the slope's partials)
and strip1x2047 / strip1x2048 (nv = 4096 / 4098, nt = 4094 / 4096: the smallest shapes on both sides of the 4096-element chunk of the
totals in the vertex and in the triangle array).  Positions: displaced(.., 1e-1) and compressed(.., 0.5); start = x minus a small
displacement, target = x plus a seeded offset.

1  parts[1..3] == the .energy of TriMesh.elastic / barrier / friction bit for bit, parts[0] and energy == the replay, the counts == the
   public calls' counts: every subset of terms, with fixed vertices and a non-positive mass;
2  grad == the replay bit for bit -- ref64_terms.gather over the per-element terms the public gradient entries leave in their scratch, plus
   the epilogue --, gradient=False gives the same energies, a second call the same bytes;
3  line search on sheets and sheets5: x, t, trials, flag, slope, energy and the whole history == the replay bit for bit (per-element
   energies from the public calls at the replay's own float32 trial positions), identical for check_every 1, 3, 8 and on a second call; the
   cases of ref64_potential.SEARCH_CASES, a NaN in the target, and t_max as the device scalar of max_step;
4  a list from step_candidates(p, t_max, margin=dhat) is complete: at every trial position the active pairs and their energies are those of
   a fresh proximity(dhat) there;
5  against truth on tiny2 and sheets5: the error of grad against the float64 reference is at most twice that of the same gradient composed
   in numpy from the three public float32 gradients;
6  three Newton iterations composed from public calls on sheets5: every search accepted, the energies strictly decreasing;
7  the argument checks, in Python and through the C ABI.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import ref64_elastic as rl
import ref64_potential as rq
import ref64_proximity as rp
import ref64_solve as rs
import ref64_terms as rt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STRIPS = ("strip14x16", "strip1x127", "strip1x128", "strip1x2047", "strip1x2048")
NAMES = rp.SCENES + STRIPS
POSITIONS = ("displaced", "compressed")
TERMS = ("elastic", "barrier", "friction")
f32 = np.float32


def _np(x):
    return None if x is None else x.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _scene(name):
    v, t, dhat = rs.scene(name)
    return v, np.asarray(t, np.int32).reshape(-1, 3), dhat


@functools.lru_cache(maxsize=None)
def _step(name, which):
    """(x, target, start, u) float32: the positions, the inertia target, the start of the step and u = x - start as the device takes it"""
    v, t, _ = _scene(name)
    x, target, start = rq.step_arrays(v, t)
    if which == "compressed":
        shift = rl.compressed(v, 0.5) - x
        x, target, start = x + shift, target + shift, start + shift
    return x, target, start, x - start


class Case:
    """a mesh with rest shape, rest lengths, proximity lists and lagged friction at the rest positions, masses from the vertex areas, and the
    incidences of the replay; built once per scene"""

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
        self.mass = (f32(rs.DENSITY) * _np(area)).astype(f32)
        t64, e = self.t.astype(np.int64), _np(mesh.edges()).astype(np.int64)
        pt, ee = _np(self.prox.pt_pairs).astype(np.int64), _np(self.prox.ee_pairs).astype(np.int64)
        self.pt, self.ee = pt, ee
        vert = np.concatenate([np.concatenate([pt[:, :1], t64[pt[:, 1]]], axis=1), np.concatenate([e[ee[:, 0]], e[ee[:, 1]]], axis=1)]).reshape(-1, 4)
        self.inc = dict(tri=rt.incidence(t64, self.nv), hinge=rt.incidence(_np(hinges).astype(np.int64).reshape(-1, 4), self.nv),
                        pair=rt.incidence(vert, self.nv))
        self._public = {}

    def potential(self, target, start, terms=TERMS, mass=None, fixed=None, scale=rs.SCALE):
        from zpc_amd.mesh_potential import MeshPotential
        return MeshPotential(self.mesh, self.mass if mass is None else mass, scale, target, start,
                             elastic=(rs.MU, rs.LAM, rs.KB) if "elastic" in terms else None,
                             barrier=(self.prox, self.dhat, rs.KAPPA) if "barrier" in terms else None,
                             friction=(self.lag, rs.FRICTION_MU, rs.EPS_V) if "friction" in terms else None, fixed=fixed)

    def system(self, fixed=None):
        from zpc_amd.mesh_solve import MeshSystem
        return MeshSystem(self.mesh, self.mass, rs.SCALE, elastic=(rs.MU, rs.LAM, rs.KB), barrier=(self.prox, self.dhat, rs.KAPPA),
                          friction=(self.lag, rs.FRICTION_MU, rs.EPS_V), fixed=fixed)

    def _pairs_gradient(self, what, x):
        """the public gradient entry of the barrier (at the positions x) or of friction (at the displacement x) through the mesh's own
        plumbing, which hands back the scratch of the call: (result, counts, pair terms [npt + nee, 4, 3])"""
        from zpc_amd.mesh import Barrier, Friction, _ptr
        m = self.mesh
        if what == "barrier":
            keep, pt, ee, npt, nee, head = m._barrier_args("barrier", self.prox, self.dhat, rs.KAPPA, x, True)
            r = Barrier()
        else:
            keep, pt, ee, npt, nee, mu, eps_v = m._friction_args("friction", self.lag, x, rs.FRICTION_MU, rs.EPS_V)
            head = (m.pol.handle, m.handle, keep.data_ptr(), _ptr(pt), npt, _ptr(ee), nee, self.lag.record.data_ptr(), mu, eps_v)
            r = Friction()
        counts, scratch = m._evaluate(r, what, head, (("pt_energy", npt), ("ee_energy", nee)), m._incidence(self.prox, pt, ee))
        return r, counts, _np(scratch).reshape(-1, 4, 3)

    def public(self, x, u, gradient=True, key=None):
        """the three public calls at x / u: dict term -> (part as the call's float64 total, per-element energies [a, b], counts, runs of the
        replay's gather or None); kept per key"""
        if key is not None and key in self._public:
            return self._public[key]
        m, out = self.mesh, {}
        el = m.elastic(rs.MU, rs.LAM, rs.KB, verts=x, gradient=gradient)
        runs = [self.inc["tri"] + (_np(el.tri_terms).reshape(-1, 3),), self.inc["hinge"] + (_np(el.hinge_terms).reshape(-1, 3),)] if gradient else None
        out["elastic"] = (float(el.energy.item()), [_np(el.tri_energy), _np(el.hinge_energy)], el.overflow, runs, _np(el.grad))
        if gradient:
            ba, cb, tb = self._pairs_gradient("barrier", x)
            fr, cf, tf = self._pairs_gradient("friction", u)
        else:
            ba, fr = m.barrier(self.prox, self.dhat, rs.KAPPA, verts=x, gradient=False), m.friction(self.lag, u, rs.FRICTION_MU, rs.EPS_V, gradient=False)
            cb, cf, tb, tf = ba.zero_distance, fr.overflow, None, None
        for k, r, c, terms in (("barrier", ba, cb, tb), ("friction", fr, cf, tf)):
            out[k] = (float(r.energy.item()), [_np(r.pt_energy), _np(r.ee_energy)], c, [self.inc["pair"] + (terms.reshape(-1, 3),)] if gradient else None,
                      _np(r.grad))
        if key is not None:
            self._public[key] = out
        return out

    def replay(self, x, target, u, terms, mass, fixed, gradient=True, scale=rs.SCALE, key=None):
        """dict(parts, energy, grad, fx) of the float32 replay on the per-element energies and terms of the public calls"""
        pub = self.public(x, u, gradient, key)
        fx = rs.fixed_mask(np.asarray(mass, f32), fixed)
        e_in, d = rq.inertia(x, target, mass, fx)
        parts = [rq.total([e_in])] + [rq.total(pub[k][1]) if k in terms else 0.0 for k in TERMS]
        g = None
        if gradient:
            runs = [r for k in TERMS if k in terms for r in pub[k][3]]
            acc = rt.gather(self.nv, runs, f32) if runs else np.zeros((self.nv, 3), f32)
            g = rq.gradient(d, mass, scale, acc, fx)
        return dict(parts=np.array(parts), energy=rq.compose(parts, scale), grad=g, fx=fx)


_cases = {}


def _case(pol, name):
    if name not in _cases:
        _cases[name] = Case(pol, name)
    return _cases[name]


def _variants(c):
    fixed = np.zeros(c.nv, np.uint8)
    fixed[2::5] = 1
    mass = c.mass.copy()
    mass[::9] = (0, -1, np.nan, np.inf)[len(c.name) % 4]
    return ((c.mass, None), (mass, fixed))


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("which", POSITIONS)
@pytest.mark.parametrize("name", NAMES)
def test_parts_energy_and_counts_for_every_subset_of_terms(pol, name, which):
    c = _case(pol, name)
    x, target, start, u = _step(name, which)
    pub = c.public(x, u, True, which)
    for n in range(4):
        for terms in itertools.combinations(TERMS, n):
            for mass, fixed in _variants(c):
                v = c.potential(target, start, terms, mass, fixed).evaluate(x)
                want = c.replay(x, target, u, terms, mass, fixed, key=which)
                parts = _np(v.parts)
                for i, k in enumerate(TERMS):
                    assert _same(parts[1 + i], np.float64(pub[k][0] if k in terms else 0.0)), (terms, k)
                assert _same(parts, want["parts"]) and _same(_np(v.energy), np.float64(want["energy"])), terms
                counts = dict(elastic=v.elastic_overflow, barrier=v.barrier_zero_distance, friction=v.friction_overflow)
                assert all(tuple(counts[k]) == (tuple(pub[k][2]) if k in terms else (0, 0)) for k in TERMS)
    if name in ("sheets", "fan", "stack", "strip14x16"):
        assert all(pub[k][0] > 0 for k in TERMS)


@pytest.mark.parametrize("which", POSITIONS)
@pytest.mark.parametrize("name", NAMES)
def test_grad_bit_for_bit_with_the_replay(pol, name, which):
    c = _case(pol, name)
    x, target, start, u = _step(name, which)
    for n in range(4):
        for terms in itertools.combinations(TERMS, n):
            for mass, fixed in _variants(c):
                P = c.potential(target, start, terms, mass, fixed)
                v, again, bare = P.evaluate(x), P.evaluate(x), P.evaluate(x, gradient=False)
                want = c.replay(x, target, u, terms, mass, fixed, key=which)
                g = _np(v.grad)
                assert g.dtype == f32 and _same(g, want["grad"]), (terms, np.abs(g - want["grad"]).max())
                assert _same(_np(again.grad), g) and _same(_np(again.parts), _np(v.parts)) and _same(_np(again.energy), _np(v.energy))
                assert bare.grad is None and _same(_np(bare.parts), _np(v.parts)) and _same(_np(bare.energy), _np(v.energy))
                if fixed is not None:
                    assert not g[2::5].any() and not g[::9].any()
    if name in ("sheets", "fan", "stack", "strip14x16"):
        assert np.abs(g).max() > 0


# ------------------------------------------------------------------------------------------------ 3
def _newton_direction(c, x, target, start, u, fixed=None):
    g = c.potential(target, start, fixed=fixed).evaluate(x).grad
    S = c.system(fixed)
    S.linearize(x, u)
    r = S.solve(-g, max_iters=400, rel_tol=1e-3)
    assert r.flag == "converged"
    return _np(r.x)


def _search_replay(c, x, target, start, u, p, t_max, fixed, **kw):
    first = c.replay(x, target, u, TERMS, c.mass, fixed)

    def energy_at(xk, uk):
        return c.replay(xk, target, uk, TERMS, c.mass, fixed, gradient=False)["energy"]
    return rq.search(energy_at, x, p, first["energy"], rq.slope(first["grad"], p, first["fx"]), t_max, first["fx"], start, **kw)


def _same64(a, b):
    """float64 numbers bit for bit; a NaN equals a NaN (numpy and the device give NaNs of different signs and payloads)"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and _same(a[~nan], b[~nan])


def _search_equal(r, want):
    assert (r.flag, r.trials) == (want["flag"], want["trials"])
    assert _same(_np(r.x), want["x"]) and _same(f32(r.t), f32(want["t"])) and _same64(r.energies, want["energies"])
    assert _same64(r.slope, want["slope"]) and _same64(r.energy, want["energy"])


@pytest.mark.parametrize("name", ("sheets", "sheets5"))
def test_line_search_bit_for_bit_with_the_replay_whatever_check_every(pol, name):
    c = _case(pol, name)
    x, target, start, u = _step(name, "displaced")
    fixed = None
    if name == "sheets5":
        fixed = np.zeros(c.nv, np.uint8)
        fixed[3::11] = 1
    d = _newton_direction(c, x, target, start, u, fixed)
    P = c.potential(target, start, fixed=fixed)
    for case, (mult, kw, flag, trials) in rq.SEARCH_CASES.items():
        p = (f32(mult) * d).astype(f32)
        want = _search_replay(c, x, target, start, u, p, 1.0, fixed, **kw)
        print("%s %s: flag %s after %d trials, t = %g, slope %.6e, energies %s" % (name, case, want["flag"], want["trials"], want["t"], want["slope"],
                                                                                   want["energies"]))
        for check_every in (1, 3, 8, 8):
            _search_equal(P.line_search(x, p, 1.0, check_every=check_every, **kw), want)
        if name == "sheets":
            assert (want["flag"], want["trials"]) == (flag, trials), case      # (pinned on the CPU: tests/test_potential_cpu.py)
        if fixed is not None and want["flag"] == "accepted":
            assert np.array_equal(want["x"][3::11], x[3::11]) and not np.array_equal(want["x"], x)
    # a NaN in the target: not_finite before any trial, x = verts
    bad = target.copy()
    bad[5, 1] = np.nan
    r = c.potential(bad, start, fixed=fixed).line_search(x, d, 1.0)
    _search_equal(r, _search_replay(c, x, bad, start, u, d, 1.0, fixed))
    assert r.flag == "not_finite" and r.trials == 0 and len(r.energies) == 1 and _same(_np(r.x), x)
    # other c1 and shrink
    kw = dict(c1=0.3, shrink=0.7, max_trials=7)
    _search_equal(P.line_search(x, (f32(8) * d).astype(f32), 1.0, check_every=2, **kw), _search_replay(c, x, target, start, u, (f32(8) * d).astype(f32), 1.0, fixed, **kw))
    # t_max as the device scalar of max_step
    bound = c.mesh.max_step(c.prox, d, verts=x)
    t = float(bound.t.item())
    assert 0 < t <= 1
    a, b = P.line_search(x, d, bound.t), P.line_search(x, d, t)
    _search_equal(a, _search_replay(c, x, target, start, u, d, t, fixed))
    assert (a.flag, a.trials, a.t) == (b.flag, b.trials, b.t) and _same(_np(a.x), _np(b.x)) and _same(a.energies, b.energies) and a.flag == "accepted"


# ------------------------------------------------------------------------------------------------ 4
def test_a_candidate_list_is_complete_for_every_trial(pol):
    from zpc_amd.mesh import TriMesh
    c = _case(pol, "sheets")
    x, target, start, u = _step("sheets", "displaced")
    p = (f32(8) * _newton_direction(c, x, target, start, u)).astype(f32)
    meshes = []
    for _ in range(2):
        m = TriMesh(pol, c.v, c.t)
        m.set_rest()
        m.refit(x)
        meshes.append(m)
    moving, fresh = meshes
    t_max = float(moving.max_step(moving.step_candidates(p, 1.0), p).t.item())
    assert 0 < t_max < 1
    cand = moving.step_candidates(p, t_max, margin=c.dhat)
    from zpc_amd.mesh_potential import MeshPotential
    P = MeshPotential(moving, c.mass, rs.SCALE, target, barrier=(cand, c.dhat, rs.KAPPA))
    none = np.zeros(c.nv, bool)
    seen = 0
    for k in range(4):
        xk = rq.trial(x, p, f32(t_max) * f32(0.5) ** k, none)
        got = moving.barrier(cand, c.dhat, rs.KAPPA, verts=xk, gradient=False)
        assert _same(_np(P.evaluate(xk, gradient=False).parts)[2], _np(got.energy))
        fresh.refit(xk)
        near = fresh.proximity(c.dhat)
        want = fresh.barrier(near, c.dhat, rs.KAPPA, gradient=False)
        assert got.zero_distance == (0, 0) == want.zero_distance
        for a, ea, b, eb in ((cand.pt_pairs, got.pt_energy, near.pt_pairs, want.pt_energy), (cand.ee_pairs, got.ee_energy, near.ee_pairs, want.ee_energy)):
            ea, eb = _np(ea), _np(eb)
            A = {(int(i), int(j)): int(_bits(ea[n:n + 1])[0]) for n, (i, j) in enumerate(_np(a)) if ea[n] != 0}
            B = {(int(i), int(j)): int(_bits(eb[n:n + 1])[0]) for n, (i, j) in enumerate(_np(b)) if eb[n] != 0}
            assert A == B
            seen += len(A)
    assert seen > 0


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", rs.SMALL)
def test_grad_against_the_float64_reference(pol, name):
    """MI355X: tiny2 device 9.9163e-07 / composed 9.9163e-07 of max |g| 9.8737e-01; sheets5 device 2.5836e-05 / composed 2.6000e-05 of max |g|
    6.4255e+00: one accumulator over the four runs rounds no worse than three gathers and a torch sum, far below the factor of 2"""
    c = _case(pol, name)
    x, target, start, u = _step(name, "displaced")
    R = rs.System(c.v, c.t, c.mass, rs.SCALE, elastic=(rs.MU, rs.LAM, rs.KB),
                  barrier=dict(pt=c.pt, ee=c.ee, dhat=c.dhat, kappa=rs.KAPPA, rest2=_np(c.mesh.rest())),
                  friction=dict(pt=c.pt, ee=c.ee, record=_np(c.lag.record), mu=rs.FRICTION_MU, eps_v=rs.EPS_V), dtype=np.float64)
    g64 = rq.Potential(R, target, start).evaluate(x.astype(np.float64))["grad"]
    dev = _np(c.potential(target, start).evaluate(x).grad)
    pub = c.public(x, u, True, "displaced")
    composed = c.mass[:, None] * (x - target) + f32(rs.SCALE) * (pub["elastic"][4] + pub["barrier"][4] + pub["friction"][4])
    assert composed.dtype == f32
    err_dev, err_np = np.abs(dev - g64).max(), np.abs(composed - g64).max()
    print("%s: max |grad - float64| device %.4e / composed from the three public gradients %.4e, of max |g| %.4e" % (name, err_dev, err_np, np.abs(g64).max()))
    assert err_dev <= 2 * err_np


# ------------------------------------------------------------------------------------------------ 6
def test_three_newton_iterations_from_public_calls(pol):
    from zpc_amd.mesh import TriMesh
    from zpc_amd.mesh_potential import MeshPotential
    from zpc_amd.mesh_solve import MeshSystem
    c = _case(pol, "sheets5")
    x0, target, start, _ = _step("sheets5", "displaced")
    mesh = TriMesh(pol, c.v, c.t)
    mesh.set_rest()
    mesh.set_rest_shape()
    lag = mesh.friction_lag(mesh.proximity(c.dhat), c.dhat, rs.KAPPA)
    terms = lambda prox: dict(elastic=(rs.MU, rs.LAM, rs.KB), barrier=(prox, c.dhat, rs.KAPPA), friction=(lag, rs.FRICTION_MU, rs.EPS_V))
    x = torch.from_numpy(x0).cuda()
    start_d = torch.from_numpy(start).cuda()
    energies = []
    for it in range(3):
        mesh.refit(x)
        near = mesh.proximity(c.dhat)
        v = MeshPotential(mesh, c.mass, rs.SCALE, target, start, **terms(near)).evaluate(x)
        S = MeshSystem(mesh, c.mass, rs.SCALE, **terms(near))
        counts = S.linearize(x, x - start_d)
        d = S.solve(-v.grad, max_iters=400, rel_tol=1e-3)
        assert d.flag == "converged"
        cand = mesh.step_candidates(d.x, 1.0, margin=c.dhat)
        bound = mesh.max_step(cand, d.x)
        r = MeshPotential(mesh, c.mass, rs.SCALE, target, start, **terms(cand)).line_search(x, d.x, bound.t)
        print("iteration %d: E0 %.9e (%.9e on the dhat list), slope %.4e, max_step %.4g, %s after %d trials at t = %g, E %.9e"
              % (it, r.energies[0], float(v.energy.item()), r.slope, float(bound.t.item()), r.flag, r.trials, r.t, r.energy))
        assert r.flag == "accepted" and r.energy < r.energies[0]
        for z in (v.elastic_overflow, v.barrier_zero_distance, v.friction_overflow, counts.elastic_overflow, counts.barrier_zero_distance,
                  counts.friction_overflow, bound.zero_distance):
            assert tuple(z) == (0, 0)
        energies += [r.energies[0], r.energy] if it == 0 else [r.energy]
        x = r.x
    assert all(b < a for a, b in zip(energies, energies[1:])), energies


# ------------------------------------------------------------------------------------------------ 7
def test_the_argument_checks(pol, hiplib):
    from zpc_amd._lib import MeshSystemDesc
    from zpc_amd.mesh_potential import MeshPotential
    c = _case(pol, "tiny2")
    x, target, start, u = _step("tiny2", "displaced")
    ok = dict(elastic=(rs.MU, rs.LAM, rs.KB), barrier=(c.prox, c.dhat, rs.KAPPA), friction=(c.lag, rs.FRICTION_MU, rs.EPS_V))
    for bad in (dict(mass=c.mass[:-1]), dict(scale=float("nan")), dict(fixed=np.zeros(c.nv + 1, np.uint8)), dict(target=target[:-1]),
                dict(target=np.zeros((c.nv, 2), f32)), dict(start=start[:-1]), dict(start=None), dict(elastic=(-1.0, 0.0, 0.0)),
                dict(barrier=(c.prox, -1.0, 1.0)), dict(friction=(c.lag, 0.3, 0.0)), dict(friction=dict(lag=c.lag, mu=0.3))):
        kw = dict(dict(mass=c.mass, scale=rs.SCALE, target=target, start=start), **ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            MeshPotential(c.mesh, kw.pop("mass"), kw.pop("scale"), kw.pop("target"), kw.pop("start"), **kw)
    MeshPotential(c.mesh, c.mass, rs.SCALE, target, elastic=ok["elastic"], barrier=ok["barrier"])      # no friction: start is optional
    P = c.potential(target, start)
    for bad in (x[:-1], np.zeros((c.nv, 2), f32)):
        with pytest.raises(ValueError):
            P.evaluate(bad)
        with pytest.raises(ValueError):
            P.line_search(bad, x, 1.0)
        with pytest.raises(ValueError):
            P.line_search(x, bad, 1.0)
    for kw in (dict(c1=-1e-4), dict(c1=float("nan")), dict(shrink=0.0), dict(shrink=1.0), dict(shrink=-0.5), dict(max_trials=0), dict(check_every=0)):
        with pytest.raises(ValueError):
            P.line_search(x, u, 1.0, **kw)
    with pytest.raises(ValueError):
        P.line_search(x, u, torch.ones(2, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        P.line_search(x, u, torch.ones((), dtype=torch.float64, device="cuda"))
    assert P.evaluate(x.astype(np.float64)).grad.dtype == torch.float32      # other float types are converted
    # the C entries: -1 and nothing written
    d = MeshSystemDesc()
    C.memmove(C.byref(d), C.byref(P._desc), C.sizeof(d))
    h, mh, by = pol.handle, c.mesh.handle, C.byref
    sizes = (C.c_size_t * 3)()
    assert hiplib.zs_rocm_mesh_potential_sizes(mh, by(d), sizes) == 0 and sizes[2] == c.nv and sizes[0] > 0
    assert sizes[1] == c.nv + c.mesh.nt + c.mesh.num_hinges + 2 * (len(c.pt) + len(c.ee))
    assert hiplib.zs_rocm_mesh_potential_sizes(None, by(d), sizes) == -1 and hiplib.zs_rocm_mesh_potential_sizes(mh, None, sizes) == -1
    assert hiplib.zs_rocm_mesh_potential_sizes(mh, by(d), None) == -1
    dev = dict(dtype=torch.float32, device="cuda")
    scratch, energies = torch.zeros(int(sizes[0]), **dev), torch.full((int(sizes[1]),), 7.0, **dev)
    parts = torch.full((5,), 7.0, dtype=torch.float64, device="cuda")
    grad, xo = torch.full((c.nv, 3), 7.0, **dev), torch.full((c.nv, 3), 7.0, **dev)
    xd, td, sd = (torch.from_numpy(a).cuda() for a in (x, target, start))
    pd = -P.evaluate(x).grad      # (a descent direction: the search that runs at the end is accepted or runs out of trials)
    rec = torch.full((4 + 5,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()

    def broken(**fields):
        e = MeshSystemDesc()
        C.memmove(C.byref(e), C.byref(d), C.sizeof(e))
        for k, v in fields.items():
            setattr(e, k, v)
        return by(e)
    descs = [broken(**fields) for fields in (dict(mass=None), dict(scale=float("inf")), dict(mu=-1.0), dict(kb=float("nan")), dict(dHat=0.0), dict(kappa=-1.0),
                                             dict(ptPairs=None), dict(starts=None), dict(entries=None), dict(record=None), dict(fStarts=None),
                                             dict(fEntries=None), dict(epsv=0.0), dict(fmu=-1.0), dict(fEePairs=None))]
    order_e = ("pol", "mesh", "d", "target", "start", "verts", "scratch", "energies", "parts", "grad", "status")
    good_e = dict(pol=h, mesh=mh, d=by(d), target=p(td), start=p(sd), verts=p(xd), scratch=p(scratch), energies=p(energies), parts=p(parts), grad=p(grad),
                status=None)
    evaluate = lambda **kw: hiplib.zs_rocm_mesh_potential_evaluate(*[dict(good_e, **kw)[k] for k in order_e])
    for kw in [dict(pol=None), dict(mesh=None), dict(d=None), dict(target=None), dict(start=None), dict(verts=None), dict(scratch=None), dict(energies=None),
               dict(parts=None)] + [dict(d=e) for e in descs]:
        assert evaluate(**kw) == -1, kw
    order = ("pol", "mesh", "d", "target", "start", "verts", "dir", "t_max", "t_dev", "c1", "shrink", "max_trials", "check_every", "scratch", "energies",
             "x", "rec")
    good = dict(pol=h, mesh=mh, d=by(d), target=p(td), start=p(sd), verts=p(xd), dir=p(pd), t_max=1.0, t_dev=None, c1=1e-4, shrink=0.5, max_trials=4,
                check_every=2, scratch=p(scratch), energies=p(energies), x=p(xo), rec=p(rec))
    search = lambda **kw: hiplib.zs_rocm_mesh_potential_line_search(*[dict(good, **kw)[k] for k in order])
    for kw in [dict(pol=None), dict(mesh=None), dict(d=None), dict(target=None), dict(start=None), dict(verts=None), dict(dir=None), dict(scratch=None),
               dict(energies=None), dict(x=None), dict(x=p(xd)), dict(x=p(pd)), dict(rec=None), dict(c1=-1e-4), dict(c1=float("nan")), dict(shrink=0.0),
               dict(shrink=1.0), dict(max_trials=0), dict(check_every=0)] + [dict(d=e) for e in descs]:
        assert search(**kw) == -1, kw
    pol.syncCtx()
    assert all(float(t.min()) == 7.0 == float(t.max()) for t in (energies, parts, grad, xo, rec))
    assert evaluate() == 0 and evaluate(grad=None, scratch=None) == 0 and search() == 0
    pol.syncCtx()
    assert int(rec[:1].view(torch.int32)[1]) in (1, 2) and _same(_np(parts[4]), _np(P.evaluate(x).energy))
