"""Additive CCD on the GPU (zpc_amd/csrc/mesh_ccd.hip, TriMesh.max_step / TriMesh.step_candidates) against the two properties of
tests/ref64_ccd.py with their derived constants, on every scene and direction, on candidate lists and on proximity lists at trial
positions; the global minimum, determinism and independence of the list order; the cases with an exact answer; the cap; the workgroup
paths of the kernel against one pair per call; NaN safety; completeness of the candidate list against a float64 brute force over all
pairs; five line-search steps end to end; the argument checks.  Prints one `CCD <what> ...` line per check.

Measured on an MI355X: every per-pair answer of every scene, direction and slack equals the float32 replay bit for bit; worst P1 0.005 of
its bound (`stack` under `random`, EE, slack 0.1), P2 never within 0.46 of its bound; t32 / t64 median 1.000000 on every scene, 0.9921 to
1.0387 on `stack`; the file runs in 9 s, its slowest case (`sheets` under `shrink`, 128 k EE pairs) in 0.8 s."""
import ctypes as C
import functools

import numpy as np
import pytest

import ref64_ccd as rc
import ref64_proximity as rp
from test_ccd_cpu import SCENES, T_MAX, below_share, cases

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _scene(name):
    v, t, dhat = rp.scene(name)
    return v, t, rp.edges(t), dhat


def _mesh(pol, name):
    from zpc_amd.mesh import TriMesh
    v, t, _, dhat = _scene(name)
    return TriMesh(pol, v, t), dhat


def _np(x):
    return None if x is None else x.cpu().numpy()


def _prox(pt=None, ee=None):
    from zpc_amd.mesh import Proximity
    p = Proximity()
    if pt is not None:
        p.pt_pairs = torch.as_tensor(np.ascontiguousarray(pt, np.int32).reshape(-1, 2), device="cuda")
    if ee is not None:
        p.ee_pairs = torch.as_tensor(np.ascontiguousarray(ee, np.int32).reshape(-1, 2), device="cuda")
    return p


def _sides(name, prox, x, p):
    """[(kind, X, P)] of the lists of prox at positions x under direction p"""
    _, t, e, _ = _scene(name)
    out = []
    for kind, pairs in (("pt", prox.pt_pairs), ("ee", prox.ee_pairs)):
        if pairs is not None:
            idx = rc.corners(t, e, _np(pairs), kind == "ee")
            out.append((kind, x[idx], p[idx]))
    return out


def _hold(what, name, prox, x, p, sb, slack, max_iter=256, ratio=False):
    """the device's StepBound against the properties and the replay's counts; returns (worst P1, worst P2, below, hits)"""
    worst = [0.0, 0.0, 0, 0]
    zero, capped = [0, 0], [0, 0]
    for kind, X, P in _sides(name, prox, x, p):
        ee = kind == "ee"
        toi = _np(sb.ee_toi if ee else sb.pt_toi)
        assert toi.dtype == np.float32 and toi.shape == (len(X),)
        r = rc.accd(X, P, ee, slack, T_MAX, max_iter, f32=True)
        same = int((toi.view(np.uint32) == r["t"].view(np.uint32)).sum())
        c = rc.check(X, P, ee, dict(t=toi, status=r["status"]), slack, T_MAX, max_iter)
        zero[ee], capped[ee] = int((r["status"] == rc.ZERO).sum()), int((r["status"] == rc.CAPPED).sum())
        line = "CCD %s %s slack %g: %d pairs, %d as the replay bit for bit, %d hits, %d breaks, %d capped, %d below resolution; worst P1 %.3f, " \
               "worst P2 %.3f of the bound" % (what, kind, slack, len(X), same, c["hits"], c["n_break"], capped[ee], c["below"], c["p1"], c["p2"])
        if ratio:
            r64 = rc.accd(X, P, ee, slack, T_MAX, max_iter)
            both = (r64["t"] > 0) & (r64["t"] < T_MAX) & (r64["status"] == rc.OK) & (r["status"] == rc.OK) & c["resolved"]
            q = toi[both].astype(np.float64) / r64["t"][both] if both.any() else np.ones(1)
            line += "; t32 / t64 median %.6f, from %.4f to %.4f" % (np.median(q), q.min(), q.max())
        print(line)
        assert c["ok"], (what, kind, slack, {k: v for k, v in c.items() if k != "resolved"})
        worst = [max(worst[0], c["p1"]), max(worst[1], c["p2"]), worst[2] + c["below"], worst[3] + c["hits"]]
    assert sb.zero_distance == tuple(zero) and sb.capped == tuple(capped), (what, sb.zero_distance, zero, sb.capped, capped)
    return worst


def _tmin(sb):
    parts = [np.float32(T_MAX)] + [_np(a).min() for a in (sb.pt_toi, sb.ee_toi) if a is not None and len(a)]
    return np.min(np.array(parts, np.float32))


# ------------------------------------------------------------------------------------------------ 1: the per-pair properties
@pytest.mark.parametrize("name,which", cases())
def test_properties_on_candidate_lists(pol, name, which):
    mesh, dhat = _mesh(pol, name)
    v = _scene(name)[0]
    p = rc.direction(name, v, which)
    cand = mesh.step_candidates(p, T_MAX)
    main, share = below_share(name)
    for slack in (0.1, 0.01):
        sb = mesh.max_step(cand, p, slack=slack, t_max=T_MAX)
        p1, p2, below, hits = _hold("candidates[%s, %s]" % (name, which), name, cand, v, p, sb, slack, ratio=which == main)
        assert sb.t.dtype == torch.float32 and sb.t.shape == () and _np(sb.t).view(np.uint32) == _tmin(sb).view(np.uint32)
        if which in ("translate", "zero"):
            assert float(sb.t) == T_MAX and all((_np(a) == T_MAX).all() for a in (sb.pt_toi, sb.ee_toi))
        if which == main:
            assert below <= share * hits
    if which == "zero":
        assert len(cand.pt_pairs) == 0 and len(cand.ee_pairs) == 0
    if name in ("sheets", "regular") and which == "approach":
        assert hits > 500 and float(sb.t) < 0.5


@pytest.mark.parametrize("name", SCENES)
def test_properties_on_proximity_lists_at_trial_positions(pol, name):
    mesh, dhat = _mesh(pol, name)
    v = _scene(name)[0]
    prox = mesh.proximity(dhat)
    which = below_share(name)[0]
    p = rc.direction(name, v, which)
    trial = (v + np.float32(0.05) * rc.direction(name, v, "random")).astype(np.float32)
    for slack in (0.1, 0.01):
        sb = mesh.max_step(prox, p, verts=trial, slack=slack, t_max=T_MAX)
        _hold("trial[%s, %s]" % (name, which), name, prox, trial, p, sb, slack)
        assert _np(sb.t).view(np.uint32) == _tmin(sb).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 2: the global minimum
def test_minimum_determinism_and_list_order(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v = _scene("sheets")[0]
    p = rc.direction("sheets", v, "approach")
    cand = mesh.step_candidates(p, T_MAX)
    a, b = mesh.max_step(cand, p), mesh.max_step(cand, p)
    assert _np(a.t).view(np.uint32) == _tmin(a).view(np.uint32) and float(a.t) < T_MAX
    for x, y in ((a.t, b.t), (a.pt_toi, b.pt_toi), (a.ee_toi, b.ee_toi)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert a.zero_distance == b.zero_distance and a.capped == b.capped
    g = np.random.default_rng(5)
    ipt, iee = g.permutation(len(cand.pt_pairs)), g.permutation(len(cand.ee_pairs))
    c = mesh.max_step(_prox(_np(cand.pt_pairs)[ipt], _np(cand.ee_pairs)[iee]), p)
    assert np.array_equal(_np(c.pt_toi).view(np.uint32), _np(a.pt_toi).view(np.uint32)[ipt])
    assert np.array_equal(_np(c.ee_toi).view(np.uint32), _np(a.ee_toi).view(np.uint32)[iee])
    assert _np(c.t).view(np.uint32) == _np(a.t).view(np.uint32)
    print("CCD minimum[sheets, approach]: t = %.9g over %d PT and %d EE pairs, the same bytes twice and under a permutation" %
          (float(a.t), len(cand.pt_pairs), len(cand.ee_pairs)))


# ------------------------------------------------------------------------------------------------ 3: exact cases
def test_empty_one_sided_and_inactive_lists(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _ = _scene("sheets")
    p = rc.direction("sheets", v, "approach")
    sb = mesh.max_step(_prox(np.zeros((0, 2)), np.zeros((0, 2))), p, t_max=0.75)
    assert float(sb.t) == 0.75 and len(sb.pt_toi) == 0 and len(sb.ee_toi) == 0 and sb.zero_distance == (0, 0) and sb.capped == (0, 0)
    tiny, _ = _mesh(pol, "tiny0")
    p0 = rc.direction("tiny0", _scene("tiny0")[0], "random")
    assert float(tiny.max_step(tiny.step_candidates(p0), p0).t) == T_MAX and float(tiny.max_step(tiny.proximity(0.05), p0).t) == T_MAX
    one = mesh.proximity(dhat, ee=False)
    sb = mesh.max_step(one, p)
    full = mesh.max_step(mesh.proximity(dhat), p)
    assert sb.ee_toi is None and torch.equal(sb.pt_toi, full.pt_toi) and float(sb.t) == float(full.pt_toi.min())
    other = mesh.max_step(mesh.proximity(dhat, pt=False), p)
    assert other.pt_toi is None and torch.equal(other.ee_toi, full.ee_toi)
    nv, nt, ne = len(v), len(t), len(e)
    bad = mesh.max_step(_prox([[nv, 0], [0, nt], [-1, 0], [3, -7], [nv + 5, nt + 5]], [[ne, 0], [0, ne], [-2, 1], [1, -1]]), p, t_max=0.5)
    assert (_np(bad.pt_toi) == 0.5).all() and (_np(bad.ee_toi) == 0.5).all() and float(bad.t) == 0.5
    print("CCD exact: empty lists, a mesh without triangles, one-sided lists and %d pairs outside the mesh give t_max" % 9)


def test_a_pair_at_zero_distance_gives_zero_and_is_counted(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _ = _scene("sheets")
    prox = mesh.proximity(dhat)
    pt = _np(prox.pt_pairs)
    vi, ti = pt[0]
    trial = v.copy()
    trial[vi] = trial[t[ti, 0]]                       # the vertex onto a corner of the triangle: the float32 distance is exactly 0
    p = rc.direction("sheets", v, "random")
    sb = mesh.max_step(prox, p, verts=trial)
    assert float(sb.t) == 0.0 and float(sb.pt_toi[0]) == 0.0 and sb.zero_distance[0] >= 1
    r = rc.accd(trial[rc.corners(t, e, pt, False)], p[rc.corners(t, e, pt, False)], False, 0.1, T_MAX, 256, f32=True)
    assert sb.zero_distance[0] == (r["status"] == rc.ZERO).sum()
    print("CCD zero distance[sheets]: %s pairs counted, t = 0" % (sb.zero_distance,))


# ------------------------------------------------------------------------------------------------ 4: the cap
def test_the_cap(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v = _scene("sheets")[0]
    p = rc.direction("sheets", v, "shrink")
    cand = mesh.step_candidates(p, T_MAX)
    sb = mesh.max_step(cand, p, max_iter=256)
    assert sb.capped[0] >= 1 and sb.capped[1] >= 1
    _hold("cap[sheets, shrink]", "sheets", cand, v, p, sb, 0.1, 256)         # the capped pairs pass P1 with the others
    one = mesh.max_step(cand, p, max_iter=1)
    seen = 0
    for kind, X, P in _sides("sheets", cand, v, p):
        r = rc.accd(X, P, kind == "ee", 0.1, T_MAX, 1, f32=True)
        toi = _np(one.ee_toi if kind == "ee" else one.pt_toi)
        loop = r["evals"] == 1                                              # passed the early out
        assert loop.sum() > 0 and (r["status"][loop] == rc.CAPPED).all() and (r["status"][~loop] != rc.CAPPED).all()
        assert np.array_equal(toi[loop].view(np.uint32), r["first"][loop].astype(np.float32).view(np.uint32))
        assert one.capped[kind == "ee"] == loop.sum()
        seen += int(loop.sum())
    print("CCD cap[sheets, shrink]: capped at 256 %s; at max_iter 1 all %d pairs behind the early out stop at their first increment" %
          (sb.capped, seen))


# ------------------------------------------------------------------------------------------------ 5: the workgroup paths
def test_workgroup_paths_against_one_pair_per_call(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v = _scene("sheets")[0]
    p = rc.direction("sheets", v, "approach")
    cand = mesh.step_candidates(p, T_MAX)
    for kind, X, P in _sides("sheets", cand, v, p):
        ee = kind == "ee"
        pairs = _np(cand.ee_pairs if ee else cand.pt_pairs)
        r = rc.accd(X, P, ee, 0.01, T_MAX, 256, f32=True)
        early, loop = np.nonzero(r["evals"] == 0)[0], np.nonzero(r["evals"] >= 1)[0]
        longest = int(np.argmax(r["evals"]))
        assert len(early) >= 511 and len(loop) >= 256 and r["evals"][longest] > 8
        # workgroup 0: early-out pairs only; 1: loop pairs only; 2: one long-running pair among finished ones
        order = np.concatenate([early[:256], loop[:256], early[256:400], [longest], early[400:511]])
        lst = pairs[order]
        mk = (lambda a: _prox(ee=a)) if ee else (lambda a: _prox(pt=a))
        get = (lambda s: _np(s.ee_toi)) if ee else (lambda s: _np(s.pt_toi))
        whole = mesh.max_step(mk(lst), p, slack=0.01)
        single = np.array([get(mesh.max_step(mk(lst[i:i + 1]), p, slack=0.01))[0] for i in range(len(lst))], np.float32)
        assert np.array_equal(get(whole).view(np.uint32), single.view(np.uint32))
        assert _np(whole.t).view(np.uint32) == single.min().view(np.uint32)
        tail = lst[256:]                                                    # starts with the loop pairs
        for n in (1, 63, 64, 65, 255, 256, 257):
            part = mesh.max_step(mk(tail[:n]), p, slack=0.01)
            assert np.array_equal(get(part).view(np.uint32), single[256:256 + n].view(np.uint32)), (kind, n)
            assert _np(part.t).view(np.uint32) == min(single[256:256 + n].min(), np.float32(T_MAX)).view(np.uint32)
        print("CCD workgroups[sheets, %s]: %d pairs in three workgroups and prefixes of 1 .. 257 equal one pair per call; most evaluations %d" %
              (kind, len(lst), r["evals"][longest]))


# ------------------------------------------------------------------------------------------------ 6: NaN
def test_a_nan_in_the_direction_gives_zero(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _ = _scene("sheets")
    p = rc.direction("sheets", v, "approach")
    cand = mesh.step_candidates(p, T_MAX)
    vi = int(_np(cand.pt_pairs)[0, 0])
    for val in (np.nan, np.inf):
        q = p.copy()
        q[vi, 1] = val
        sb = mesh.max_step(cand, q)
        assert float(sb.t) == 0.0
        for kind, pairs, toi in (("pt", cand.pt_pairs, sb.pt_toi), ("ee", cand.ee_pairs, sb.ee_toi)):
            touched = (rc.corners(t, e, _np(pairs), kind == "ee") == vi).any(axis=1)
            assert touched.any() and (_np(toi)[touched] == 0).all() and np.isfinite(_np(toi)).all()
    with pytest.raises(ValueError):
        mesh.step_candidates(q, T_MAX)
    print("CCD NaN[sheets]: a NaN or Inf in one direction row gives t = 0 for the pairs of that vertex")


# ------------------------------------------------------------------------------------------------ 7: completeness of step_candidates
def _all_pairs(t, e, nv):
    vi, ti = np.meshgrid(np.arange(nv), np.arange(len(t)), indexing="ij")
    pt = np.stack([vi.ravel(), ti.ravel()], axis=1)
    pt = pt[(t[pt[:, 1]] != pt[:, :1]).all(axis=1)]
    i, j = np.triu_indices(len(e), 1)
    share = (e[i, 0] == e[j, 0]) | (e[i, 0] == e[j, 1]) | (e[i, 1] == e[j, 0]) | (e[i, 1] == e[j, 1])
    return pt, np.stack([i, j], axis=1)[~share]


@pytest.mark.parametrize("name", ["sheets", "stack"])
def test_step_candidates_are_complete(pol, name):
    from zpc_amd.mesh import candidate_radius, proximity_grey
    mesh, dhat = _mesh(pol, name)
    v, t, e, _ = _scene(name)
    p = rc.direction(name, v, "random")
    cand = mesh.step_candidates(p, T_MAX)
    sb = mesh.max_step(cand, p)
    lo, hi = v.min(axis=0), v.max(axis=0)
    top = float(np.linalg.norm(p.astype(np.float64), axis=1).max())
    margin = proximity_grey(candidate_radius(top, T_MAX, None, lo, hi), lo, hi) / (1 + 2.0 ** -15)     # the default margin, from below
    best_all, best_list = T_MAX, T_MAX
    for kind, pairs, listed in (("pt", _all_pairs(t, e, len(v))[0], cand.pt_pairs), ("ee", _all_pairs(t, e, len(v))[1], cand.ee_pairs)):
        ee = kind == "ee"
        idx = rc.corners(t, e, pairs, ee)
        X, P = v[idx].astype(np.float64), p[idx].astype(np.float64)
        r = rc.accd(X, P, ee, 0.1, T_MAX, 256)
        code = pairs[:, 0] * (1 << 20) + pairs[:, 1]
        got = _np(listed).astype(np.int64)
        inside = np.isin(code, got[:, 0] * (1 << 20) + got[:, 1])
        assert inside.sum() == len(got)                                    # the list has no pair the brute force does not know
        floor = r["d0"] - rc.speed_bound(P, ee) * T_MAX                     # the least the distance can be anywhere on [0, t_max]
        assert (r["t"][~inside] == T_MAX).all() and (floor[~inside] >= margin).all()
        best_all, best_list = min(best_all, r["t"].min()), min(best_list, r["t"][inside].min() if inside.any() else T_MAX)
        print("CCD complete[%s, %s]: %d of %d pairs listed; outside the list the distance stays above %.3e (margin %.3e)" %
              (name, kind, inside.sum(), len(pairs), floor[~inside].min() if (~inside).any() else np.inf, margin))
    assert best_list == best_all
    print("CCD complete[%s]: first contact bound over all pairs %.9g (float64), over the list %.9g, device %.9g" %
          (name, best_all, best_list, float(sb.t)))
    if name == "sheets":        # (the closest pairs of `stack` are under the float32 resolution: its two numbers need not be close)
        assert abs(float(sb.t) - best_all) <= 1e-3 * best_all


# ------------------------------------------------------------------------------------------------ 8: end to end
def test_five_line_search_steps_keep_the_barrier_finite(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v = _scene("sheets")[0]
    p = torch.as_tensor(rc.direction("sheets", v, "approach"), device="cuda")
    x = torch.as_tensor(v, device="cuda")
    mesh.set_rest()
    steps = []
    for k in range(5):
        sb = mesh.max_step(mesh.step_candidates(p, T_MAX), p)
        assert sb.zero_distance == (0, 0) and float(sb.t) > 0
        x = x + sb.t * p
        mesh.refit(x)
        B = mesh.barrier(mesh.proximity(dhat), dhat, 1.0)
        assert B.zero_distance == (0, 0) and np.isfinite(float(B.energy)) and torch.isfinite(B.grad).all()
        steps.append((float(sb.t), float(B.energy)))
    print("CCD end to end[sheets, approach]: (t, barrier energy) per step %s" % ", ".join("(%.4g, %.4g)" % s for s in steps))
    assert steps[0][1] > 0


# ------------------------------------------------------------------------------------------------ 9: argument errors
def test_argument_errors(pol):
    mesh, dhat = _mesh(pol, "tiny2")
    v = _scene("tiny2")[0]
    p = rc.direction("tiny2", v, "random")
    prox = mesh.proximity(dhat)
    for kw in (dict(slack=0.0), dict(slack=1.0), dict(slack=-0.5), dict(slack=float("nan")), dict(t_max=0.0), dict(t_max=-1.0),
               dict(t_max=float("inf")), dict(max_iter=0), dict(max_iter=-3)):
        with pytest.raises(ValueError):
            mesh.max_step(prox, p, **kw)
    for bad in (p[:-1], p[:, :2], np.zeros((len(v), 4), np.float32)):
        with pytest.raises(ValueError):
            mesh.max_step(prox, bad)
    with pytest.raises(ValueError):
        mesh.max_step((prox.pt_pairs, prox.ee_pairs), p)
    with pytest.raises(ValueError):
        mesh.max_step(prox, p, verts=v[:-1])
    from zpc_amd import lib
    L = lib()
    d = torch.as_tensor(p, device="cuda")
    out = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    npt, nee = len(prox.pt_pairs), len(prox.ee_pairs)

    def call(pol_=pol.handle, m=mesh.handle, dir_=d.data_ptr(), pt=prox.pt_pairs.data_ptr(), ee=prox.ee_pairs.data_ptr(), slack=0.1, t_max=1.0,
             it=256, tmin=out.data_ptr()):
        return L.zs_rocm_mesh_ccd(pol_, m, None, dir_, pt, npt, ee, nee, slack, t_max, it, None, None, tmin, None)
    assert npt and nee
    assert call(pol_=None) == -1 and call(m=None) == -1 and call(dir_=None) == -1 and call(tmin=None) == -1
    assert call(pt=None) == -1 and call(ee=None) == -1
    assert call(slack=0.0) == -1 and call(slack=1.0) == -1 and call(t_max=0.0) == -1 and call(t_max=float("inf")) == -1 and call(it=0) == -1
    assert L.zs_rocm_mesh_ccd(pol.handle, mesh.handle, None, d.data_ptr(), None, 1 << 28, None, 0, 0.1, 1.0, 256, None, None, out.data_ptr(),
                              None) == -1
    pol.syncCtx()
    assert float(out[0]) == -1.0                                           # nothing written
    assert call() == 0
    pol.syncCtx()
    assert 0.0 < float(out[0]) <= 1.0
