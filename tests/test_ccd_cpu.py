"""Additive CCD without a GPU (tests/ref64_ccd.py, include/zensim_rocm/ccd_device.hpp): the float64 reference against the two properties
in exact form and on the cases with a known answer, the float32 replay of the device chain against the properties with the derived
constants on random pairs (angles between edges down to 1e-7 rad, d0 / |p| from 1e-4 to 10) and on every scene and direction, the header
itself compiled for the host under the sanitizers and compared bit for bit with the replay, the host logic of TriMesh.step_candidates and
the entry's declaration and binding.  Prints one `CCD <what> ...` line per check."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import ref64_ccd as rc
import ref64_proximity as rp
from test_barrier_cpu import ROOT, random_ee, random_pt

T_MAX = 1.0
SCENES = ("tiny0", "tiny1", "tiny2", "fan", "stack", "regular", "sheets", "torus")


def box_of(v):
    return v.min(axis=0), v.max(axis=0)


@functools.lru_cache(maxsize=None)
def scene_case(name, which):
    """(X, P) [n, 4, 3] of the PT and of the EE candidates of a scene under a direction: the float64 brute force within the radius of
    step_candidates (ref64_proximity keeps everything within twice its argument); None where the direction is not defined"""
    from zpc_amd.mesh import candidate_radius
    v, t, dhat = rp.scene(name)
    p = rc.direction(name, v, which)
    if p is None:
        return None
    top = float(np.linalg.norm(p.astype(np.float64), axis=1).max())
    radius = candidate_radius(top, T_MAX, None, *box_of(v)) if top > 0 and len(t) else dhat
    _, _, e, pt, ee, _ = _pairs(name, float(np.float32(radius)))
    out = {}
    for kind, pairs in (("pt", pt), ("ee", ee)):
        idx = rc.corners(t, e, pairs, kind == "ee")
        out[kind] = (v[idx], p[idx])
    return out


@functools.lru_cache(maxsize=None)
def _pairs(name, radius):
    return rc.scene_pairs(name, radius)


def cases():
    return [(n, w) for n in SCENES for w in rc.DIRECTIONS if not (w == "approach" and n not in ("sheets", "regular"))]


# ------------------------------------------------------------------------------------------------ float64 ACCD
@pytest.mark.parametrize("name,which", cases())
def test_float64_accd_holds_both_properties_exactly(name, which):
    case = scene_case(name, which)
    for slack in (0.1, 0.01):
        for kind in ("pt", "ee"):
            X, P = case[kind]
            r = rc.accd(X, P, kind == "ee", slack, T_MAX, 256)
            c = rc.check(X, P, kind == "ee", r, slack, T_MAX, 256, exact=True)
            print("CCD float64[%s, %s, %s, slack %g]: %d pairs, %d early, %d hits, %d breaks, %d capped, most evaluations %d; P1 %.3g, P2 %.3g "
                  "of the float64 rounding" % (name, which, kind, slack, len(X), r["early"].sum(), c["hits"], c["n_break"],
                                               (r["status"] == rc.CAPPED).sum(), r["evals"].max() if len(X) else 0, c["p1"], c["p2"]))
            assert c["ok"], (name, which, kind, slack, c)
            if which in ("translate", "zero"):
                assert (r["t"] == T_MAX).all() and (r["evals"] == 0).all()
    if name == "sheets" and which == "approach":
        assert c["hits"] > 100


def test_float64_accd_head_on_stops_at_the_first_increment():
    """`regular` under the pure approach (-0.06 in z on the upper sheet, gap 0.02): the facing pairs close head-on with l_p = 0.06, so the
    first increment 0.9 d0 / l_p = 0.3 already leaves exactly slack d0 and the next evaluation breaks"""
    v, t, dhat = rp.scene("regular")
    p = np.zeros_like(v)
    p[len(v) // 2:, 2] = -0.06
    _, _, e, pt, ee, _ = _pairs("regular", float(np.float32(dhat)))
    seen = 0
    for kind, pairs in (("pt", pt), ("ee", ee)):
        idx = rc.corners(t, e, pairs, kind == "ee")
        X, P = v[idx], p[idx]
        r = rc.accd(X, P, kind == "ee", 0.1, T_MAX, 256)
        facing = np.abs(r["d0"] - 0.02) < 1e-6
        moving = r["lp"] > 0
        assert (r["t"][~moving] == T_MAX).all()
        assert facing.sum() > 50 and np.allclose(r["t"][facing & moving], 0.3, rtol=0, atol=1e-6)
        seen += int((facing & moving).sum())
    print("CCD float64[regular, head-on]: %d facing pairs stop at 0.3" % seen)


# ------------------------------------------------------------------------------------------------ the float32 replay
def random_directions(X, ee, seed):
    """rows with a common part and a relative part of size d0 / ratio, ratio log-uniform in [1e-4, 10]; every eighth pair moves rigidly"""
    g = np.random.default_rng(seed)
    n = len(X)
    d0 = rc.distance(X.astype(np.float64), ee)
    ratio = np.exp(g.uniform(np.log(1e-4), np.log(10.0), n))
    rel = g.standard_normal((n, 4, 3))
    rel *= (d0 / ratio / np.linalg.norm(rel, axis=2).max(axis=1))[:, None, None]
    rel[::8] = 0
    return (g.uniform(-0.02, 0.02, (n, 1, 3)) + rel).astype(np.float32), ratio


def _hold(what, X, P, ee, slack, max_iter=256, res=None):
    r = rc.accd(X, P, ee, slack, T_MAX, max_iter, f32=True) if res is None else res
    c = rc.check(X, P, ee, r, slack, T_MAX, max_iter)
    r64 = rc.accd(X, P, ee, slack, T_MAX, max_iter)
    both = (r64["t"] > 0) & (r64["t"] < T_MAX) & (r64["status"] == rc.OK) & (np.asarray(r["status"]) == rc.OK) & c["resolved"]
    ratio = r["t"][both].astype(np.float64) / r64["t"][both] if both.any() else np.ones(1)
    print("CCD %s slack %g: %d pairs, %d hits, %d breaks, %d capped, %d zero, %d below resolution; worst P1 %.3f, worst P2 %.3f of the bound; "
          "t32 / t64 median %.6f, from %.4f to %.4f" % (what, slack, len(X), c["hits"], c["n_break"], (r["status"] == rc.CAPPED).sum(),
                                                        (r["status"] == rc.ZERO).sum(), c["below"], c["p1"], c["p2"], np.median(ratio),
                                                        ratio.min(), ratio.max()))
    assert c["ok"], (what, slack, c)
    return r, c


def test_float32_replay_holds_both_properties_on_random_pairs():
    n = 100000
    for kind, Q in (("pt", random_pt(n, 41)), ("ee", random_ee(n, 42))):
        X = np.stack(Q, axis=1)
        P, ratio = random_directions(X, kind == "ee", 43)
        for slack in (0.1, 0.01):
            r, c = _hold("replay %s" % kind, X, P, kind == "ee", slack)
            assert c["hits"] > n // 20 and c["n_break"] > n // 50 and r["early"].sum() > n // 20
        assert ratio.min() < 2e-4 and ratio.max() > 5 and (r["t"][::8] == T_MAX).all()


def below_share(name):
    """(direction, share): the share of a scene's hit pairs (PT and EE) that may lie under the float32 resolution, so that the properties
    are not asserted on next to nothing: 1 %, `stack` 10 % (its triangles start as close as 5e-8).  It is a condition on the scene's
    main direction -- the approach of the two-sheet scenes, `random` elsewhere.  The same few close pairs are hit under every direction,
    and the directions that hit little else (`slide`, `shrink`: a handful of pairs) have nothing to compare them with; their count is
    printed"""
    return ("approach" if name in ("sheets", "regular") else "random"), (0.10 if name == "stack" else 0.01)


@pytest.mark.parametrize("name", SCENES)
def test_float32_replay_holds_both_properties_on_the_scenes(name):
    main, share = below_share(name)
    for slack in (0.1, 0.01):
        for which in rc.DIRECTIONS:
            case = scene_case(name, which)
            if case is None:
                continue
            below = hits = 0
            for kind in ("pt", "ee"):
                X, P = case[kind]
                r, c = _hold("replay[%s, %s, %s]" % (name, which, kind), X, P, kind == "ee", slack)
                below, hits = below + c["below"], hits + c["hits"]
                if which in ("translate", "zero"):
                    assert (r["t"] == T_MAX).all()
            print("CCD replay[%s, %s] slack %g: %d of %d hit pairs under resolution" % (name, which, slack, below, hits))
            if which == main:
                assert below <= share * hits


# ------------------------------------------------------------------------------------------------ the header on the host
def host_records(kind, n, seed):
    """n random records and the special ones: zero distance, zero direction, NaN and Inf rows, slowly closing pairs that run into the
    cap, max_iter = 1"""
    f = np.float32
    Q = random_pt(n, seed) if kind == "pt" else random_ee(n, seed)
    X = np.stack(Q, axis=1)
    P, _ = random_directions(X, kind == "ee", seed + 1)
    slack = np.where(np.arange(n) % 2 == 0, f(0.1), f(0.01)).astype(f)
    it = np.where(np.arange(n) % 5 == 0, 1, np.where(np.arange(n) % 7 == 0, 3, 256)).astype(f)
    k = 64
    # slowly closing: the relative motion is tiny against the common one and aims at the other primitive, so the steps shrink with d
    Xs, Ps = X[:k].copy(), np.zeros((k, 4, 3), f)
    aim = (Xs[:, 1:].mean(axis=1) - Xs[:, 0]) if kind == "pt" else (Xs[:, 2:].mean(axis=1) - Xs[:, :2].mean(axis=1))
    Ps[:, 0] = 1.02 * aim
    if kind == "ee":
        Ps[:, 1] = 1.02 * aim
    Xz, Pz = X[:k].copy(), P[:k].copy()
    Xz[:, 0] = Xz[:, 2 if kind == "ee" else 1]            # zero distance: the point on a corner / a shared end point
    Pz[:, 0, 0] += f(0.01)                                # (and no rigid motion among them: that is decided before the distance)
    Xn, Pn = X[:k].copy(), P[:k].copy()
    Xn[0::4, 2, 1] = np.nan
    Pn[1::4, 0, 0] = np.nan
    Pn[2::4, 3, 2] = np.inf
    Xn[3::4, 0, 0] = -np.inf
    X = np.concatenate([X, Xs, Xz, Xn, X[:k]])
    P = np.concatenate([P, Ps, Pz, Pn, np.zeros((k, 4, 3), f)])
    slack = np.concatenate([slack, np.full(4 * k, f(0.1))])
    it = np.concatenate([it, np.full(k, f(40)), np.full(3 * k, f(256))])
    return X, P, slack, it


def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_ccd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_ccd.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    f = np.float32
    for kind in ("pt", "ee"):
        X, P, slack, it = host_records(kind, 50000, 51 if kind == "pt" else 53)
        m = len(X)
        rec = np.concatenate([X.reshape(m, 12), P.reshape(m, 12), slack[:, None], np.full((m, 1), f(T_MAX)), it[:, None], np.zeros((m, 1), f)],
                             axis=1).astype(f)
        r = subprocess.run([exe, kind], input=rec.tobytes(), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = r.stderr.decode()
        assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err
        out = np.frombuffer(r.stdout, np.dtype([("t", f), ("status", np.int32), ("evals", np.int32)]))
        assert len(out) == m
        t, st, ev = np.zeros(m, f), np.zeros(m, np.int32), np.zeros(m, np.int32)
        for s in np.unique(slack):
            for k in np.unique(it):
                sel = (slack == s) & (it == k)
                q = rc.accd(X[sel], P[sel], kind == "ee", s, T_MAX, int(k), f32=True)
                t[sel], st[sel], ev[sel] = q["t"], q["status"], q["evals"]
        assert np.array_equal(out["status"], st)
        assert np.array_equal(out["evals"], ev)
        assert np.array_equal(out["t"].view(np.uint32), t.view(np.uint32))
        nan = ~(np.isfinite(X).all(axis=(1, 2)) & np.isfinite(P).all(axis=(1, 2)))
        one = it == 1
        print("CCD host %s: %d records bit for bit with the replay in t, status and evaluations; status counts %s, %d with a NaN or Inf (t = 0), "
              "%d at max_iter 1, most evaluations %d" % (kind, m, np.bincount(st, minlength=3).tolist(), nan.sum(), one.sum(), ev.max()))
        assert nan.sum() >= 64 and (out["t"][nan] == 0).all() and (st[nan] == rc.OK).all()
        assert (st == rc.ZERO).sum() >= 64 and (out["t"][st == rc.ZERO] == 0).all()
        assert (st == rc.CAPPED).sum() >= 64 and (ev[st == rc.CAPPED] == it[st == rc.CAPPED]).all()
        assert (st[-64:] == rc.OK).all() and (out["t"][-64:] == T_MAX).all() and (ev[-64:] == 0).all()      # zero direction
        assert (ev[one] <= 1).all() and ((st[one] == rc.CAPPED) == (ev[one] == 1)).all()


# ------------------------------------------------------------------------------------------------ host logic, binding
def test_step_candidates_radius_is_rounded_up_and_covers_the_grey_zone():
    from zpc_amd.mesh import candidate_radius, proximity_grey
    g = np.random.default_rng(7)
    lo, hi = np.array([0.2, 0.2, 0.5]), np.array([0.8, 0.8, 0.52])
    for _ in range(2000):
        top, t_max = float(np.float32(np.exp(g.uniform(np.log(1e-6), np.log(10.0))))), float(np.exp(g.uniform(np.log(1e-3), np.log(10.0))))
        margin = None if g.random() < 0.5 else float(np.exp(g.uniform(np.log(1e-9), np.log(1e-2))))
        r = candidate_radius(top, t_max, margin, lo, hi)
        assert r == float(np.float32(r))                               # a float32 number
        grey = proximity_grey(r, lo, hi)
        want = 2 * t_max * top + (grey if margin is None else margin) + grey
        assert r >= want                                               # never below, in exact arithmetic on float64 operands
        assert r <= want * (1 + 2.0 ** -20) + 2 * grey * 2.0 ** -15    # and no more than the allowances above it
    # the grey zone is the bound of ref64_proximity with S and M replaced by what the box allows
    v, t, dhat = rp.scene("sheets")
    R = rp.Reference(v, t, dhat)
    assert proximity_grey(dhat, *box_of(v)) >= max(R.pt_b.max(), R.ee_b.max())
    assert proximity_grey(dhat, *box_of(v)) < 1e-5


def test_the_entry_is_declared_exported_and_bound(hiplib):
    header = open(os.path.join(ROOT, "include", "zs_rocm.h")).read()
    from zpc_amd.mesh import StepBound, TriMesh
    assert re.search(r"ZS_ROCM_EXPORT\s+int\s+zs_rocm_mesh_ccd\(", header)
    assert len(hiplib.zs_rocm_mesh_ccd.argtypes) == 15
    assert callable(getattr(TriMesh, "max_step", None)) and callable(getattr(TriMesh, "step_candidates", None))
    assert StepBound.__slots__ == ("t", "pt_toi", "ee_toi", "zero_distance", "capped")
