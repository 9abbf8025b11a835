"""Mesh barrier potential without a GPU (tests/ref64_barrier.py, include/zensim_rocm/barrier_device.hpp): the float64 closed forms against
torch.autograd and central differences, the float32 replay of the device chain against the derived bounds on random pairs down to angles of
1e-7 rad and d / dHat of 1e-3, the measured constant of the vacuity guard, the header itself compiled for the host under the sanitizers
and compared bit for bit with the replay, and the invariants of the gradient.  Prints one `BARRIER <what> ...` line per check."""
import ctypes
import ctypes.util
import functools
import os
import subprocess

import numpy as np
import pytest

import ref64_barrier as rb
import ref64_proximity as rp
from test_proximity_cpu import seeded_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = rp.U
KAPPA = 1.0


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(verts, tris, edges, pt hits, ee hits, dhat, rest2) of a scene of ref64_proximity, the hits from its float64 brute force"""
    v, t, dhat = rp.scene(name)
    R = rp.Reference(v, t, dhat)
    pt, ee = R.pt[R.pt_d < R.dhat], R.ee[R.ee_d < R.dhat]
    return v, t, R.edges, pt, ee, dhat, rb.rest_len2(v, R.edges)


@pytest.mark.parametrize("name", rp.SCENES)
def test_closed_forms_against_autograd(name):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    R = rb.Reference(v, t, pt, ee, dhat, KAPPA, rest2, e)
    energy, grad = rb.autograd_energy(v, t, e, pt, ee, R.dhat2, KAPPA, rest2)
    scale = max(np.abs(grad).max(), np.abs(R.grad).max(), 1e-300)
    err = np.abs(grad - R.grad).max() / scale
    print("BARRIER autograd[%s]: %d PT, %d EE pairs, energy %.6e (closed %.6e), largest |g| %.3e, closed form - autograd %.2e of it" %
          (name, len(pt), len(ee), energy, R.energy, scale, err))
    assert abs(energy - R.energy) <= 1e-12 * max(abs(energy), 1e-300)
    # both sides are float64; autograd's line-line distance (w . n)^2 / |n|^2 loses 1 / sin^2 of the angle between the edges in relative
    # accuracy and `stack` has interior pairs below 1e-3 rad after the jitter of its nearly parallel triangles: 1e-16 x 1e6 per pair, a few
    # tens of pairs per vertex.  A wrong weight or a missing term is an error of order one.
    assert err <= 1e-7
    if name in ("sheets", "torus", "fan", "stack", "regular"):
        assert np.abs(R.grad).max() > 0


def test_closed_forms_against_central_differences_on_tiny2():
    v, t, e, pt, ee, dhat, rest2 = _scene("tiny2")
    assert len(pt) and len(ee)
    R = rb.Reference(v, t, pt, ee, dhat, KAPPA, rest2, e)
    h = 1e-7
    fd = np.zeros_like(R.grad)
    for i in range(len(v)):
        for d in range(3):
            e2 = []
            for sgn in (1, -1):
                x = rp._v64(v).copy()
                x[i, d] += sgn * h
                e2.append(_energy64(x, t, e, pt, ee, R.dhat2, rest2))
            fd[i, d] = (e2[0] - e2[1]) / (2 * h)
    scale = np.abs(R.grad).max()
    print("BARRIER differences[tiny2]: largest |g| %.3e, closed form - central difference %.2e of it" % (scale, np.abs(fd - R.grad).max() / scale))
    assert np.abs(fd - R.grad).max() <= 1e-5 * scale


def _energy64(x, t, e, pt, ee, dhat2, rest2):
    """the energy at float64 positions x (not rounded to float32: the differences need the small step)"""
    import ref64_mesh as rm
    p, a, b, c = x[pt[:, 0]], x[t[pt[:, 1], 0]], x[t[pt[:, 1], 1]], x[t[pt[:, 1], 2]]
    total = rb.barrier(rm.tri_closest(p, a, b, c)[0], dhat2, KAPPA)[0].sum()
    a0, a1, b0, b1 = rb._ee_vertices(x, np.asarray(e, np.int64), ee)
    n = rb._cross(a1 - a0, b1 - b0)
    m = rb.mollifier(rb._dot(n, n), 1e-2 * rest2[ee[:, 0]] * rest2[ee[:, 1]])[0]
    return total + (m * rb.barrier(rp.ee_closest(a0, a1, b0, b1)[0], dhat2, KAPPA)[0]).sum()


# ------------------------------------------------------------------------------------------------ the float32 replay on random pairs
def random_ee(n, seed):
    """seeded_pairs of test_proximity_cpu (angles log-uniform in [1e-7, 1] rad) with the separation redrawn so that d / dHat is log-uniform
    in [1e-3, 1] where the minimiser is interior; dHat = 0.03"""
    a0, a1, b0, b1 = (x.astype(np.float64) for x in seeded_pairs(n, seed))
    g = np.random.default_rng(seed + 100)
    u, v = a1 - a0, b1 - b0
    nrm = np.cross(u, v)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cur = ((b0 - a0) * nrm).sum(axis=1)
    want = 0.03 * np.exp(g.uniform(np.log(1e-3), 0.0, n))
    shift = (want - cur)[:, None] * nrm
    return tuple(x.astype(np.float32) for x in (a0, a1, b0 + shift, b1 + shift))


def random_pt(n, seed):
    """points over and around random triangles (edges 0.015 .. 0.075 inside [0.2, 0.8]^3), heights with d / dHat log-uniform in [1e-3, 1]"""
    g = np.random.default_rng(seed)
    a = g.uniform(0.3, 0.7, (n, 3))
    e1 = g.standard_normal((n, 3))
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(e1, g.standard_normal((n, 3)))
    e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
    b = a + g.uniform(0.015, 0.075, n)[:, None] * e1
    ang = g.uniform(0.2, 2.5, n)
    c = a + g.uniform(0.015, 0.075, n)[:, None] * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
    w = g.uniform(-0.25, 0.75, (n, 2))                 # barycentrics of the foot: inside, over an edge, beyond a vertex
    foot = a + w[:, :1] * (b - a) + w[:, 1:] * (c - a)
    h = 0.03 * np.exp(g.uniform(np.log(1e-3), 0.0, n))
    p = foot + h[:, None] * np.cross(e1, e2)
    return tuple(x.astype(np.float32) for x in (p, a, b, c))


def _as_mesh(P, kind):
    """n independent pairs as one vertex array with a triangle / edge list and the pair list"""
    n = len(P[0])
    verts = np.stack(P, axis=1).reshape(-1, 3)
    i = np.arange(n)
    if kind == "pt":
        return verts, np.stack([4 * i + 1, 4 * i + 2, 4 * i + 3], axis=1), np.stack([4 * i, i], axis=1)
    return verts, np.stack([4 * i, 4 * i + 1, 4 * i + 2, 4 * i + 3], axis=1).reshape(-1, 2), np.stack([2 * i, 2 * i + 1], axis=1)


def _ratios(e32, g32, q):
    """(energy, gradient) errors over their bounds: 0 where the error is exactly zero or the bound infinite, inf for an error against a
    zero bound"""
    with np.errstate(invalid="ignore", divide="ignore"):
        ee = np.where(e32.astype(np.float64) == q["e"], 0.0, np.abs(e32.astype(np.float64) - q["e"]))
        eg = rb._norm(g32.astype(np.float64) - q["g"])
        re = np.where((ee == 0) | np.isinf(q["be"]), 0.0, ee / q["be"])
        rg = np.where((eg == 0) | np.isinf(q["bg"]), 0.0, eg / q["bg"])
    return re, rg


def test_float32_replay_stays_within_the_bounds():
    n, dhat = 120000, 0.03
    dhat2 = rb.dhat2_f32(dhat)
    P = random_pt(n, 21)
    verts, tris, pairs = _as_mesh(P, "pt")
    q = rb.pt_pairs64(verts, tris, pairs, dhat2, KAPPA)
    e32, g32, st = rb.pt32(*P, dhat2, KAPPA)
    re, rg = _ratios(e32, g32, q)
    act = (q["d"] < dhat)
    print("BARRIER replay PT: %d pairs, %d active, d / dHat from %.1e; worst energy %.3f, worst gradient %.3f of the bound; median bound / |g| "
          "%.2e; %d unbounded" % (n, act.sum(), (q["d"][act] / dhat).min(), re.max(), rg.max(),
                                  np.median((q["bg"][act, 0] / rb._norm(q["g"][act, 0]))), (~np.isfinite(q["bg"][act])).sum()))
    assert n >= 10 ** 5 and act.sum() > n // 2 and np.isfinite(g32).all()
    assert (re <= 1).all() and (rg <= 1).all()
    assert np.isfinite(q["bg"][act]).mean() > 0.99

    P = random_ee(n, 22)
    verts, edges, pairs = _as_mesh(P, "ee")
    rest2 = rb.rest_len2(verts, edges)
    for mollify in (True, False):
        q = rb.ee_pairs64(verts, edges, pairs, dhat2, KAPPA, rest2 if mollify else None)
        eps = rb.ee_eps32(rest2[pairs[:, 0]].astype(np.float32), rest2[pairs[:, 1]].astype(np.float32)) if mollify else np.float32(0)
        e32, g32, st = rb.ee32(*P, dhat2, KAPPA, eps)
        re, rg = _ratios(e32, g32, q)
        act = q["d"] < dhat
        gn = rb._norm(q["g"][act]).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            med = np.median(q["bg"][act].max(axis=1) / gn)
        print("BARRIER replay EE (mollify %s): %d pairs, %d active, %d mollified (m < 1), d / dHat from %.1e; worst energy %.3f, worst gradient "
              "%.3f of the bound; median bound / |g| %.2e; %d unbounded" %
              (mollify, n, act.sum(), (q["m"] < 1).sum(), (q["d"][act] / dhat).min(), re.max(), rg.max(), med, (~np.isfinite(q["bg"][act])).sum()))
        assert act.sum() > n // 4 and np.isfinite(g32).all()
        assert (re <= 1).all() and (rg <= 1).all()
        if mollify:
            assert (q["m"] < 1).sum() > n // 10


def test_the_vacuity_guard_constant_is_the_measured_one():
    v, t, e, pt, ee, dhat, rest2 = _scene("sheets")
    R = rb.Reference(v, t, pt, ee, dhat, KAPPA, rest2, e)
    contact = R.ninc > 0
    ratio = R.vbound[contact] / np.linalg.norm(R.grad[contact], axis=1)
    med = float(np.median(ratio))
    print("BARRIER vacuity[sheets]: %d contact vertices, bound / |g| median %.3e (constant %.3e), smallest %.2e, largest %.2e" %
          (contact.sum(), med, rb.SHEETS_MEDIAN_BOUND_OVER_G, ratio.min(), ratio.max()))
    assert contact.sum() > 200
    assert abs(med - rb.SHEETS_MEDIAN_BOUND_OVER_G) <= 0.02 * rb.SHEETS_MEDIAN_BOUND_OVER_G
    assert med < 1e-2       # a bound that says something: the median vertex is held to better than a percent of its gradient


@pytest.mark.parametrize("name", ["sheets", "torus", "stack"])
def test_the_gradient_has_no_net_force_and_no_net_torque(name):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    R = rb.Reference(v, t, pt, ee, dhat, KAPPA, rest2, e)
    x = rp._v64(v)
    size = np.abs(R.grad).sum()
    force, torque = np.abs(R.grad.sum(axis=0)).max(), np.abs(np.cross(x - x.mean(axis=0), R.grad).sum(axis=0)).max()
    print("BARRIER invariants[%s]: sum |g| %.3e, net force %.2e, net torque %.2e" % (name, size, force, torque))
    assert size > 0 and force <= 1e-12 * size and torque <= 1e-12 * size


# ------------------------------------------------------------------------------------------------ the header on the host
def _libm_logf():
    """the logf the host program calls: the replay takes its logarithm from the same library, everything else is IEEE arithmetic"""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    one = np.frompyfunc(lambda x: libm.logf(float(x)), 1, 1)
    return lambda x: one(np.asarray(x, np.float32)).astype(np.float32)


def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_barrier")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_barrier.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    log = _libm_logf()
    n, dhat2 = 50000, np.float32(rb.dhat2_f32(0.03))
    f = np.float32
    # degenerate input next to the random pairs: coincident points (zero distance), zero-length and exactly parallel edges, a point in
    # the plane of its triangle, a pair beyond dHat
    extra = np.array([[[.3, .3, .3], [.3, .3, .3], [.4, .3, .3], [.3, .4, .3]], [[.32, .32, .3], [.3, .3, .3], [.4, .3, .3], [.3, .4, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.3, .3, .31], [.4, .3, .31]], [[.3, .3, .3], [.3, .3, .3], [.3, .3, .3], [.3, .3, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.35, .25, .3], [.35, .35, .3]], [[.3, .3, .3], [.4, .3, .3], [.3, .3, .5], [.4, .31, .5]]], f)
    for kind, P in (("pt", random_pt(n, 31)), ("ee", random_ee(n, 32))):
        P = tuple(np.concatenate([x, extra[:, k]]) for k, x in enumerate(P))
        m = len(P[0])
        kappa = np.where(np.arange(m) % 2 == 0, f(1), f(1e3)).astype(f)
        if kind == "ee":
            la, lb = rb._dot(P[1] - P[0], P[1] - P[0]), rb._dot(P[3] - P[2], P[3] - P[2])
            eps = np.where(np.arange(m) % 3 == 0, f(0), rb.ee_eps32(la, lb)).astype(f)      # every third pair unmollified
        else:
            eps = np.zeros(m, f)
        rec = np.concatenate([np.stack(P, axis=1).reshape(m, 12), np.full((m, 1), dhat2, f), kappa[:, None], eps[:, None], np.zeros((m, 1), f)],
                             axis=1).astype(f)
        fin, fout = str(tmp_path / (kind + ".bin")), str(tmp_path / (kind + ".out"))
        rec.tofile(fin)
        r = subprocess.run([exe, fin, fout, kind], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        out = np.fromfile(fout, np.dtype([("e", f), ("g", f, (4, 3)), ("status", np.int32)]))
        assert len(out) == m
        # kappa differs per pair: the replay is vectorised over it
        if kind == "pt":
            e32, g32, st = _per_kappa(lambda k, sel: rb.pt32(*(x[sel] for x in P), dhat2, k, log), kappa)
        else:
            e32, g32, st = _per_kappa(lambda k, sel: rb.ee32(*(x[sel] for x in P), dhat2, k, eps[sel], log), kappa)
        assert np.array_equal(out["status"], st)
        assert np.array_equal(out["e"].view(np.uint32), e32.view(np.uint32))
        assert np.array_equal(out["g"].view(np.uint32), g32.view(np.uint32))
        assert np.isfinite(out["g"]).all() and not np.isnan(out["e"]).any()
        zero = out["status"] == 2
        assert np.isinf(out["e"][zero]).all() and (out["g"][zero] == 0).all() and (out["g"][out["status"] == 0] == 0).all()
        print("BARRIER host %s: %d pairs bit for bit with the replay, status counts %s, exactly zero gradients %d" %
              (kind, m, np.bincount(out["status"], minlength=3).tolist(), (np.abs(out["g"]).max(axis=(1, 2)) == 0).sum()))
        assert zero.sum() >= 1 and (out["status"] == 0).sum() >= 1 and (out["status"] == 1).sum() > n // 4
    # (the exactly parallel pair of `extra`, mollified or not, and the pair beyond dHat were among the EE records)


def _per_kappa(fn, kappa):
    m = len(kappa)
    e, g, st = np.zeros(m, np.float32), np.zeros((m, 4, 3), np.float32), np.zeros(m, np.int32)
    for k in np.unique(kappa):
        sel = kappa == k
        e[sel], g[sel], st[sel] = fn(k, sel)
    return e, g, st
