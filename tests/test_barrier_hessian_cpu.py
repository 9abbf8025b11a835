"""Mesh barrier Hessian-vector product without a GPU (tests/ref64_barrier_hessian.py, include/zensim_rocm/barrier_device.hpp): the float64
closed forms against torch.autograd's double backward and against central differences of the float64 gradient, the float32 replay of the
device chain against the derived bounds on the random pairs of test_barrier_cpu.py, the measured constant of the vacuity guard, the
invariants of H and H+, the entry's declaration and binding, and the header itself compiled for the host under the sanitizers and compared bit for bit with the replay.
Prints one `HESSIAN <what> ...` line per check."""
import os
import re
import subprocess

import numpy as np
import pytest

import ref64_barrier as rb
import ref64_barrier_hessian as rh
import ref64_proximity as rp
from test_barrier_cpu import KAPPA, ROOT, _as_mesh, _libm_logf, _scene, random_ee, random_pt


def test_the_entry_is_declared_exported_and_bound(hiplib):
    header = open(os.path.join(ROOT, "include", "zs_rocm.h")).read()
    from zpc_amd.mesh import TriMesh
    name = "zs_rocm_mesh_barrier_hessian_product"
    assert re.search(r"ZS_ROCM_EXPORT\s+int\s+%s\(" % name, header), name + " is not declared in zs_rocm.h"
    assert len(getattr(hiplib, name).argtypes) == 17 and callable(getattr(TriMesh, "barrier_hessian_product", None))


def _single(v, t, e, pt, ee, dhat, rest2):
    """the pairs with one eligible candidate (the second derivative of the min-over-candidates distance exists there)"""
    Q = rh.Reference(v, t, pt, ee, dhat, KAPPA, rh.direction(len(v), 1), rest2, e)
    return pt[Q.pt["elig"].sum(axis=1) == 1], ee[Q.ee["elig"].sum(axis=1) == 1]


@pytest.mark.parametrize("mollify", [True, False])
@pytest.mark.parametrize("name", rp.SCENES)
def test_closed_forms_against_autograd_double_backward(name, mollify):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    rest2 = rest2 if mollify else None
    pt1, ee1 = _single(v, t, e, pt, ee, dhat, rest2)
    dirs = [rh.direction(len(v), s) for s in (1, 2)]
    auto = rh.autograd_hvp(v, t, e, pt1, ee1, rb.dhat2_f32(dhat), KAPPA, rest2, dirs)
    for x, a in zip(dirs, auto):
        R = rh.Reference(v, t, pt1, ee1, dhat, KAPPA, x, rest2, e)
        scale = max(np.abs(a).max(), np.abs(R.hx).max(), 1e-300)
        err = np.abs(a - R.hx).max() / scale
        print("HESSIAN autograd[%s, mollify %s]: %d of %d PT, %d of %d EE pairs with one candidate, largest |Hx| %.3e, closed form - autograd "
              "%.2e of it" % (name, mollify, len(pt1), len(pt), len(ee1), len(ee), scale, err))
        # both sides float64; the reasoning of the gradient test (autograd's line-line distance loses 1 / sin^2 of the edge angle) holds
        # one derivative up as well: measured 1.4e-10 at most (stack), so its 1e-7 stands
        assert err <= 1e-7
    if name in ("sheets", "torus", "stack"):
        assert len(pt1) > len(pt) // 4 and len(ee1) > len(ee) // 4 and np.abs(auto[0]).max() > 0


def test_closed_forms_against_central_differences_of_the_gradient_on_tiny2():
    v, t, e, pt, ee, dhat, rest2 = _scene("tiny2")
    assert len(pt) and len(ee)
    x = rh.direction(len(v), 3).astype(np.float64)
    R = rh.Reference(v, t, pt, ee, dhat, KAPPA, x, rest2, e)
    h = 1e-7
    # the gradient at float64 positions v +- h x: ref64_barrier.Reference rounds its input to float32, so the pairs are evaluated directly
    g = [_grad64(rp._v64(v) + s * h * x, t, e, pt, ee, R.dhat2, rest2) for s in (1, -1)]
    fd = (g[0] - g[1]) / (2 * h)
    scale = np.abs(R.hx).max()
    print("HESSIAN differences[tiny2]: largest |Hx| %.3e, closed form - central difference %.2e of it" % (scale, np.abs(fd - R.hx).max() / scale))
    assert np.abs(fd - R.hx).max() <= 1e-5 * scale


def _grad64(x, t, e, pt, ee, dhat2, rest2):
    """the float64 gradient of ref64_barrier at float64 positions (not rounded to float32: the differences need the small step)"""
    import ref64_mesh as rm
    g = np.zeros_like(x)
    vert = np.concatenate([pt[:, :1], np.asarray(t, np.int64)[pt[:, 1]]], axis=1)
    p, a, b, c = (x[vert[:, k]] for k in range(4))
    d2, cp, bary, _ = rm.tri_closest(p, a, b, c)
    bp = rb.barrier(d2, dhat2, KAPPA)[1]
    w = np.concatenate([np.ones((len(pt), 1)), -bary], axis=1)
    np.add.at(g, vert.ravel(), ((2 * bp)[:, None, None] * w[:, :, None] * (p - cp)[:, None, :]).reshape(-1, 3))
    ed = np.asarray(e, np.int64)
    vert = np.concatenate([ed[ee[:, 0]], ed[ee[:, 1]]], axis=1)
    a0, a1, b0, b1 = (x[vert[:, k]] for k in range(4))
    d2, s, tt, _, _ = rp.ee_closest(a0, a1, b0, b1)
    bb, bp = rb.barrier(d2, dhat2, KAPPA)
    u, vv = a1 - a0, b1 - b0
    n = rb._cross(u, vv)
    m, mp = rb.mollifier(rb._dot(n, n), 1e-2 * rest2[ee[:, 0]] * rest2[ee[:, 1]])
    w = np.stack([1 - s, s, -(1 - tt), -tt], axis=1)
    r = (a0 + s[:, None] * u) - (b0 + tt[:, None] * vv)
    gcu, gcv = 2 * rb._cross(vv, n), 2 * rb._cross(n, u)
    gc = np.stack([-gcu, gcu, -gcv, gcv], axis=1)
    np.add.at(g, vert.ravel(), ((2 * m * bp)[:, None, None] * w[:, :, None] * r[:, None, :] + (mp * bb)[:, None, None] * gc).reshape(-1, 3))
    return g


# ------------------------------------------------------------------------------------------------ the float32 replay on random pairs
def _pair_directions(n, seed):
    return np.random.default_rng(seed).standard_normal((4 * n, 3)).astype(np.float32)


@pytest.mark.parametrize("psd", [False, True])
def test_float32_replay_stays_within_the_bounds(psd):
    n, dhat = 120000, 0.03
    dhat2 = rb.dhat2_f32(dhat)
    P = random_pt(n, 21)
    verts, tris, pairs = _as_mesh(P, "pt")
    xdir = _pair_directions(n, 41)
    q = rh.pt_candidates64(verts, tris, pairs, xdir, dhat2, KAPPA, psd)
    h32, st = rh.pt_hvp32(*P, xdir.reshape(n, 4, 3), dhat2, KAPPA, psd)
    ratio, unb = rh.pair_ratio(h32, q)
    act = q["d"] < dhat
    print("HESSIAN replay PT (psd %s): %d pairs, %d active, worst %.3f of the bound, %d unbounded, %d pairs with more than one candidate" %
          (psd, n, act.sum(), ratio.max(), (unb & act).sum(), (q["elig"].sum(axis=1) > 1).sum()))
    assert act.sum() > n // 2 and np.isfinite(h32).all()
    assert (ratio <= 1).all()
    assert (unb & act).mean() < 0.01

    P = random_ee(n, 22)
    verts, edges, pairs = _as_mesh(P, "ee")
    rest2 = rb.rest_len2(verts, edges)
    for mollify in (True, False):
        q = rh.ee_candidates64(verts, edges, pairs, xdir, dhat2, KAPPA, psd, rest2 if mollify else None)
        eps = rb.ee_eps32(rest2[pairs[:, 0]].astype(np.float32), rest2[pairs[:, 1]].astype(np.float32)) if mollify else np.float32(0)
        h32, st = rh.ee_hvp32(*P, xdir.reshape(n, 4, 3), dhat2, KAPPA, eps, psd)
        ratio, unb = rh.pair_ratio(h32, q)
        act = q["d"] < dhat
        print("HESSIAN replay EE (psd %s, mollify %s): %d pairs, %d active, %d mollified (m < 1), worst %.3f of the bound, %d unbounded, %d pairs "
              "with more than one candidate" % (psd, mollify, n, act.sum(), (q["m"] < 1).sum(), ratio.max(), (unb & act).sum(),
                                                (q["elig"].sum(axis=1) > 1).sum()))
        assert act.sum() > n // 4 and np.isfinite(h32).all()
        assert (ratio <= 1).all()


def _sheets_median(psd=False):
    v, t, e, pt, ee, dhat, rest2 = _scene("sheets")
    R = rh.Reference(v, t, pt, ee, dhat, KAPPA, rh.direction(len(v), 1), rest2, e, psd=psd)
    contact = R.ninc > 0
    return R, contact, R.vbound[contact] / np.linalg.norm(R.hx[contact], axis=1)


def test_the_vacuity_guard_constant_is_the_measured_one():
    R, contact, ratio = _sheets_median()
    med = float(np.median(ratio))
    print("HESSIAN vacuity[sheets]: %d contact vertices, bound / |Hx| median %.3e (constant %.3e), smallest %.2e, largest %.2e" %
          (contact.sum(), med, rh.SHEETS_MEDIAN_BOUND_OVER_HX, ratio.min(), ratio.max()))
    assert contact.sum() > 200
    assert abs(med - rh.SHEETS_MEDIAN_BOUND_OVER_HX) <= 0.02 * rh.SHEETS_MEDIAN_BOUND_OVER_HX


@pytest.mark.parametrize("name", ["sheets", "torus", "stack"])
def test_the_invariants_of_the_product_in_float64(name):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    nv = len(v)
    x, y = rh.direction(nv, 1).astype(np.float64), rh.direction(nv, 2).astype(np.float64)
    H = lambda z, mol=True, psd=False: rh.Reference(v, t, pt, ee, dhat, KAPPA, z, rest2 if mol else None, e, psd=psd)

    def terms(R, z):
        """z^T H x as the sum over (pair, corner) terms, and the sum of their absolute values"""
        s = a = 0.0
        for q in (R.pt, R.ee):
            hq = rh.own(q)[0]
            prod = (hq * z[q["vert"]]).sum(axis=2)
            s, a = s + prod.sum(), a + np.abs(prod).sum()
        return s, a
    for psd in (False, True):
        Rx, Ry = H(x, psd=psd), H(y, psd=psd)
        (yx, a1), (xy, a2) = terms(Rx, y), terms(Ry, x)
        assert abs(yx - xy) <= 1e-12 * (a1 + a2), (name, psd)
        xx, a3 = terms(Rx, x)
        print("HESSIAN invariants[%s, psd %s]: y^T H x %.6e, x^T H y %.6e, x^T H x %.6e" % (name, psd, yx, xy, xx))
        if psd:
            assert xx >= -1e-12 * a3
    # one translation for all vertices: every pair's product vanishes
    Rt = H(np.broadcast_to(np.array([0.3, -1.1, 0.7]), (nv, 3)))
    mag = sum(np.abs(rh.own(q)[0]).sum() for q in (H(x).pt, H(x).ee))
    assert max(np.abs(rh.own(q)[0]).sum() for q in (Rt.pt, Rt.ee)) <= 1e-12 * mag
    # unmollified: H+ majorises H
    (pl, a1), (ex, a2) = terms(H(x, False, True), x), terms(H(x, False, False), x)
    assert pl >= ex - 1e-12 * (a1 + a2) and pl >= -1e-12 * a1


# ------------------------------------------------------------------------------------------------ the header on the host
def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_barrier_hessian")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_barrier_hessian.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    log = _libm_logf()
    n, dhat2 = 50000, np.float32(rb.dhat2_f32(0.03))
    f = np.float32
    # the degenerate records of test_barrier_cpu.py's host test: coincident points (zero distance), zero-length and exactly parallel edges,
    # a point in the plane of its triangle, a pair beyond dHat
    extra = np.array([[[.3, .3, .3], [.3, .3, .3], [.4, .3, .3], [.3, .4, .3]], [[.32, .32, .3], [.3, .3, .3], [.4, .3, .3], [.3, .4, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.3, .3, .31], [.4, .3, .31]], [[.3, .3, .3], [.3, .3, .3], [.3, .3, .3], [.3, .3, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.35, .25, .3], [.35, .35, .3]], [[.3, .3, .3], [.4, .3, .3], [.3, .3, .5], [.4, .31, .5]]], f)
    for kind, P in (("pt", random_pt(n, 31)), ("ee", random_ee(n, 32))):
        P = tuple(np.concatenate([x, extra[:, k]]) for k, x in enumerate(P))
        m = len(P[0])
        kappa = np.where(np.arange(m) % 4 < 2, f(1), f(1e3)).astype(f)
        psd = np.arange(m) % 2 == 1
        if kind == "ee":
            la, lb = rb._dot(P[1] - P[0], P[1] - P[0]), rb._dot(P[3] - P[2], P[3] - P[2])
            eps = np.where(np.arange(m) % 3 == 0, f(0), rb.ee_eps32(la, lb)).astype(f)      # every third pair unmollified
        else:
            eps = np.zeros(m, f)
        xdir = _pair_directions(m, 51).reshape(m, 4, 3)
        rec = np.concatenate([np.stack(P, axis=1).reshape(m, 12), np.full((m, 1), dhat2, f), kappa[:, None], eps[:, None],
                              psd.astype(f)[:, None], xdir.reshape(m, 12)], axis=1).astype(f)
        fin, fout = str(tmp_path / (kind + ".bin")), str(tmp_path / (kind + ".out"))
        rec.tofile(fin)
        r = subprocess.run([exe, fin, fout, kind], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        out = np.fromfile(fout, np.dtype([("h", f, (4, 3)), ("status", np.int32)]))
        assert len(out) == m
        h32, st = np.zeros((m, 4, 3), f), np.zeros(m, np.int32)
        for k in np.unique(kappa):
            for mode in (False, True):
                sel = (kappa == k) & (psd == mode)
                args = tuple(x[sel] for x in P) + (xdir[sel], dhat2, k)
                h32[sel], st[sel] = rh.pt_hvp32(*args, mode, log) if kind == "pt" else rh.ee_hvp32(*args, eps[sel], mode, log)
        assert np.array_equal(out["status"], st)
        assert np.array_equal(out["h"].view(np.uint32), h32.view(np.uint32))
        assert np.isfinite(out["h"]).all()
        idle = out["status"] != 1
        assert (out["h"][idle].view(np.uint32) == 0).all()
        print("HESSIAN host %s: %d pairs bit for bit with the replay, status counts %s, exactly zero products %d" %
              (kind, m, np.bincount(out["status"], minlength=3).tolist(), (np.abs(out["h"]).max(axis=(1, 2)) == 0).sum()))
        assert (out["status"] == 2).sum() >= 1 and (out["status"] == 0).sum() >= 1 and (out["status"] == 1).sum() > n // 4
        if kind == "ee":
            # the exactly parallel pair of `extra` (record n + 2): mollified it has m = 0 and what is left, b m' hess c . x, is finite
            assert np.isfinite(out["h"][n + 2]).all() and out["status"][n + 2] == 1
