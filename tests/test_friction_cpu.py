"""Mesh friction without a GPU (tests/ref64_friction.py, include/zensim_rocm/friction_device.hpp): the entries' declarations and bindings;
the projector I - n n^T against the reference's per-feature tangent bases, and the closed-form gradient and product against
torch.autograd's backward and double backward of that basis form; the exact cases u = 0 and y = eps_v; the invariants of the gradient and
of H in float64; the float32 replay of the device chain (lag and evaluation) against the derived bounds on the random pairs of
test_barrier_cpu.py; the measured constant of the vacuity guard; and the header itself compiled for the host under the sanitizers and
compared bit for bit with the replay.  Prints one `FRICTION <what> ...` line per check."""
import os
import re
import subprocess

import numpy as np
import pytest

import ref64_barrier as rb
import ref64_friction as rf
import ref64_proximity as rp
from test_barrier_cpu import KAPPA, ROOT, _as_mesh, _libm_logf, _scene, random_ee, random_pt

MU, EPS = rf.MU, rf.EPS_V
ENTRIES = {"zs_rocm_mesh_friction_lag": 12, "zs_rocm_mesh_friction_energy": 14, "zs_rocm_mesh_friction_gradient": 18,
           "zs_rocm_mesh_friction_hessian_product": 16}


def test_the_entries_are_declared_exported_and_bound(hiplib):
    header = open(os.path.join(ROOT, "include", "zs_rocm.h")).read()
    from zpc_amd.mesh import TriMesh
    for name, nargs in ENTRIES.items():
        assert re.search(r"ZS_ROCM_EXPORT\s+int\s+%s\(" % name, header), name + " is not declared in zs_rocm.h"
        assert len(getattr(hiplib, name).argtypes) == nargs, name
    for method in ("friction_lag", "friction", "friction_hessian_product"):
        assert callable(getattr(TriMesh, method, None)), method


def _reference(name, scale, seed=1, x=None, mollify=True):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    u = rf.displacement(len(v), seed, scale * EPS)
    return rf.Reference(v, t, pt, ee, dhat, KAPPA, u, MU, EPS, x, rest2 if mollify else None, e), u


# ------------------------------------------------------------------------------------------------ the projector against the reference's bases
@pytest.mark.parametrize("name", rp.SCENES)
def test_the_projector_against_the_per_feature_bases_and_autograd(name):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    nv = len(v)
    dirs = [rf.displacement(nv, 10 + s, 1.0).astype(np.float64) for s in (1, 2)]
    for scale in rf.SCALES:
        R, u = _reference(name, scale, x=dirs[0])
        R2 = rf.Reference(v, t, pt, ee, dhat, KAPPA, u, MU, EPS, dirs[1], rest2, e)
        u64 = u.astype(np.float64)
        keep, T, energies, grad, hx = [], [], [], np.zeros((nv, 3)), [np.zeros((nv, 3)), np.zeros((nv, 3))]
        below = above = 0
        for q, q2, basis in ((R.pt, R2.pt, rf.bases_pt(v, t, pt)), (R.ee, R2.ee, rf.bases_ee(v, e, ee))):
            ok = q["act"] & (q["ncand"] == 1) & (q["ev"]["y"] > 0) & (q["lam"] > 0)
            keep.append(ok)
            # the energy on the basis: |T^T ur| in place of |(I - n n^T) ur|
            ur = (q["w"][:, :, None] * u64[q["vert"]]).sum(axis=1)
            yb = np.sqrt((np.einsum("ndk,nd->nk", np.where(ok[:, None, None], basis, 0.0), ur) ** 2).sum(axis=1))
            eb = MU * q["lam"] * rf.f0(yb, EPS)
            energies.append((q["ev"]["e"][ok], eb[ok]))
            T.append((basis[ok], q["lam"][ok], q["w"][ok], q["vert"][ok]))
            np.add.at(grad, q["vert"][ok].ravel(), q["ev"]["g"][ok].reshape(-1, 3))
            np.add.at(hx[0], q["vert"][ok].ravel(), q["ev"]["h"][ok].reshape(-1, 3))
            np.add.at(hx[1], q["vert"][ok].ravel(), q2["ev"]["h"][ok].reshape(-1, 3))
            below, above = below + (q["ev"]["y"][ok] < EPS).sum(), above + (q["ev"]["y"][ok] >= EPS).sum()
        own, onbasis = (np.concatenate([a[k] for a in energies]) for k in (0, 1))
        cat = [np.concatenate([a[k] for a in T]) for k in range(4)]
        _, ag, ahx = rf.basis_energy_autograd(cat[0], cat[1], cat[2], cat[3], u64, MU, EPS, dirs)
        worst = []
        for got, want in ((own, onbasis), (grad, ag), (hx[0], ahx[0]), (hx[1], ahx[1])):
            top = max(np.abs(want).max(), np.abs(got).max(), 1e-300) if len(want) else 1.0
            worst.append(np.abs(got - want).max() / top if len(want) else 0.0)
        print("FRICTION projector[%s, u = %g eps_v]: %d of %d PT, %d of %d EE pairs (y > 0, one candidate), %d below and %d at or above the "
              "threshold; projector - basis: energy %.2e, gradient - autograd %.2e, products - double backward %.2e, %.2e of the largest entry" %
              (name, scale, keep[0].sum(), len(pt), keep[1].sum(), len(ee), below, above, worst[0], worst[1], worst[2], worst[3]))
        # both sides float64: the project's tolerance for closed forms against autograd.  Measured: 2.2e-8 at worst (stack, a product at
        # 100 eps_v: pairs at d = 1e-7 leave float64 nine digits of n), 1.2e-11 or better on the other scenes
        assert max(worst) <= 1e-7
        if name in ("sheets", "torus", "stack"):
            assert keep[0].sum() > len(pt) // 4 and keep[1].sum() > len(ee) // 4 and np.abs(ag).max() > 0 and np.abs(ahx[0]).max() > 0
        if scale == 1.0 and len(own) > 50:
            assert below > 0 and above > 0      # both branches of f0 hold active pairs


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("name", ["sheets", "stack"])
def test_at_rest_the_energy_is_the_constant_and_the_gradient_is_zero(name):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    nv = len(v)
    x = rf.displacement(nv, 5, 1.0)
    R = rf.Reference(v, t, pt, ee, dhat, KAPPA, np.zeros((nv, 3), np.float32), MU, EPS, x, rest2, e)
    n = 0
    for q in (R.pt, R.ee):
        ev = q["ev"]
        assert np.array_equal(ev["e"], MU * q["lam"] * (EPS / 3)) and (ev["g"] == 0).all() and (ev["y"] == 0).all()
        want = (2 * MU * q["lam"] / EPS)[:, None, None] * q["w"][:, :, None] * ev["zt"][:, None, :]
        assert np.abs(ev["h"] - want).max() <= 1e-14 * np.abs(want).max()
        # the float32 chain on the float32 record: the same exact statements
        rec = q["rec"].astype(np.float32)
        rows = np.zeros((len(rec), 4, 3), np.float32)
        r32 = rf.evaluate32(rec, rows, MU, EPS, x[q["vert"]])
        f = np.float32
        assert np.array_equal(r32["e"], (f(MU) * rec[:, 3]) * (f(EPS) / f(3))) and (r32["g"] == 0).all() and (r32["st_g"] == r32["st_e"]).all()
        active = r32["st_h"] == 1
        want32 = (2 * MU * q["lam"] / EPS)[:, None, None] * q["w"][:, :, None] * ev["zt"][:, None, :]
        scale = np.abs(want32).max()
        assert np.abs(r32["h"][active] - want32[active]).max() <= 64 * rf.U * scale      # 13 float32 roundings of the chain on terms of that size
        n += active.sum()
    print("FRICTION at rest[%s]: %d active pairs, energy mu lambda eps_v / 3, gradient exactly zero, product 2 mu lambda / eps_v w_k zt" % (name, n))
    assert n > 100


def test_the_branches_agree_at_the_threshold_and_at_its_float_neighbours():
    eps = EPS
    for y in (np.nextafter(eps, 0.0), eps, np.nextafter(eps, 1.0)):
        low0, high0 = y * y * (eps - y / 3) / (eps * eps) + eps / 3, y
        low1, high1 = (2 * eps - y) / (eps * eps), 1 / y
        assert abs(low0 - high0) <= 4 * np.finfo(np.float64).eps * eps and abs(low1 - high1) <= 4 * np.finfo(np.float64).eps / eps
        # the eigenvalue along ut, c1 + c2 y^2: 2 (eps - y) / eps^2 below, 0 above
        along = float(rf.c1(y, eps) + rf.c2(y, eps) * y * y)
        assert abs(along) <= 8 * np.finfo(np.float64).eps / eps
        assert abs(float(rf.f0(y, eps)) - y) <= 4 * np.finfo(np.float64).eps * eps
    # the float32 chain: a record with n = e_z, lambda = 1, w = (1, -1, 0, 0) and u_0 = (y, 0, 0), x_0 = (1, 0, 0)
    f = np.float32
    e32 = f(EPS)
    ys = np.array([np.nextafter(e32, f(0)), e32, np.nextafter(e32, f(1))], f)
    rec = np.tile(np.array([0, 0, 1, 1, 1, -1, 0, 0], f), (3, 1))
    rows, xr = np.zeros((3, 4, 3), f), np.zeros((3, 4, 3), f)
    rows[:, 0, 0], xr[:, 0, 0] = ys, 1
    r = rf.evaluate32(rec, rows, 1.0, e32, xr)
    u32 = float(np.finfo(f).eps)
    print("FRICTION threshold: y / eps_v - 1 = %s, energy / y - 1 = %s, g c1 eps_v - 1 = %s, eigenvalue along ut x eps_v = %s" %
          ((ys / e32 - 1).tolist(), (r["e"] / ys - 1).tolist(), (r["g"][:, 0, 0] / ys * e32 - 1).tolist(), (r["h"][:, 0, 0] * e32).tolist()))
    assert (r["st_e"] == 1).all() and (r["st_h"] == 1).all()
    assert (np.abs(r["e"].astype(np.float64) / ys - 1) <= 8 * u32).all()
    assert (np.abs(r["g"][:, 0, 0].astype(np.float64) / ys * float(e32) - 1) <= 8 * u32).all()
    assert (np.abs(r["h"][:, 0, 0].astype(np.float64) * float(e32)) <= 16 * u32).all()


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("name", ["sheets", "torus", "stack"])
def test_the_invariants_in_float64(name):
    v, t, e, pt, ee, dhat, rest2 = _scene(name)
    nv = len(v)
    x, y = rf.displacement(nv, 21, 1.0).astype(np.float64), rf.displacement(nv, 22, 1.0).astype(np.float64)
    for scale in rf.SCALES:
        u = rf.displacement(nv, 1, scale * EPS)
        H = lambda z, uu=u: rf.Reference(v, t, pt, ee, dhat, KAPPA, uu, MU, EPS, z, rest2, e)

        def terms(R, z):
            """z^T H x as the sum over (pair, corner) terms, and the sum of their absolute values"""
            s = a = 0.0
            for q in (R.pt, R.ee):
                prod = (q["ev"]["h"] * z[q["vert"]]).sum(axis=2)
                s, a = s + prod.sum(), a + np.abs(prod).sum()
            return s, a
        Rx, Ry = H(x), H(y)
        (yx, a1), (xy, a2), (xx, a3) = terms(Rx, y), terms(Ry, x), terms(Rx, x)
        assert abs(yx - xy) <= 1e-12 * (a1 + a2) and xx >= -1e-12 * a3 and a3 > 0
        # one common translation added to u changes nothing (evaluate64 on the float64 sum u + c: Reference would round it to float32);
        # f0 has slope at most 1, so the energies move by no more than ut does
        c = np.array([0.3, -1.1, 0.7]) * scale * EPS
        size = np.abs(c).max() + np.abs(u).max()
        for q in (Rx.pt, Rx.ee):
            moved = rf.evaluate64(q["rec"], (u.astype(np.float64) + c)[q["vert"]], MU, EPS, x[q["vert"]])
            assert np.abs(moved["ut"] - q["ev"]["ut"]).max() <= 1e-12 * size
            assert np.abs(moved["e"] - q["ev"]["e"]).sum() <= 1e-12 * MU * (q["lam"] * size).sum()
        # a constant x: every pair's product vanishes; the gradient sums to zero over the vertices
        Rc = H(np.broadcast_to(np.array([0.3, -1.1, 0.7]), (nv, 3)))
        mag = sum(np.abs(q["ev"]["h"]).sum() for q in (Rx.pt, Rx.ee))
        assert max(np.abs(q["ev"]["h"]).sum() for q in (Rc.pt, Rc.ee)) <= 1e-12 * mag
        net, size = np.abs(Rx.grad.sum(axis=0)).max(), np.abs(Rx.pair_g).sum()
        assert size > 0 and net <= 1e-12 * size
        print("FRICTION invariants[%s, u = %g eps_v]: y^T H x %.6e, x^T H y %.6e, x^T H x %.6e, sum |g| %.3e, net force %.2e" %
              (name, scale, yx, xy, xx, size, net))


# ------------------------------------------------------------------------------------------------ the float32 replay on random pairs
def _rows(n, seed, scale):
    return (scale * np.random.default_rng(seed).standard_normal((n, 4, 3))).astype(np.float32)


def _ratio(err, bound):
    """error over bound: 0 where the error is exactly zero or the bound infinite, inf for an error against a zero bound"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((err == 0) | np.isinf(bound), 0.0, err / bound)


def _replay_against_bounds(what, q, rec32, n_pairs):
    """the lag record, and energy, gradient and product at the three scales, of the float32 replay against the float64 dict q"""
    r64 = q["rec"]
    worst = dict(n=_ratio(rb._norm(rec32[:, :3].astype(np.float64) - r64[:, :3]), q["dn"]).max(),
                 lam=_ratio(np.abs(rec32[:, 3].astype(np.float64) - r64[:, 3]), q["dlam"]).max(),
                 w=_ratio(np.abs(rec32[:, 4:].astype(np.float64) - r64[:, 4:]), q["dw"]).max())
    act = q["act"]
    unbounded = act & ~(np.isfinite(q["dn"]) & np.isfinite(q["dlam"]) & np.isfinite(q["dw"]).all(axis=1))
    xr = _rows(n_pairs, 43, 1.0)
    med = {}
    for scale in rf.SCALES:
        ur = _rows(n_pairs, 42, scale * EPS)
        ev = rf.evaluate64(r64, ur, MU, EPS, xr)
        be, bg, bh = rf.evaluate_bounds(q, ev, ur, MU, EPS, xr)
        r32 = rf.evaluate32(rec32, ur, MU, EPS, xr)
        assert np.isfinite(r32["g"]).all() and np.isfinite(r32["h"]).all() and np.isfinite(r32["e"]).all()
        assert (r32["st_e"] != 2).all() and (r32["st_g"] != 2).all() and (r32["st_h"] != 2).all()
        worst["e %g" % scale] = _ratio(np.abs(r32["e"].astype(np.float64) - ev["e"]), be).max()
        worst["g %g" % scale] = _ratio(rb._norm(r32["g"].astype(np.float64) - ev["g"]), bg).max()
        worst["h %g" % scale] = _ratio(rb._norm(r32["h"].astype(np.float64) - ev["h"]), bh).max()
        unbounded |= act & ~(np.isfinite(bg).all(axis=1) & np.isfinite(bh).all(axis=1) & np.isfinite(be))
        with np.errstate(invalid="ignore", divide="ignore"):
            med[scale] = np.median((bg[act].max(axis=1) / rb._norm(ev["g"][act]).max(axis=1)))
    print("FRICTION replay %s: %d pairs, %d active, %d with more than one candidate; worst error over bound: %s; median bound / |g| %s; "
          "%d active pairs unbounded" % (what, n_pairs, act.sum(), (q["ncand"] > 1).sum(), ", ".join("%s %.3f" % kv for kv in worst.items()),
                                         ", ".join("%.2e" % med[s] for s in rf.SCALES), unbounded.sum()))
    assert max(worst.values()) <= 1
    assert unbounded.sum() < 0.01 * act.sum()
    return act


def test_float32_replay_stays_within_the_bounds():
    n, dhat = 120000, 0.03
    dhat2 = rb.dhat2_f32(dhat)
    P = random_pt(n, 21)
    verts, tris, pairs = _as_mesh(P, "pt")
    q = rf.lag_pt64(verts, tris, pairs, dhat2, KAPPA)
    rec32, st, _ = rf.lag_pt32(*P, dhat2, KAPPA)
    act = _replay_against_bounds("PT", q, rec32, n)
    assert act.sum() > n // 2 and (st != 2).all()

    P = random_ee(n, 22)
    verts, edges, pairs = _as_mesh(P, "ee")
    rest2 = rb.rest_len2(verts, edges)
    for mollify in (True, False):
        q = rf.lag_ee64(verts, edges, pairs, dhat2, KAPPA, rest2 if mollify else None)
        eps = rb.ee_eps32(rest2[pairs[:, 0]].astype(np.float32), rest2[pairs[:, 1]].astype(np.float32)) if mollify else np.float32(0)
        rec32, st, _ = rf.lag_ee32(*P, dhat2, KAPPA, eps)
        act = _replay_against_bounds("EE (mollify %s)" % mollify, q, rec32, n)
        assert act.sum() > n // 4 and (st != 2).all()


def test_the_vacuity_guard_constant_is_the_measured_one():
    R, u = _reference("sheets", 1.0)
    contact = R.ninc > 0
    with np.errstate(divide="ignore"):
        ratio = R.vbound_g[contact] / np.linalg.norm(R.grad[contact], axis=1)
    med = float(np.median(ratio))
    print("FRICTION vacuity[sheets]: %d contact vertices, bound / |g| median %.3e (constant %.3e; the barrier's %.3e), smallest %.2e, largest "
          "%.2e" % (contact.sum(), med, rf.SHEETS_MEDIAN_BOUND_OVER_G, rb.SHEETS_MEDIAN_BOUND_OVER_G, ratio.min(), ratio.max()))
    assert contact.sum() > 200
    assert abs(med - rf.SHEETS_MEDIAN_BOUND_OVER_G) <= 0.02 * rf.SHEETS_MEDIAN_BOUND_OVER_G
    assert med < 1e-2       # a bound that says something: the median vertex is held to better than a percent of its friction force


# ------------------------------------------------------------------------------------------------ the header on the host
def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_friction")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_friction.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    log = _libm_logf()
    n, dhat2 = 50000, np.float32(rb.dhat2_f32(0.03))
    f = np.float32
    # degenerate geometry next to the random pairs, as in test_barrier_cpu.py: coincident points (zero distance), zero-length and exactly
    # parallel edges, a point in the plane of its triangle, a pair beyond dHat; then one geometry with n = +-e_z six times over, for the
    # degenerate evaluations: u = 0, y = eps_v, mu = 0, a u whose y^2 overflows, one whose y^3 alone does, and an ordinary one
    extra = np.array([[[.3, .3, .3], [.3, .3, .3], [.4, .3, .3], [.3, .4, .3]], [[.32, .32, .3], [.3, .3, .3], [.4, .3, .3], [.3, .4, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.3, .3, .31], [.4, .3, .31]], [[.3, .3, .3], [.3, .3, .3], [.3, .3, .3], [.3, .3, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.35, .25, .3], [.35, .35, .3]], [[.3, .3, .3], [.4, .3, .3], [.3, .3, .5], [.4, .31, .5]]], f)
    flat = {"pt": [[.32, .32, .31], [.3, .3, .3], [.4, .3, .3], [.3, .4, .3]], "ee": [[.3, .3, .3], [.4, .3, .3], [.35, .25, .31], [.35, .35, .31]]}
    for kind, P in (("pt", random_pt(n, 31)), ("ee", random_ee(n, 32))):
        special = np.tile(np.array(flat[kind], f), (6, 1, 1))
        P = tuple(np.concatenate([x, extra[:, k], special[:, k]]) for k, x in enumerate(P))
        m = len(P[0])
        kappa = np.where(np.arange(m) % 2 == 0, f(1), f(1e3)).astype(f)
        if kind == "ee":
            la, lb = rb._dot(P[1] - P[0], P[1] - P[0]), rb._dot(P[3] - P[2], P[3] - P[2])
            eps = np.where(np.arange(m) % 3 == 0, f(0), rb.ee_eps32(la, lb)).astype(f)      # every third pair unmollified
            eps[n + 2] = rb.ee_eps32(la, lb)[n + 2]                                         # the exactly parallel pair: mollified
        else:
            eps = np.zeros(m, f)
        scale = np.array([rf.SCALES[i % 3] for i in range(m)]) * EPS
        urows = (_rows(m, 61, 1.0) * scale[:, None, None]).astype(f)
        xrows = _rows(m, 62, 1.0)
        mu = np.full(m, MU, f)
        s0 = n + len(extra)
        urows[s0] = 0
        urows[s0 + 1] = 0
        urows[s0 + 1, :(1 if kind == "pt" else 2), 0] = f(EPS)      # ur = (eps_v, 0, 0): the weights of the point, or of edge i, sum to 1
        mu[s0 + 2] = 0
        urows[s0 + 3] = 0
        urows[s0 + 3, 0, 0] = f(1e25)
        urows[s0 + 4] = 0
        urows[s0 + 4, 0, 0] = f(1e15)
        rec = np.concatenate([np.stack(P, axis=1).reshape(m, 12), np.full((m, 1), dhat2, f), kappa[:, None], eps[:, None], np.zeros((m, 1), f),
                              urows.reshape(m, 12), xrows.reshape(m, 12), mu[:, None], np.full((m, 1), EPS, f), np.zeros((m, 2), f)],
                             axis=1).astype(f)
        fin, fout = str(tmp_path / (kind + ".bin")), str(tmp_path / (kind + ".out"))
        rec.tofile(fin)
        r = subprocess.run([exe, fin, fout, kind], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        i32 = np.int32
        out = np.fromfile(fout, np.dtype([("rec", f, 8), ("lag", i32), ("e", f), ("st_e", i32), ("eg", f), ("g", f, (4, 3)), ("st_g", i32),
                                          ("h", f, (4, 3)), ("st_h", i32)]))
        assert len(out) == m
        rec32, st = np.zeros((m, 8), f), np.zeros(m, i32)
        for k in np.unique(kappa):
            sel = kappa == k
            args = tuple(x[sel] for x in P) + (dhat2, k)
            rec32[sel], st[sel], _ = rf.lag_pt32(*args, log) if kind == "pt" else rf.lag_ee32(*args, eps[sel], log)
        bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
        assert np.array_equal(out["lag"], st) and np.array_equal(bits(out["rec"]), bits(rec32))
        ev = rf.evaluate32(rec32, urows, mu, f(EPS), xrows)
        for key, want in (("e", "e"), ("eg", "eg"), ("g", "g"), ("h", "h"), ("st_e", "st_e"), ("st_g", "st_g"), ("st_h", "st_h")):
            assert np.array_equal(bits(out[key]), bits(ev[want])), (kind, key)
        assert not np.isnan(out["rec"]).any() and np.isfinite(out["e"]).all() and np.isfinite(out["g"]).all() and np.isfinite(out["h"]).all()
        idle = out["lag"] != 1
        for key in ("rec", "e", "eg", "g", "h"):      # idle pairs are exactly zero, in the record and in everything computed from it
            assert (bits(out[key][idle]) == 0).all(), key
        assert (out["st_e"][idle] == 0).all() and (out["st_h"][idle] == 0).all()
        # the degenerate evaluations did what the header says
        assert out["lag"][s0] == 1 and (out["g"][s0] == 0).all() and out["e"][s0] == (mu[s0] * out["rec"][s0, 3]) * (f(EPS) / f(3))
        assert out["st_e"][s0 + 1] == 1 and abs(float(out["e"][s0 + 1]) / (MU * float(out["rec"][s0 + 1, 3]) * EPS) - 1) < 1e-5
        assert out["st_e"][s0 + 2] == 0 and out["st_h"][s0 + 2] == 0 and (bits(out["g"][s0 + 2]) == 0).all() and (bits(out["h"][s0 + 2]) == 0).all()
        assert out["st_e"][s0 + 3] == 2 and out["st_g"][s0 + 3] == 2 and out["st_h"][s0 + 3] == 2 and out["e"][s0 + 3] == 0
        assert out["st_e"][s0 + 4] == 1 and out["st_h"][s0 + 4] == 2 and (bits(out["h"][s0 + 4]) == 0).all()
        assert out["lag"][n + 5] == 0 and (out["lag"][[n + 3]] == 2).all()
        if kind == "ee":
            assert out["lag"][n + 2] == 1 and out["rec"][n + 2, 3] == 0 and out["st_e"][n + 2] == 0      # exactly parallel, mollified: m = 0
            # (records n and n + 3 have zero-length edges: one beyond dHat, one at zero distance; the crossing edges of record n + 4 are
            # a rounding apart in float32)
            assert np.isfinite(out["rec"][n + 4]).all()
        print("FRICTION host %s: %d pairs bit for bit with the replay (record, energy, gradient, product, statuses); lag status counts %s, "
              "evaluation status counts %s / %s / %s" % (kind, m, np.bincount(out["lag"], minlength=3).tolist(),
                                                         np.bincount(out["st_e"], minlength=3).tolist(),
                                                         np.bincount(out["st_g"], minlength=3).tolist(),
                                                         np.bincount(out["st_h"], minlength=3).tolist()))
        assert (out["lag"] == 2).sum() >= 1 and (out["lag"] == 0).sum() >= 1 and (out["lag"] == 1).sum() > n // 4
