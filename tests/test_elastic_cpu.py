"""Mesh elasticity without a GPU (tests/ref64_elastic.py, include/zensim_rocm/elastic_device.hpp): the entries' declarations and bindings;
the closed-form gradient and product against torch.autograd's backward and double backward in float64; the exact cases (rest, a flat
sheet, uniform stretch, a single folded hinge); the invariants of the energy, the gradient, H and H+ in float64; the float32 replay of the
device chain against the derived bounds on 100 000 random triangles and hinges; the header itself compiled for the host under the
sanitizers and compared bit for bit with the replay; and the measured constant of the vacuity guard.  Prints one `ELASTIC <what> ...` line
per check.

Measured: closed form against autograd 1.5e-16 of the largest entry at worst; replay against float64, worst error over bound: triangles
0.089 (record), 0.017 (energy), 0.002 (gradient), 0.001 (product), 0.001 (psd product), hinges 0.072 (record), 0.010 (energy), 0.015
(gradient), 0.042 (product), none unbounded; 38 262 of the 100 000 triangles have a projected stress between S and 0.  The vacuity figure:
on `sheets` at the middle displacement scale (0.1 mean edge length) the median over the 288 vertices of bound / |force| is 8.114e-3
(smallest 2.1e-3, largest 9.2e-2), computed here from the float64 reference and the module's bounds; the test asserts it at twice that
value (ref64_elastic.SHEETS_MEDIAN_BOUND_OVER_G), and tests/test_elastic_gpu.py holds the device to the same figure."""
import os
import re
import subprocess

import numpy as np
import pytest

import ref64_elastic as rl
import ref64_proximity as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU, LAM, KB = rl.MU, rl.LAM, rl.KB
ENTRIES = {"zs_rocm_mesh_set_rest_shape": 3, "zs_rocm_mesh_rest_shape_sizes": 2, "zs_rocm_mesh_rest_shape": 6, "zs_rocm_mesh_elastic_energy": 10,
           "zs_rocm_mesh_elastic_gradient": 12, "zs_rocm_mesh_elastic_hessian_product": 11}


def test_the_entries_are_declared_exported_and_bound(hiplib):
    header = open(os.path.join(ROOT, "include", "zs_rocm.h")).read()
    from zpc_amd.mesh import TriMesh
    for name, nargs in ENTRIES.items():
        assert re.search(r"ZS_ROCM_EXPORT\s+int\s+%s\(" % name, header), name + " is not declared in zs_rocm.h"
        assert len(getattr(hiplib, name).argtypes) == nargs, name
    for method in ("set_rest_shape", "rest_shape", "elastic", "elastic_hessian_product"):
        assert callable(getattr(TriMesh, method, None)), method


# ------------------------------------------------------------------------------------------------ random elements
def random_tris(n, seed, special=True):
    """(X, x, z [n, 3, 3] float32, group [n]): rest triangles with edges around 0.05 inside [0.2, 0.8]^3, deformed by 1e-3, 1e-1 or 1 edge
    length; group 1: rest-degenerate (X1 = X0, or three points on a line along an axis), 2: collapsed to a point, 3: inverted, 4: far
    enough out to overflow, 0: the rest"""
    g = np.random.default_rng(seed)
    X0 = 0.3 + 0.4 * g.random((n, 1, 3))
    X = np.concatenate([X0, X0 + 0.05 * g.standard_normal((n, 2, 3))], axis=1).astype(np.float32)
    scale = np.array(rl.SCALES)[np.arange(n) % 3]
    x = (X + 0.05 * scale[:, None, None] * g.standard_normal((n, 3, 3))).astype(np.float32)
    z = g.standard_normal((n, 3, 3)).astype(np.float32)
    group = np.zeros(n, np.int32)
    if special:
        group[:40] = np.repeat([1, 2, 3, 4], 10)
        X[:5, 1] = X[:5, 0]
        X[5:10, 1] = X[5:10, 0] + np.float32([0.03125, 0, 0])
        X[5:10, 2] = X[5:10, 0] + np.float32([0.0625, 0, 0])
        x[10:20] = x[10:20, :1]
        x[20:30] = x[20:30][:, [0, 2, 1]]
        x[30:40] *= np.float32(1e12)
        z[30:40] *= np.float32(1e12)
    return X, x, z, group


def random_hinges(n, seed, special=True):
    """the same for hinges [n, 4, 3]: two triangles over a common edge, folded by a random angle at rest"""
    g = np.random.default_rng(seed)
    X0 = 0.3 + 0.4 * g.random((n, 1, 3))
    X = np.concatenate([X0, X0 + 0.05 * g.standard_normal((n, 3, 3))], axis=1).astype(np.float32)
    scale = np.array(rl.SCALES)[np.arange(n) % 3]
    x = (X + 0.05 * scale[:, None, None] * g.standard_normal((n, 4, 3))).astype(np.float32)
    z = g.standard_normal((n, 4, 3)).astype(np.float32)
    group = np.zeros(n, np.int32)
    if special:
        group[:40] = np.repeat([1, 2, 3, 4], 10)
        X[:5, 1] = X[:5, 0]
        X[5:10, 1] = X[5:10, 0] + np.float32([0.03125, 0, 0])
        X[5:10, 2] = X[5:10, 0] + np.float32([0.0625, 0, 0])
        x[10:20] = x[10:20, :1]
        x[20:30] = x[20:30][:, [1, 0, 2, 3]]
        x[30:40] *= np.float32(1e21)
        z[30:40] = np.float32(3e38)      # times a weight above 1.2 (they are around 50): beyond the float range
    return X, x, z, group


# ------------------------------------------------------------------------------------------------ closed forms against autograd
def test_the_closed_forms_against_autograd():
    torch = pytest.importorskip("torch")
    n = 2000
    X, x, z, _ = random_tris(n, 1, special=False)
    x[::5] = (0.4 * X[::5]).astype(np.float32)      # compressed ones: the stress has negative eigenvalues
    X64, z64 = X.astype(np.float64), z.astype(np.float64)
    rec, _ = rl.tri_rest(X64[:, 0], X64[:, 1], X64[:, 2])
    r = rl.tri_eval(rec, x.astype(np.float64), MU, LAM, z64)
    xt, B = torch.tensor(x.astype(np.float64), requires_grad=True), torch.tensor(rec)
    d1, d2 = xt[:, 1] - xt[:, 0], xt[:, 2] - xt[:, 0]
    F = torch.stack([B[:, 0, None] * d1, B[:, 1, None] * d1 + B[:, 2, None] * d2], dim=2)
    E = 0.5 * (F.transpose(1, 2) @ F - torch.eye(2, dtype=torch.float64))
    psi = (B[:, 3] * (MU * (E * E).sum(dim=(1, 2)) + LAM / 2 * (E[:, 0, 0] + E[:, 1, 1]) ** 2)).sum()
    ga, = torch.autograd.grad(psi, xt, create_graph=True)
    ha, = torch.autograd.grad((ga * torch.tensor(z64)).sum(), xt)
    worst = [np.abs(r["g"] - ga.detach().numpy()).max() / np.abs(r["g"]).max(), np.abs(r["h"] - ha.numpy()).max() / np.abs(r["h"]).max()]
    X, x, z, _ = random_hinges(n, 2, special=False)
    X64, z64 = X.astype(np.float64), z.astype(np.float64)
    k, _ = rl.hinge_rest(X64[:, 0], X64[:, 1], X64[:, 2], X64[:, 3])
    r = rl.hinge_eval(k, x.astype(np.float64), KB, z64)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    w = (torch.tensor(k)[:, :, None] * xt).sum(dim=1)
    psi = (KB / 2 * (w * w).sum(dim=1)).sum()
    ga, = torch.autograd.grad(psi, xt, create_graph=True)
    ha, = torch.autograd.grad((ga * torch.tensor(z64)).sum(), xt)
    worst += [np.abs(r["g"] - ga.detach().numpy()).max() / np.abs(r["g"]).max(), np.abs(r["h"] - ha.numpy()).max() / np.abs(r["h"]).max()]
    print("ELASTIC autograd: %d triangles and hinges; closed form - autograd over the largest entry: membrane gradient %.2e, product %.2e, "
          "bending gradient %.2e, product %.2e" % (n, worst[0], worst[1], worst[2], worst[3]))
    assert max(worst) <= 1e-7      # both sides float64: the project's tolerance for closed forms against autograd
    assert abs(k.sum(axis=1)).max() <= 1e-9 * np.abs(k).max()      # the bending weights sum to zero


# ------------------------------------------------------------------------------------------------ exact cases
def test_at_rest_a_flat_sheet_and_a_uniform_stretch():
    v, t = rp.grid_sheet(12, 0.5, 0.6, 1)
    v[:, 2] = 0.5      # jittered in the plane only: flat
    R64, R32 = rl.Rest(v, t), rl.Rest(v, t, np.float32)
    assert R64.counts == (0, 0, 0) and len(R64.hinges) == len(rp.edges(t)) - 4 * 11
    T, H, grad, _ = R64.evaluate(v, MU, LAM, KB)
    x = v.astype(np.float64)[R64.tris]
    be, bg, _ = rl.tri_bounds(x, x, R64.tri_record, MU, LAM)
    assert np.abs(T["E"]).max() <= 1e-14      # F^T F = I in float64
    T32, H32, grad32, _ = R32.evaluate(v, MU, LAM, KB)
    f = np.sqrt(2.0)
    dE = 2 * rl.U * (f * f + 1) + f * (2 * rl.K_REC * 4 + 4) * rl.U * f      # the module's dE at |F| = sqrt(2), aspect below 4
    assert np.abs(T32["E"]).max() <= dE and (np.abs(T32["e"]) <= be).all() and (rl._norm(T32["g"]) <= bg[:, None]).all()
    xh = v.astype(np.float64)[R64.hinges]
    he, hg, _ = rl.hinge_bounds(xh, xh, KB)
    assert np.abs(H["e"]).max() <= 1e-20 and (H32["e"] <= he).all() and (rl._norm(H32["g"]) <= hg).all()
    print("ELASTIC at rest[flat jittered sheet]: %d triangles, %d hinges; float64 |E| %.1e, bending energy %.1e; float32 |E| %.2e (bound %.2e), "
          "largest bending energy %.2e (bound %.2e)" % (len(t), len(R64.hinges), np.abs(T["E"]).max(), H["e"].max(), np.abs(T32["E"]).max(), dE,
                                                        H32["e"].max(), he.max()))
    area = R64.tri_record[:, 3].sum()
    assert abs(R64.vertex_area.sum() - area) <= 1e-12 * area
    for s in (0.5, 1.25):
        c = v.astype(np.float64).mean(axis=0)
        xs = c + s * (v.astype(np.float64) - c)
        T = rl.tri_eval(R64.tri_record, xs[R64.tris], MU, LAM)
        e = (s * s - 1) / 2
        want = area * 2 * (MU + LAM) * e * e
        Hh = rl.hinge_eval(R64.hinge_record, xs[R64.hinges], KB)
        print("ELASTIC stretch %g: membrane energy %.12e, area 2 (mu + lam) e^2 = %.12e; bending %.1e" % (s, T["e"].sum(), want, Hh["e"].sum()))
        assert abs(T["e"].sum() - want) <= 1e-12 * want and Hh["e"].sum() <= 1e-18


def test_a_single_hinge_folded_by_an_angle():
    X = np.array([[0, 0, 0.], [1, 0.1, 0], [0.3, 0.9, 0], [0.6, -0.8, 0]])
    k, st = rl.hinge_rest(X[None, 0], X[None, 1], X[None, 2], X[None, 3])
    cr = lambda a, b: np.linalg.norm(np.cross(a, b))
    A0, A1, L = cr(X[1] - X[0], X[2] - X[0]) / 2, cr(X[1] - X[0], X[3] - X[0]) / 2, np.linalg.norm(X[1] - X[0])
    for th in (0.01, 0.1, 1.0, 3.0):
        e = (X[1] - X[0]) / L
        p = X[3] - X[0]
        Y = X.copy()
        Y[3] = X[0] + p * np.cos(th) + np.cross(e, p) * np.sin(th) + e * (e @ p) * (1 - np.cos(th))
        got = rl.hinge_eval(k, Y[None], KB)["e"][0]
        want = KB / 2 * 3 * L * L / (A0 + A1) * (2 * np.sin(th / 2)) ** 2
        print("ELASTIC fold %g: energy %.15e, kb / 2 3 L^2 / (A0 + A1) (2 sin(th / 2))^2 = %.15e" % (th, got, want))
        assert abs(got - want) <= 1e-12 * want


# ------------------------------------------------------------------------------------------------ invariants
def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


@pytest.mark.parametrize("name", ["sheets", "torus", "fan"])
def test_the_invariants_in_float64(name):
    v, t, _ = rp.scene(name)
    R = rl.Rest(v, t)
    nv = len(v)
    g = np.random.default_rng(7)
    zx, zy = g.standard_normal((nv, 3)).astype(np.float32), g.standard_normal((nv, 3)).astype(np.float32)
    for what, pos in (("1e-1", rl.displaced(v, t, 1, 1e-1)), ("1", rl.displaced(v, t, 1, 1.0)), ("s = 0.5", rl.compressed(v, 0.5)),
                      ("s = 1.3", rl.compressed(v, 1.3))):
        T, H, grad, hx = R.evaluate(pos, MU, LAM, KB, zx)
        Ty, Hy, _, hy = R.evaluate(pos, MU, LAM, KB, zy)
        Tp, Hp, _, hpx = R.evaluate(pos, MU, LAM, KB, zx, psd=True)
        energy = T["e"].sum() + H["e"].sum()
        # rigid motions leave the energy unchanged (in float64: evaluate rounds positions to float32, so the elements are moved directly)
        Q, c = _rotation(3), np.array([0.3, -1.1, 0.7])
        moved = pos.astype(np.float64) @ Q.T + c
        em = rl.tri_eval(R.tri_record, moved[R.tris], MU, LAM)["e"].sum() + rl.hinge_eval(R.hinge_record, moved[R.hinges], KB)["e"].sum()
        size = np.abs(T["e"]).sum() + np.abs(H["e"]).sum()
        assert abs(em - energy) <= 1e-11 * size + 1e-11 * KB * np.abs(R.hinge_record).max() ** 2
        # per element: the terms sum to zero (membrane exactly by construction, bending to the sum of the weights) and carry no torque
        x64 = pos.astype(np.float64)
        for D, elems in ((T, R.tris), (H, R.hinges)):
            mag = np.abs(D["g"]).sum(axis=(1, 2)) + 1e-300
            assert (np.abs(D["g"].sum(axis=1)).max(axis=1) <= 1e-9 * mag).all()
            torque = np.cross(x64[elems] - x64[elems[:, :1]], D["g"]).sum(axis=1)
            assert (np.abs(torque).max(axis=1) <= 1e-9 * mag * np.abs(x64[elems] - x64[elems[:, :1]]).max(axis=(1, 2)) + 1e-300).all()
        dot = lambda a, b: float((a * b.astype(np.float64)).sum())
        mag = sum(np.abs(D["h"]).sum() for D in (T, H)) * np.abs(zy).max()
        yx, xy, xx, xpx = dot(hx, zy), dot(hy, zx), dot(hx, zx), dot(hpx, zx)
        assert abs(yx - xy) <= 1e-12 * mag
        assert xpx >= -1e-12 * mag and xpx - xx >= -1e-12 * mag
        if what == "s = 1.3":      # stretched everywhere: S is positive definite and H+ = H
            assert (np.linalg.eigvalsh(np.stack([T["S"][:, [0, 1]], T["S"][:, [1, 2]]], axis=1)) > 0).all()
            R32 = rl.Rest(v, t, np.float32)
            a, b = R32.evaluate(pos, MU, LAM, KB, zx)[0], R32.evaluate(pos, MU, LAM, KB, zx, psd=True)[0]
            assert np.array_equal(a["h"].view(np.uint32), b["h"].view(np.uint32)) and np.abs(a["h"]).max() > 0
        if what == "s = 0.5":
            assert (T["S"][:, 0] + T["S"][:, 2] < 0).all() and xpx > xx
        print("ELASTIC invariants[%s, %s]: energy %.6e (moved rigidly %.6e), y^T H x %.6e, x^T H y %.6e, x^T H x %.6e, x^T H+ x %.6e" %
              (name, what, energy, em, yx, xy, xx, xpx))


# ------------------------------------------------------------------------------------------------ the float32 replay on random elements
def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((err == 0) | np.isinf(bound), 0.0, err / bound)


def _tri_rec_bound(X64, rec64):
    c = 1.0 / rec64[:, 2]
    kap = np.maximum(rl._norm(X64[:, 2] - X64[:, 0]) / c, 1.0)
    nB = np.sqrt((rec64[:, :3] ** 2).sum(axis=1))
    return rl.K_REC * rl.U * kap[:, None] * np.stack([nB, nB, nB, rec64[:, 3]], axis=1), kap


def test_float32_replay_stays_within_the_bounds():
    n = 100000
    X, x, z, group = random_tris(n, 11)
    X64, x64, z64 = X.astype(np.float64), x.astype(np.float64), z.astype(np.float64)
    rec64, st64 = rl.tri_rest(X64[:, 0], X64[:, 1], X64[:, 2])
    rec32, st32 = rl.tri_rest(X[:, 0], X[:, 1], X[:, 2])
    assert np.array_equal(st32, st64) and ((st32 == rl.DEGENERATE) == (group == 1)).all() and (rec32[group == 1] == 0).all()
    with np.errstate(all="ignore"):
        brec, kap = _tri_rec_bound(X64, rec64)
    act = st64 == rl.ACTIVE
    worst = dict(record=_ratio(np.abs(rec32 - rec64), brec)[act].max())
    be, bg, bh = rl.tri_bounds(X64, x64, rec64, MU, LAM, z64)
    ref, ref_psd = rl.tri_eval(rec64, x64, MU, LAM, z64), rl.tri_eval(rec64, x64, MU, LAM, z64, psd=True)
    r32, r32_psd = rl.tri_eval(rec32, x, MU, LAM, z), rl.tri_eval(rec32, x, MU, LAM, z, psd=True)
    over = group == 4
    for r in (r32, r32_psd):
        assert all(np.isfinite(r[k]).all() for k in ("e", "eg", "g", "h"))
        assert ((r["st_g"] == rl.OVERFLOW) == over).all() and ((r["st_h"] == rl.OVERFLOW) == over).all() and (r["st_e"][over] == rl.OVERFLOW).all()
        assert (r["g"][over] == 0).all() and (r["h"][over] == 0).all() and (r["e"][over] == 0).all() and (r["eg"][over] == 0).all()
        assert (r["st_e"][group == 1] == rl.IDLE).all() and (r["g"][group == 1] == 0).all() and (r["h"][group == 1] == 0).all()
    keep = act & ~over
    worst["energy"] = _ratio(np.abs(r32["e"] - ref["e"]), be)[keep].max()
    worst["gradient"] = _ratio(rl._norm(r32["g"] - ref["g"]), bg[:, None])[keep].max()
    worst["product"] = _ratio(rl._norm(r32["h"] - ref["h"]), bh[:, None])[keep].max()
    worst["psd product"] = _ratio(rl._norm(r32_psd["h"] - ref_psd["h"]), bh[:, None])[keep].max()
    mixed = (ref_psd["T"] != ref["S"]).any(axis=1) & (ref_psd["T"] != 0).any(axis=1)
    unbounded = keep & ~(np.isfinite(be) & np.isfinite(bg) & np.isfinite(bh))
    print("ELASTIC replay triangles: %d, %d active, %d overflowing, largest aspect %.1f, %d with a projected stress between S and 0; worst error "
          "over bound: %s; %d unbounded" % (n, act.sum(), over.sum(), kap[keep].max(), mixed.sum(), ", ".join("%s %.3f" % kv for kv in worst.items()),
                                            unbounded.sum()))
    assert max(worst.values()) <= 1 and unbounded.sum() == 0 and mixed.sum() > n // 20

    X, x, z, group = random_hinges(n, 12)
    X64, x64, z64 = X.astype(np.float64), x.astype(np.float64), z.astype(np.float64)
    k64, st64, q, cmax, chi = rl.hinge_rest(X64[:, 0], X64[:, 1], X64[:, 2], X64[:, 3], details=True)
    k32, st32 = rl.hinge_rest(X[:, 0], X[:, 1], X[:, 2], X[:, 3])
    assert np.array_equal(st32, st64) and ((st32 == rl.DEGENERATE) == (group == 1)).all() and (k32[group == 1] == 0).all()
    act, over = st64 == rl.ACTIVE, group == 4
    with np.errstate(all="ignore"):
        dk = rl.K_HINGE * rl.U * chi * q * (1 + cmax)
    worst = dict(record=_ratio(np.abs(k32 - k64), dk[:, None])[act].max())
    be, bg, bh = rl.hinge_bounds(X64, x64, KB, z64)
    ref, r32 = rl.hinge_eval(k64, x64, KB, z64), rl.hinge_eval(k32, x, KB, z)
    assert all(np.isfinite(r32[k]).all() for k in ("e", "eg", "g", "h"))
    assert ((r32["st_g"] == rl.OVERFLOW) == over).all() and ((r32["st_h"] == rl.OVERFLOW) == over).all()
    assert (r32["g"][over] == 0).all() and (r32["h"][over] == 0).all() and (r32["e"][over] == 0).all()
    keep = act & ~over
    worst["energy"] = _ratio(np.abs(r32["e"] - ref["e"]), be)[keep].max()
    worst["gradient"] = _ratio(rl._norm(r32["g"] - ref["g"]), bg)[keep].max()
    worst["product"] = _ratio(rl._norm(r32["h"] - ref["h"]), bh)[keep].max()
    unbounded = keep & ~(np.isfinite(be) & np.isfinite(bg).all(axis=1) & np.isfinite(bh).all(axis=1))
    print("ELASTIC replay hinges: %d, %d active, %d overflowing, largest 1 / sin %.1f; worst error over bound: %s; %d unbounded" %
          (n, act.sum(), over.sum(), chi[keep].max(), ", ".join("%s %.3f" % kv for kv in worst.items()), unbounded.sum()))
    assert max(worst.values()) <= 1 and unbounded.sum() == 0


def vacuity(name="sheets", scale=rl.SCALES[1]):
    """(bound / |force| per vertex with a force, the count of vertices) on a scene at a displacement scale, from the float64 reference"""
    v, t, _ = rp.scene(name)
    R = rl.Rest(v, t)
    pos = rl.displaced(v, t, 1, scale)
    T, H, grad, _ = R.evaluate(pos, MU, LAM, KB)
    bound = R.vertex_bounds(pos, MU, LAM, KB, T, H)[0]
    size = np.linalg.norm(grad, axis=1)
    return bound[size > 0] / size[size > 0], len(v)


def test_the_vacuity_guard_constant_is_the_measured_one():
    ratio, nv = vacuity()
    med = float(np.median(ratio))
    print("ELASTIC vacuity[sheets, 1e-1 edge]: %d vertices, bound / |force| median %.3e (constant %.3e), smallest %.2e, largest %.2e" %
          (len(ratio), med, rl.SHEETS_MEDIAN_BOUND_OVER_G, ratio.min(), ratio.max()))
    assert len(ratio) == nv
    assert med <= 2 * rl.SHEETS_MEDIAN_BOUND_OVER_G
    assert med < 1e-2       # a bound that says something: the median vertex is held to better than a percent of its elastic force


# ------------------------------------------------------------------------------------------------ the header on the host
def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_elastic")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_elastic.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    f, i32, n = np.float32, np.int32, 50000
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for kind, (X, x, z, group) in (("tri", random_tris(n, 31)), ("hinge", random_hinges(n, 32))):
        N = X.shape[1]
        pad = lambda a: np.concatenate([a, np.zeros((n, 4 - N, 3), f)], axis=1).reshape(n, 12)
        mu = np.where(np.arange(n) % 7 == 0, f(0), f(MU)).astype(f)      # mu = 0 with lam > 0 is an ordinary input
        lam, kb = np.full(n, LAM, f), np.where(np.arange(n) % 2 == 0, f(KB), f(50)).astype(f)
        rows = np.concatenate([pad(X), pad(x), pad(z), mu[:, None], lam[:, None], kb[:, None], np.zeros((n, 1), f)], axis=1).astype(f)
        fin, fout = str(tmp_path / (kind + ".bin")), str(tmp_path / (kind + ".out"))
        rows.tofile(fin)
        r = subprocess.run([exe, fin, fout, kind], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        out = np.fromfile(fout, np.dtype([("rec", f, 4), ("st", i32), ("e", f), ("st_e", i32), ("eg", f), ("g", f, (4, 3)), ("st_g", i32),
                                          ("h", f, (4, 3)), ("st_h", i32), ("hp", f, (4, 3)), ("st_p", i32)]))
        assert len(out) == n
        if kind == "tri":
            rec, st = rl.tri_rest(X[:, 0], X[:, 1], X[:, 2])
            ev, evp = rl.tri_eval(rec, x, mu, lam, z), rl.tri_eval(rec, x, mu, lam, z, psd=True)
        else:
            rec, st = rl.hinge_rest(X[:, 0], X[:, 1], X[:, 2], X[:, 3])
            ev = evp = rl.hinge_eval(rec, x, kb, z)
        assert np.array_equal(out["st"], st) and np.array_equal(bits(out["rec"]), bits(rec)), kind
        for key, want in (("e", ev["e"]), ("eg", ev["eg"]), ("g", ev["g"]), ("h", ev["h"]), ("hp", evp["h"]), ("st_e", ev["st_e"]),
                          ("st_g", ev["st_g"]), ("st_h", ev["st_h"]), ("st_p", evp["st_h"])):
            got = out[key][:, :N] if out[key].ndim == 3 else out[key]
            assert np.array_equal(bits(got), bits(want)), (kind, key)
        for key in ("rec", "e", "eg", "g", "h", "hp"):
            assert not np.isnan(out[key]).any(), key
        idle = out["st"] != rl.ACTIVE
        for key in ("rec", "e", "eg", "g", "h", "hp"):      # degenerate rest elements are exactly zero, in the record and in everything after it
            assert (bits(out[key][idle]) == 0).all(), key
        assert idle.sum() == 10 and (out["st_g"][group == 4] == rl.OVERFLOW).all() and (bits(out["g"][group == 4]) == 0).all()
        assert (out["st_g"][group == 2] == rl.ACTIVE).all() and (out["st_g"][group == 3] == rl.ACTIVE).all()
        if kind == "tri":
            assert (bits(out["hp"]) != bits(out["h"])).any(axis=(1, 2)).sum() > n // 20      # the projection is at work
        print("ELASTIC host %s: %d elements bit for bit with the replay (record, energy, gradient, product, psd product, statuses); record "
              "status counts %s, gradient status counts %s" % (kind, n, np.bincount(out["st"], minlength=4).tolist(),
                                                               np.bincount(out["st_g"], minlength=4).tolist()))
