"""Mesh friction on the GPU (the friction operations of zpc_amd/csrc/mesh_barrier.hip, TriMesh.friction_lag / friction /
friction_hessian_product) against tests/ref64_friction.py: the lag record on every scene of ref64_proximity.SCENES, mollified and not and at
trial positions (n, w and the pair's d2 bit for bit with the float32 replay, n and lambda against float64 within the pair bounds); energy,
gradient and product from the device's own record bit for bit with the replay, and grad / hx with the gather replayed in list order; lists
cut at the workgroup edges; determinism on `large`; a side that is None; indices outside the mesh; mu = 0; a pair at zero distance; the
invariants within the bounds; lag and evaluation end to end against float64 on `sheets`; the argument checks.  No pair and no vertex is
left out of a comparison: where a bound is infinite the line printed says how many.  Prints one `FRICTION <what> ...` line per check.

Measured on an MI355X: every bit-for-bit comparison holds; lag record against float64: n 0.462 of its bound at worst (stack), lambda 0.044
(torus), a weight at its cap of 1 on torus (1.000), 4 pairs of `stack` unbounded; end to end on `sheets`: worst pair energy 0.006, vertex
gradient 0.004, vertex product 0.005 of the bound, median bound / |g| 4.6e-3 .. 5.1e-3 over the three scales; most incidences at one vertex
821 (fan); the file runs in 3.0 s."""
import functools

import numpy as np
import pytest

import ref64_barrier as rb
import ref64_friction as rf
import ref64_proximity as rp
import ref64_terms as rt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
KAPPA, MU, EPS = 1.0, rf.MU, rf.EPS_V


@functools.lru_cache(maxsize=None)
def _scene(name):
    v, t, dhat = rp.scene(name)
    e = rp.edges(t)
    return v, t, e, dhat, rb.rest_len2(v, e)


def _mesh(pol, name):
    from zpc_amd.mesh import TriMesh
    v, t, _, dhat, _ = _scene(name)
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    return mesh, dhat


def _np(x):
    return None if x is None else x.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pairs(prox):
    z = np.zeros((0, 2), np.int32)
    return (z if prox.pt_pairs is None else _np(prox.pt_pairs)), (z if prox.ee_pairs is None else _np(prox.ee_pairs))


def _verts_of(t, e, pt, ee):
    """the four corner vertices of every pair, PT then EE"""
    t, e = np.asarray(t, np.int64).reshape(-1, 3), np.asarray(e, np.int64).reshape(-1, 2)
    return np.concatenate([np.concatenate([pt[:, :1].astype(np.int64), t[pt[:, 1]]], axis=1).reshape(-1, 4),
                           np.concatenate([e[ee[:, 0]], e[ee[:, 1]]], axis=1).reshape(-1, 4)])


def _replay_lag(mesh, verts, t, e, pt, ee, dhat, mollify):
    """the float32 replay of the lag step on the lists: (record [npt + nee, 8], status, d2)"""
    v = np.asarray(verts, np.float32)
    vert = _verts_of(t, e, pt, ee)
    P = [v[vert[:len(pt), k]] for k in range(4)]
    Q = [v[vert[len(pt):, k]] for k in range(4)]
    dhat2 = np.float32(rb.dhat2_f32(dhat))
    rest = _np(mesh.rest())
    eps = rb.ee_eps32(rest[ee[:, 0]], rest[ee[:, 1]]) if mollify else np.zeros(len(ee), np.float32)
    a, b = rf.lag_pt32(*P, dhat2, KAPPA), rf.lag_ee32(*Q, dhat2, KAPPA, eps)
    return tuple(np.concatenate([a[k], b[k]]) for k in range(3))


def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((err == 0) | np.isinf(bound), 0.0, err / bound)


def _check_lag(what, mesh, lag, verts, t, e, dhat, mollify, rest2, own_d2=None):
    """one FrictionLag against the replay (bits) and against float64 (bounds); returns the float64 lag dicts"""
    pt, ee = _pairs(lag.prox)
    rec = _np(lag.record)
    assert rec.shape == (len(pt) + len(ee), 8) and rec.dtype == np.float32 and np.isfinite(rec).all()
    assert np.array_equal(_np(lag.normal), rec[:, :3]) and np.array_equal(_np(lag.lam), rec[:, 3]) and np.array_equal(_np(lag.weights), rec[:, 4:])
    r32, st, d2 = _replay_lag(mesh, verts, t, e, pt, ee, dhat, mollify)
    # everything but lambda has no logarithm in its chain: the bits of the replay.  (Active or not does not depend on the logarithm
    # either, unless b' leaves the float range.)
    assert np.array_equal(_bits(rec[:, :3]), _bits(r32[:, :3])) and np.array_equal(_bits(rec[:, 4:]), _bits(r32[:, 4:])), what
    assert np.array_equal(rec[:, 3] == 0, r32[:, 3] == 0)
    if own_d2 is not None:      # the replay's d2 is the device's: the proximity pass computed it at the same positions with the same code
        assert np.array_equal(_bits(d2), _bits(own_d2)), what
    dhat2 = rb.dhat2_f32(dhat)
    M = rp.coord_max(verts)
    qp = rf.lag_pt64(verts, t, pt, dhat2, KAPPA, M)
    qe = rf.lag_ee64(verts, e, ee, dhat2, KAPPA, rest2 if mollify else None, M)
    r64 = np.concatenate([qp["rec"], qe["rec"]])
    dn, dlam = np.concatenate([qp["dn"], qe["dn"]]), np.concatenate([qp["dlam"], qe["dlam"]])
    rn = _ratio(rb._norm(rec[:, :3].astype(np.float64) - r64[:, :3]), dn)
    rl = _ratio(np.abs(rec[:, 3].astype(np.float64) - r64[:, 3]), dlam)
    rw = _ratio(np.abs(rec[:, 4:].astype(np.float64) - r64[:, 4:]), np.concatenate([qp["dw"], qe["dw"]]))
    top = lambda r: r.max() if len(r) else 0.0
    print("FRICTION lag %s: %d PT, %d EE pairs, %d active; n, w and d2 bit for bit with the replay; against float64: n %.3f, lambda %.3f, w %.3f "
          "of the bound; unbounded: n %d, lambda %d; largest lambda %.3e" %
          (what, len(pt), len(ee), (rec[:, 3] != 0).sum(), top(rn), top(rl), top(rw), np.isinf(dn).sum(), np.isinf(dlam).sum(),
           rec[:, 3].max() if len(rec) else 0.0))
    assert (rn <= 1).all() and (rl <= 1).all() and (rw <= 1).all(), what
    return qp, qe


# ------------------------------------------------------------------------------------------------ 1: the lag record
# unmollified without `regular`, as in test_barrier_gpu.py: between its exactly parallel edges only the mollified potential is defined
@pytest.mark.parametrize("name,mollify", [(n, True) for n in rp.SCENES] + [(n, False) for n in rp.SCENES if n != "regular"])
def test_the_lag_record_against_the_replay_and_the_float64_reference(pol, name, mollify):
    mesh, dhat = _mesh(pol, name)
    v, t, e, _, rest2 = _scene(name)
    prox = mesh.proximity(dhat)
    lag = mesh.friction_lag(prox, dhat, KAPPA, mollify=mollify)
    own = np.concatenate([_np(prox.pt_dist2), _np(prox.ee_dist2)])
    _check_lag("%s (mollify %s)" % (name, mollify), mesh, lag, v, t, e, dhat, mollify, rest2, own)
    assert lag.zero_distance == (0, 0) and lag.prox is prox
    rec = _np(lag.record)
    if name == "tiny0":
        assert len(rec) == 0
        F = mesh.friction(lag, np.zeros((mesh.nv, 3), np.float32), MU, EPS)
        assert float(F.energy.item()) == 0.0 and (_np(F.grad) == 0).all() and len(F.pt_energy) == 0 and len(F.ee_energy) == 0
        H = mesh.friction_hessian_product(lag, np.zeros((mesh.nv, 3), np.float32), MU, EPS, rf.displacement(mesh.nv, 3, 1.0))
        assert (_np(H.hx) == 0).all() and len(H.pair_terms) == 0 and F.overflow == (0, 0) and H.overflow == (0, 0)
    if name == "tiny1":
        assert len(prox.ee_pairs) == 0 and len(prox.pt_pairs) > 0 and (rec[:, 3] > 0).all()
    if name in ("sheets", "regular", "torus", "fan", "stack"):
        assert (rec[:, 3] > 0).sum() > len(rec) // 2
        # the weights sum to zero, to the rounding of 1 - s, 1 - t or 1 - b1 - b2
        act = rec[:, 3] > 0
        assert np.abs(rec[act, 4:].astype(np.float64).sum(axis=1)).max() <= 8 * rf.U


def test_the_lag_record_at_trial_positions(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _, rest2 = _scene("sheets")
    prox = mesh.proximity(dhat)
    moved = (v + 2e-3 * (np.random.default_rng(7).random(v.shape) - 0.5)).astype(np.float32)
    lag = mesh.friction_lag(prox, dhat, KAPPA, verts=moved)
    _check_lag("sheets, trial positions", mesh, lag, moved, t, e, dhat, True, rest2)
    assert _np(lag.record).tobytes() != _np(mesh.friction_lag(prox, dhat, KAPPA).record).tobytes()


def test_a_pair_at_zero_distance_is_counted_and_gets_a_zero_record(pol):
    from zpc_amd.mesh import TriMesh
    v = np.array([[0.3, 0.3, 0.5], [0.5, 0.3, 0.5], [0.3, 0.5, 0.5], [0.35, 0.35, 0.5], [0.45, 0.4, 0.56], [0.4, 0.45, 0.56]], np.float32)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    prox = mesh.proximity(0.05)
    row = _np(prox.pt_pairs).tolist().index([3, 0])
    lag = mesh.friction_lag(prox, 0.05, KAPPA)
    rec = _np(lag.record)
    assert lag.zero_distance == (1, 0) and (_bits(rec[row]) == 0).all() and (rec[:, 3] > 0).sum() > 0 and np.isfinite(rec).all()
    F = mesh.friction(lag, rf.displacement(6, 1, EPS), MU, EPS)
    assert _np(F.pt_energy)[row] == 0 and np.isfinite(_np(F.grad)).all() and float(F.energy.item()) > 0 and F.overflow == (0, 0)


# ------------------------------------------------------------------------------------------------ 2: evaluation from the device's own record
def _gradient_terms(pol, mesh, lag, u):
    """the [4][3] records of the gradient call, which TriMesh.friction does not return: the C entry on the incidence kept on lag.prox"""
    from zpc_amd import lib
    p = lag.prox
    starts, entries, nscratch = p._incidence
    scratch = torch.empty(nscratch, dtype=torch.float32, device="cuda")
    grad = torch.empty(mesh.nv, 3, dtype=torch.float32, device="cuda")
    ud = torch.from_numpy(u).cuda()
    ptr = lambda x: None if x is None else x.data_ptr()
    npt, nee = (0 if p.pt_pairs is None else len(p.pt_pairs)), (0 if p.ee_pairs is None else len(p.ee_pairs))
    assert lib().zs_rocm_mesh_friction_gradient(pol.handle, mesh.handle, ud.data_ptr(), ptr(p.pt_pairs), npt, ptr(p.ee_pairs), nee,
                                                lag.record.data_ptr(), MU, EPS, starts.data_ptr(), entries.data_ptr(), scratch.data_ptr(), None,
                                                None, None, grad.data_ptr(), None) == 0
    pol.syncCtx()
    return _np(scratch).reshape(-1, 4, 3), _np(grad)


def _check_evaluation(what, pol, mesh, lag, t, e, u, x, mu=MU):
    """energy, gradient and product of the device against the float32 replay on the record read back; returns (Friction, product)"""
    pt, ee = _pairs(lag.prox)
    npt = len(pt)
    vert = _verts_of(t, e, pt, ee)
    rec = _np(lag.record)
    ev = rf.evaluate32(rec, u[vert], mu, EPS, x[vert])
    F, E, H = mesh.friction(lag, u, mu, EPS), mesh.friction(lag, u, mu, EPS, gradient=False), mesh.friction_hessian_product(lag, u, mu, EPS, x)
    assert E.grad is None and F.energy.dtype == torch.float64
    got = lambda r: np.concatenate([a for a in (_np(r.pt_energy), _np(r.ee_energy)) if a is not None] or [np.zeros(0, np.float32)])
    assert np.array_equal(_bits(got(F)), _bits(ev["eg"])) and np.array_equal(_bits(got(E)), _bits(ev["e"])), what
    overflow = lambda st: (int((st[:npt] == 2).sum()), int((st[npt:] == 2).sum()))
    assert F.overflow == overflow(ev["st_g"]) and E.overflow == overflow(ev["st_e"]) and H.overflow == overflow(ev["st_h"]), what
    terms = _np(H.pair_terms)
    assert np.array_equal(_bits(terms), _bits(ev["h"])), what
    nv = mesh.nv
    assert np.array_equal(_bits(_np(H.hx)), _bits(rf.gather32(terms, vert, nv))), what
    if mu == MU:
        gterms, grad = _gradient_terms(pol, mesh, lag, u)
        assert np.array_equal(_bits(gterms), _bits(ev["g"])) and grad.tobytes() == _np(F.grad).tobytes(), what
    assert np.array_equal(_bits(_np(F.grad)), _bits(rf.gather32(ev["g"], vert, nv))), what
    total, own = float(F.energy.item()), float(got(F).astype(np.float64).sum())      # the total is the sum of the energies it returns
    assert (total == own or abs(total - own) <= 1e-13 * own) and _np(E.energy).tobytes() == _np(F.energy).tobytes()
    assert _np(F.energy).tobytes() == np.float64(rt.total(got(F))).tobytes(), what      # the reduction of ref64_terms, bit for bit
    return F, H


@pytest.mark.parametrize("name", rp.SCENES)
def test_energy_gradient_and_product_from_the_devices_own_record(pol, name):
    mesh, dhat = _mesh(pol, name)
    v, t, e, _, _ = _scene(name)
    prox = mesh.proximity(dhat)
    lag = mesh.friction_lag(prox, dhat, KAPPA)
    x = rf.displacement(mesh.nv, 3, 1.0)
    pt, ee = _pairs(prox)
    ninc = np.bincount(_verts_of(t, e, pt, ee).ravel(), minlength=mesh.nv)
    for scale in rf.SCALES:
        u = rf.displacement(mesh.nv, 1, scale * EPS)
        F, H = _check_evaluation("%s, u = %g eps_v" % (name, scale), pol, mesh, lag, t, e, u, x)
        g, hx = _np(F.grad), _np(H.hx)
        assert np.isfinite(g).all() and np.isfinite(hx).all() and (g[ninc == 0] == 0).all() and (hx[ninc == 0] == 0).all()
        print("FRICTION evaluation[%s, u = %g eps_v]: %d PT, %d EE pairs: energies, gradient terms, product terms, grad and hx bit for bit "
              "with the replay; energy %.6e, largest |g| %.3e, largest |Hx| %.3e, most incidences at one vertex %d" %
              (name, scale, len(pt), len(ee), float(F.energy.item()), np.abs(g).max() if len(g) else 0, np.abs(hx).max() if len(hx) else 0,
               ninc.max()))
        assert F.overflow == (0, 0) and H.overflow == (0, 0)
        if name in ("sheets", "regular", "torus", "fan", "stack"):
            assert float(F.energy.item()) > 0 and np.abs(g).max() > 0 and np.abs(hx).max() > 0
    if name in ("fan", "stack"):      # runs longer than a wave
        assert ninc.max() > 64
    if name == "stack":      # the total's two arrays meet inside a chunk of 4096, off a multiple of 256
        assert len(pt) + len(ee) > 4096 and len(pt) % 256 != 0 and len(pt) % 4096 != 0
    if name == "tiny0":
        assert len(pt) + len(ee) == 0


def test_a_displacement_beyond_the_float_range_is_counted_and_adds_nothing(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _, _ = _scene("sheets")
    lag = mesh.friction_lag(mesh.proximity(dhat), dhat, KAPPA)
    u = rf.displacement(mesh.nv, 1, EPS)
    u[: mesh.nv // 2] *= np.float32(1e28)      # the lower sheet: |ut|^2 of every pair between the sheets overflows
    F, H = _check_evaluation("sheets, overflow", pol, mesh, lag, t, e, u, rf.displacement(mesh.nv, 3, 1.0))
    print("FRICTION overflow[sheets]: %s PT, EE pairs counted by the gradient call, %s by the product; everything finite" % (F.overflow, H.overflow))
    assert F.overflow[0] > 100 and F.overflow[1] > 100 and np.isfinite(_np(F.grad)).all() and np.isfinite(_np(H.hx)).all()
    assert np.isfinite(float(F.energy.item()))


# ------------------------------------------------------------------------------------------------ 3: workgroup edges
def _cut(prox, n):
    from zpc_amd.mesh import Proximity
    p = Proximity()
    p.pt_pairs, p.ee_pairs = prox.pt_pairs[:n].contiguous(), prox.ee_pairs[:n].contiguous()
    return p


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_lists_cut_at_the_workgroup_edges_give_the_same_bytes_per_pair(pol, n):
    mesh, dhat = _mesh(pol, "sheets")
    full = mesh.proximity(dhat)
    npt = len(full.pt_pairs)
    assert npt > 512 and len(full.ee_pairs) > 512
    u, x = rf.displacement(mesh.nv, 1, EPS), rf.displacement(mesh.nv, 3, 1.0)
    L = [mesh.friction_lag(p, dhat, KAPPA) for p in (full, _cut(full, n))]
    rec = [_np(l.record) for l in L]
    rows = np.r_[0:n, npt:npt + n]
    assert rec[1].shape == (2 * n, 8) and rec[1].tobytes() == rec[0][rows].tobytes()
    F = [mesh.friction(l, u, MU, EPS) for l in L]
    H = [mesh.friction_hessian_product(l, u, MU, EPS, x) for l in L]
    assert _np(F[1].pt_energy).tobytes() == _np(F[0].pt_energy)[:n].tobytes() and _np(F[1].ee_energy).tobytes() == _np(F[0].ee_energy)[:n].tobytes()
    assert _np(H[1].pair_terms).tobytes() == _np(H[0].pair_terms)[rows].tobytes()
    assert np.abs(_np(H[1].pair_terms)).max() > 0 and float(F[1].energy.item()) > 0


# ------------------------------------------------------------------------------------------------ 4: determinism and inputs
def test_two_calls_give_the_same_bytes_on_large(pol):
    mesh, dhat = _mesh(pol, "large")
    prox = mesh.proximity(dhat)
    u, x = rf.displacement(mesh.nv, 1, EPS), rf.displacement(mesh.nv, 3, 1.0)
    L = [mesh.friction_lag(prox, dhat, KAPPA) for _ in range(2)]
    assert _np(L[0].record).tobytes() == _np(L[1].record).tobytes() and L[0].zero_distance == (0, 0)
    A, B = mesh.friction(L[0], u, MU, EPS), mesh.friction(L[1], u, MU, EPS)
    E = mesh.friction(L[0], u, MU, EPS, gradient=False)
    for k in ("energy", "pt_energy", "ee_energy"):
        a = _np(getattr(A, k)).tobytes()
        assert a == _np(getattr(B, k)).tobytes() and a == _np(getattr(E, k)).tobytes(), k
    assert _np(A.grad).tobytes() == _np(B.grad).tobytes()
    P, Q = (mesh.friction_hessian_product(L[0], u, MU, EPS, x) for _ in range(2))
    assert _np(P.hx).tobytes() == _np(Q.hx).tobytes() and _np(P.pair_terms).tobytes() == _np(Q.pair_terms).tobytes()
    print("FRICTION determinism[large]: %d PT, %d EE pairs, energy %.6e, %d vertices with a gradient" %
          (len(prox.pt_pairs), len(prox.ee_pairs), float(A.energy.item()), (np.abs(_np(A.grad)).max(axis=1) > 0).sum()))
    assert len(prox.pt_pairs) > 1000 and len(prox.ee_pairs) > 1000 and float(A.energy.item()) > 0 and np.abs(_np(P.hx)).max() > 0
    # the barrier calls share the incidence kept on the Proximity
    first = prox._incidence
    mesh.barrier(prox, dhat, KAPPA)
    assert prox._incidence is first


def test_a_side_that_is_none_and_mu_zero(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _, _ = _scene("sheets")
    u, x = rf.displacement(mesh.nv, 1, EPS), rf.displacement(mesh.nv, 3, 1.0)
    full = mesh.friction_lag(mesh.proximity(dhat), dhat, KAPPA)
    Ff = mesh.friction(full, u, MU, EPS)
    only_pt, only_ee = mesh.proximity(dhat, ee=False), mesh.proximity(dhat, pt=False)
    Lp, Le = mesh.friction_lag(only_pt, dhat, KAPPA), mesh.friction_lag(only_ee, dhat, KAPPA)
    npt = len(only_pt.pt_pairs)
    assert _np(Lp.record).tobytes() == _np(full.record)[:npt].tobytes() and _np(Le.record).tobytes() == _np(full.record)[npt:].tobytes()
    P, E = mesh.friction(Lp, u, MU, EPS), mesh.friction(Le, u, MU, EPS)
    assert P.ee_energy is None and E.pt_energy is None and len(P.pt_energy) > 0 and len(E.ee_energy) > 0      # the totals: _check_evaluation
    assert _np(P.pt_energy).tobytes() == _np(Ff.pt_energy).tobytes() and _np(E.ee_energy).tobytes() == _np(Ff.ee_energy).tobytes()
    both = float(P.energy.item()) + float(E.energy.item())
    assert abs(both - float(Ff.energy.item())) <= 1e-14 * both and both > 0
    _check_evaluation("sheets, PT only", pol, mesh, Lp, t, e, u, x)
    _check_evaluation("sheets, EE only", pol, mesh, Le, t, e, u, x)
    # mu = 0: exactly zero everywhere, nothing counted
    Z, ZH = _check_evaluation("sheets, mu = 0", pol, mesh, full, t, e, u, x, mu=0.0)
    assert float(Z.energy.item()) == 0.0 and (_np(Z.pt_energy) == 0).all() and (_np(Z.ee_energy) == 0).all()
    assert (_bits(_np(Z.grad)) == 0).all() and (_bits(_np(ZH.hx)) == 0).all() and (_bits(_np(ZH.pair_terms)) == 0).all()
    assert Z.overflow == (0, 0) and ZH.overflow == (0, 0)


# ------------------------------------------------------------------------------------------------ 5: indices outside the mesh
def _spliced(pairs, bad):
    """pairs with the four rows of bad at positions 0, 255, 256 and last (test_barrier_gpu.py has the reason); returns the list and the
    mask of the rows that came from pairs"""
    n = len(pairs) + 4
    at = [0, 255, 256, n - 1]
    keep = np.ones(n, bool)
    keep[at] = False
    out = np.empty((n, 2), np.int32)
    out[at], out[keep] = bad, pairs
    return out, keep


def test_pairs_with_indices_outside_the_mesh_get_zero_records(pol):
    from zpc_amd.mesh import Proximity
    mesh, dhat = _mesh(pol, "sheets")
    nv, nt, ne = mesh.nv, mesh.nt, mesh.num_edges
    clean = mesh.proximity(dhat)
    assert len(clean.pt_pairs) > 512 and len(clean.ee_pairs) > 512
    pt, kpt = _spliced(_np(clean.pt_pairs), [(-1, 0), (nv, 0), (0, -1), (0, nt)])
    ee, kee = _spliced(_np(clean.ee_pairs), [(-1, 0), (ne, 0), (0, -1), (0, ne)])
    keep = np.concatenate([kpt, kee])
    dirty = Proximity()
    dirty.pt_pairs, dirty.ee_pairs = torch.from_numpy(pt).cuda(), torch.from_numpy(ee).cuda()
    u, x = rf.displacement(nv, 1, EPS), rf.displacement(nv, 3, 1.0)

    def same(what, rows, out):
        c, d = (r.reshape(len(r), -1).view(np.uint32) for r in rows)
        assert len(d) == len(keep) and (d[~keep] == 0).all(), what
        assert np.array_equal(d[keep], c), what
        assert out[1].tobytes() == out[0].tobytes(), what

    L = [mesh.friction_lag(p, dhat, KAPPA) for p in (clean, dirty)]
    assert L[0].zero_distance == L[1].zero_distance == (0, 0)
    same("lag", [_np(l.record) for l in L], [np.zeros(0), np.zeros(0)])      # (the lag step has no per-vertex output)
    F = [mesh.friction(l, u, MU, EPS) for l in L]
    same("energy", [np.concatenate([_np(f.pt_energy), _np(f.ee_energy)]) for f in F], [_np(f.energy) for f in F])
    recs = [_gradient_terms(pol, mesh, l, u) for l in L]
    same("gradient", [r[0] for r in recs], [_np(f.grad) for f in F])
    H = [mesh.friction_hessian_product(l, u, MU, EPS, x) for l in L]
    same("product", [_np(h.pair_terms) for h in H], [_np(h.hx) for h in H])
    # a record that is not zero on a bad row (a caller's own record) is not read through the bad indices either
    forged = L[1]
    forged.record[~torch.from_numpy(keep).cuda()] = 1.0
    G, P = mesh.friction(forged, u, MU, EPS), mesh.friction_hessian_product(forged, u, MU, EPS, x)
    assert _np(G.grad).tobytes() == _np(F[0].grad).tobytes() and _np(P.hx).tobytes() == _np(H[0].hx).tobytes()
    assert (_np(P.pair_terms)[~keep] == 0).all() and G.overflow == (0, 0)
    print("FRICTION indices outside the mesh: %d + 4 PT, %d + 4 EE pairs; the 8 bad rows are zero, every other row, the total, grad and hx are "
          "those of the clean lists" % (len(clean.pt_pairs), len(clean.ee_pairs)))
    assert np.abs(_np(F[0].grad)).max() > 0 and np.abs(_np(H[0].hx)).max() > 0


# ------------------------------------------------------------------------------------------------ 6, 7: against float64, end to end
@functools.lru_cache(maxsize=None)
def _reference(name, scale, xseed, pt_bytes, ee_bytes):
    v, t, e, dhat, rest2 = _scene(name)
    pt, ee = np.frombuffer(pt_bytes, np.int32).reshape(-1, 2), np.frombuffer(ee_bytes, np.int32).reshape(-1, 2)
    u, x = rf.displacement(len(v), 1, scale * EPS), rf.displacement(len(v), xseed, 1.0)
    return rf.Reference(v, t, pt, ee, dhat, KAPPA, u, MU, EPS, x, rest2, e), u, x


def _run(pol, name, scale, xseed):
    mesh, dhat = _mesh(pol, name)
    prox = mesh.proximity(dhat)
    pt, ee = _pairs(prox)
    R, u, x = _reference(name, scale, xseed, pt.tobytes(), ee.tobytes())
    lag = mesh.friction_lag(prox, dhat, KAPPA)
    return R, x, mesh.friction(lag, u, MU, EPS), mesh.friction_hessian_product(lag, u, MU, EPS, x)


@pytest.mark.parametrize("scale", rf.SCALES)
def test_lag_and_evaluation_end_to_end_against_float64_on_sheets(pol, scale):
    R, x, F, H = _run(pol, "sheets", scale, 3)
    g, hx = _np(F.grad).astype(np.float64), _np(H.hx).astype(np.float64)
    rg = _ratio(np.linalg.norm(g - R.grad, axis=1), R.vbound_g)
    rh = _ratio(np.linalg.norm(hx - R.hx, axis=1), R.vbound_h)
    energies = np.concatenate([_np(F.pt_energy), _np(F.ee_energy)]).astype(np.float64)
    re = _ratio(np.abs(energies - np.concatenate([R.pt_e, R.ee_e])), np.concatenate([R.pt_be, R.ee_be]))
    tb = R.energy_bound + 1e-15 * (np.abs(R.pt_e).sum() + np.abs(R.ee_e).sum())
    contact = R.ninc > 0
    with np.errstate(divide="ignore"):
        med = float(np.median(R.vbound_g[contact] / np.linalg.norm(R.grad[contact], axis=1)))
        medh = float(np.median(R.vbound_h[contact] / np.linalg.norm(R.hx[contact], axis=1)))
    print("FRICTION end to end[sheets, u = %g eps_v]: energy %.6e (float64 %.6e); worst pair energy %.3f, vertex gradient %.3f, vertex product "
          "%.3f of the bound; unbounded: %d vertices; bound / |g| median %.3e (the reference's own at eps_v %.3e), bound / |Hx| median %.3e" %
          (scale, float(F.energy.item()), R.energy, re.max(), rg.max(), rh.max(), np.isinf(R.vbound_g).sum(), med, rf.SHEETS_MEDIAN_BOUND_OVER_G,
           medh))
    assert (re <= 1).all() and (rg <= 1).all() and (rh <= 1).all()
    assert np.isinf(tb) or abs(float(F.energy.item()) - R.energy) <= tb
    assert contact.sum() > 200 and (g[~contact] == 0).all()
    if scale == 1.0:
        assert med < 4 * rf.SHEETS_MEDIAN_BOUND_OVER_G


@pytest.mark.parametrize("name", ["sheets", "torus"])
def test_the_invariants_within_the_bounds(pol, name):
    Rx, x, F, Hx = _run(pol, name, 1.0, 3)
    Ry, y, _, Hy = _run(pol, name, 1.0, 4)
    x, y = x.astype(np.float64), y.astype(np.float64)
    hx, hy = _np(Hx.hx).astype(np.float64), _np(Hy.hx).astype(np.float64)
    nx, ny = np.linalg.norm(x, axis=1), np.linalg.norm(y, axis=1)
    yHx, xHy, xHx = (y * hx).sum(), (x * hy).sum(), (x * hx).sum()
    slack = (ny * Rx.vbound_h).sum() + (nx * Ry.vbound_h).sum()
    net = np.linalg.norm(_np(F.grad).astype(np.float64).sum(axis=0))
    print("FRICTION invariants[%s]: y^T H x %.6e, x^T H y %.6e (difference %.2e, bounds %.2e), x^T H x %.6e (bounds %.2e); |sum g| %.3e, sum of "
          "the vertex bounds %.3e, sum |g| %.3e" % (name, yHx, xHy, abs(yHx - xHy), slack, xHx, (nx * Rx.vbound_h).sum(), net, Rx.vbound_g.sum(),
                                                   np.linalg.norm(_np(F.grad), axis=1).sum()))
    assert abs(yHx - xHy) <= slack
    assert xHx >= -(nx * Rx.vbound_h).sum() and xHx > 0
    assert net <= Rx.vbound_g.sum()


# ------------------------------------------------------------------------------------------------ 8: arguments
def test_arguments(pol):
    from zpc_amd import lib
    from zpc_amd.mesh import TriMesh
    v, t, _, dhat, _ = _scene("sheets")
    mesh = TriMesh(pol, v, t)
    prox = mesh.proximity(dhat)
    nv = mesh.nv
    u, x = rf.displacement(nv, 1, EPS), rf.displacement(nv, 3, 1.0)
    with pytest.raises(ValueError):
        mesh.friction_lag(prox, dhat, KAPPA)                      # mollify=True before set_rest
    plain = mesh.friction_lag(prox, dhat, KAPPA, mollify=False)   # ... which the unmollified contact force does not need
    mesh.set_rest()
    lag = mesh.friction_lag(prox, dhat, KAPPA)
    npt = len(prox.pt_pairs)
    # lambda of a PT pair does not depend on the mollifier, lambda of an EE pair is at most the unmollified one (m <= 1)
    assert _np(plain.record)[:npt].tobytes() == _np(lag.record)[:npt].tobytes() and (_np(plain.lam)[npt:] >= _np(lag.lam)[npt:]).all()
    for bad in (0.0, -0.01, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError):
            mesh.friction_lag(prox, bad, KAPPA)
        with pytest.raises(ValueError):
            mesh.friction_lag(prox, dhat, bad)
        with pytest.raises(ValueError):
            mesh.friction(lag, u, MU, bad)
        with pytest.raises(ValueError):
            mesh.friction_hessian_product(lag, u, MU, bad, x)
    for bad in (-0.1, float("inf"), float("nan"), 1e60):
        with pytest.raises(ValueError):
            mesh.friction(lag, u, bad, EPS)
        with pytest.raises(ValueError):
            mesh.friction_hessian_product(lag, u, bad, EPS, x)
    for call in (lambda: mesh.friction_lag(prox, dhat, KAPPA, verts=v[:-1]), lambda: mesh.friction_lag(None, dhat, KAPPA),
                 lambda: mesh.friction(prox, u, MU, EPS), lambda: mesh.friction(lag, u[:-1], MU, EPS),
                 lambda: mesh.friction_hessian_product(None, u, MU, EPS, x), lambda: mesh.friction_hessian_product(lag, u[:-1], MU, EPS, x),
                 lambda: mesh.friction_hessian_product(lag, u, MU, EPS, x[:-1])):
        with pytest.raises(ValueError):
            call()
    stale = mesh.friction_lag(mesh.proximity(dhat), dhat, KAPPA)
    stale.prox.pt_pairs = stale.prox.pt_pairs[:-1]
    with pytest.raises(ValueError):
        mesh.friction(stale, u, MU, EPS)
    # the C entries: -1 and nothing written
    L = lib()
    nee = len(prox.ee_pairs)
    F = mesh.friction(lag, u, MU, EPS)
    starts, entries, nscratch = prox._incidence
    scratch = torch.full((nscratch,), 7.0, dtype=torch.float32, device="cuda")
    total = torch.full((), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((nv, 3), 7.0, dtype=torch.float32, device="cuda")
    record = torch.full((npt + nee, 8), 7.0, dtype=torch.float32, device="cuda")
    ud, xd = torch.from_numpy(u).cuda(), torch.from_numpy(x).cuda()
    ptp, eep = prox.pt_pairs.data_ptr(), prox.ee_pairs.data_ptr()
    fresh = TriMesh(pol, v, t)
    big = 1 << 28

    def c_lag(m=mesh.handle, d=dhat, k=KAPPA, mol=1, rec=record.data_ptr(), n=npt, p=pol.handle):
        return L.zs_rocm_mesh_friction_lag(p, m, None, ptp, n, eep, nee, d, k, mol, rec, None)

    def c_energy(m=mesh.handle, uu=ud.data_ptr(), rec=lag.record.data_ptr(), mu=MU, ev=EPS, n=npt, p=pol.handle):
        return L.zs_rocm_mesh_friction_energy(p, m, uu, ptp, n, eep, nee, rec, mu, ev, None, None, total.data_ptr(), None)

    def c_gradient(m=mesh.handle, uu=ud.data_ptr(), rec=lag.record.data_ptr(), mu=MU, ev=EPS, n=npt, p=pol.handle, g=out.data_ptr(),
                   st=starts.data_ptr()):
        return L.zs_rocm_mesh_friction_gradient(p, m, uu, ptp, n, eep, nee, rec, mu, ev, st, entries.data_ptr(), scratch.data_ptr(), None, None,
                                                total.data_ptr(), g, None)

    def c_product(m=mesh.handle, uu=ud.data_ptr(), rec=lag.record.data_ptr(), mu=MU, ev=EPS, n=npt, p=pol.handle, xx=xd.data_ptr(),
                  h=out.data_ptr()):
        return L.zs_rocm_mesh_friction_hessian_product(p, m, uu, xx, ptp, n, eep, nee, rec, mu, ev, starts.data_ptr(), entries.data_ptr(),
                                                       scratch.data_ptr(), h, None)
    assert c_lag(m=None) == -1 and c_lag(p=None) == -1 and c_lag(rec=None) == -1 and c_lag(n=big) == -1 and c_lag(m=fresh.handle) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert c_lag(d=bad) == -1 and c_lag(k=bad) == -1
    for fn in (c_energy, c_gradient, c_product):
        assert fn(m=None) == -1 and fn(p=None) == -1 and fn(uu=None) == -1 and fn(rec=None) == -1 and fn(n=big) == -1
        for bad in (-1.0, float("inf"), float("nan")):
            assert fn(mu=bad) == -1
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(ev=bad) == -1
    assert c_gradient(g=None) == -1 and c_gradient(st=None) == -1 and c_product(xx=None) == -1 and c_product(h=None) == -1
    pol.syncCtx()
    assert float(total.item()) == 7.0 and (out == 7).all() and (record == 7).all() and (scratch == 7).all()
    # ... and the same closures with good arguments run
    assert c_lag() == 0 and c_energy() == 0 and c_gradient() == 0
    pol.syncCtx()
    assert record.cpu().numpy().tobytes() == _np(lag.record).tobytes() and _np(out).tobytes() == _np(F.grad).tobytes()
    assert float(total.item()) == float(F.energy.item())
    assert c_product() == 0
    pol.syncCtx()
    assert _np(out).tobytes() == _np(mesh.friction_hessian_product(lag, u, MU, EPS, x).hx).tobytes()
