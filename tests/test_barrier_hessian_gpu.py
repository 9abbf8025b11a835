"""Mesh barrier Hessian-vector product on the GPU (zpc_amd/csrc/mesh_barrier.hip, TriMesh.barrier_hessian_product) against the float64
reference and the derived bounds of tests/ref64_barrier_hessian.py: the per-pair terms by the candidate rule and the per-vertex product
on every scene of ref64_proximity.SCENES, mollified and not, exact and psd; the gather replayed bit for bit; determinism on `large`; the
exact algebra of a linear operator; the invariants on the device output; trial positions; a pair at zero distance; the argument checks.
No pair and no vertex is left out of a comparison: where a bound is infinite the line printed says how many.  Prints one
`HESSIAN <what> ...` line per check.

Measured on an MI355X: worst pair 0.070 of its bound (stack, PT, psd), worst vertex 0.020 (stack); 4 pairs and 16 vertices of `stack` have
an infinite bound, and so have all 288 contact vertices of `torus` and 132 of 162 of `regular` (nearly parallel edges: the
two-parameter candidate of ref64_barrier_hessian.ee_candidates64); most incidences at one vertex 821 (fan); the file runs in 4.4 s."""
import functools

import numpy as np
import pytest

import ref64_barrier as rb
import ref64_barrier_hessian as rh
import ref64_proximity as rp
import ref64_terms as rt

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
KAPPA = 1.0


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


def _bytes(x):
    return _np(x).tobytes()


def _compare(what, P, R, nv, npt):
    """the checks of one BarrierHessianProduct against one Reference; returns the per-vertex ratio"""
    terms, hx = _np(P.pair_terms), _np(P.hx)
    assert terms.dtype == np.float32 and terms.shape == (len(R.pair_terms), 4, 3) and np.isfinite(terms).all()
    worst, unbounded, weak = {}, 0, 0
    for k, got, q in (("pt", terms[:npt], R.pt), ("ee", terms[npt:], R.ee)):
        ratio, unb = rh.pair_ratio(got, q)
        worst[k] = ratio.max() if len(ratio) else 0.0
        unbounded += int(unb.sum())
        weak += int(rh.some_unbounded(q).sum())
        assert (ratio <= 1).all(), (what, k, worst[k])
    assert hx.shape == (nv, 3) and hx.dtype == np.float32 and np.isfinite(hx).all()
    err = np.linalg.norm(hx.astype(np.float64) - R.hx, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rv = np.where((err == 0) | np.isinf(R.vbound), 0.0, err / R.vbound)
    assert (hx[R.ninc == 0] == 0).all()
    print("HESSIAN %s: %d PT, %d EE pairs; worst pair %.3f / %.3f, worst vertex %.3f of the bound; most incidences at one vertex %d; unbounded: "
          "%d pairs (%d with an unbounded candidate), %d vertices" % (what, npt, len(terms) - npt, worst["pt"], worst["ee"], rv.max() if len(rv) else 0.0,
                                                                      R.ninc.max() if nv else 0, unbounded, weak, np.isinf(R.vbound).sum()))
    assert (rv <= 1).all(), what
    return rv


# ------------------------------------------------------------------------------------------------ 1: against the float64 reference
# unmollified without `regular`, as for the gradient: between its exactly parallel edges only the mollified potential is defined
@pytest.mark.parametrize("psd", [False, True])
@pytest.mark.parametrize("name,mollify", [(n, True) for n in rp.SCENES] + [(n, False) for n in rp.SCENES if n != "regular"])
def test_pair_terms_and_product_against_the_float64_reference(pol, name, mollify, psd):
    mesh, dhat = _mesh(pol, name)
    v, t, e, _, rest2 = _scene(name)
    prox = mesh.proximity(dhat)
    x = rh.direction(len(v), 1)
    P = mesh.barrier_hessian_product(prox, dhat, KAPPA, x, mollify=mollify, psd=psd)
    R = rh.Reference(v, t, _np(prox.pt_pairs), _np(prox.ee_pairs), dhat, KAPPA, x, rest2 if mollify else None, e, psd=psd)
    _compare("%s (mollify %s, psd %s)" % (name, mollify, psd), P, R, len(v), len(prox.pt_pairs))
    assert P.zero_distance == (0, 0) and R.zero == (0, 0)
    if name == "tiny0":
        assert (_np(P.hx).view(np.uint32) == 0).all() and P.pair_terms.shape == (0, 4, 3)
    if name == "tiny1":
        assert len(prox.ee_pairs) == 0 and len(prox.pt_pairs) > 0 and len(P.pair_terms) == len(prox.pt_pairs)
    if name in ("fan", "stack"):      # runs longer than a wave
        assert R.ninc.max() > 64
    if name == "regular":
        assert (R.ee["m"] == 0).sum() > 0
    if name in ("sheets", "regular", "torus", "fan", "stack"):
        assert np.abs(_np(P.hx)).max() > 0
    if name == "sheets" and mollify and not psd:
        contact = R.ninc > 0
        med = float(np.median(R.vbound[contact] / np.linalg.norm(R.hx[contact], axis=1)))
        print("HESSIAN vacuity[sheets]: bound / |Hx| median %.3e, the reference's own %.3e" % (med, rh.SHEETS_MEDIAN_BOUND_OVER_HX))
        assert med < 4 * rh.SHEETS_MEDIAN_BOUND_OVER_HX


# ------------------------------------------------------------------------------------------------ 2: the gather, exactly
@pytest.mark.parametrize("name", ["fan", "sheets"])
def test_the_product_is_the_front_to_back_float32_sum_of_the_pair_terms(pol, name):
    mesh, dhat = _mesh(pol, name)
    prox = mesh.proximity(dhat)
    P = mesh.barrier_hessian_product(prox, dhat, KAPPA, rh.direction(mesh.nv, 1))
    starts, entries = (_np(z).astype(np.int64) for z in prox._incidence[:2])
    run = np.diff(starts)
    s = rt.gather(mesh.nv, [(starts, entries, _np(P.pair_terms).reshape(-1, 3))], np.float32)
    print("HESSIAN gather[%s]: %d vertices, longest run %d" % (name, mesh.nv, run.max()))
    assert starts[-1] == 4 * len(P.pair_terms) and run.max() > (64 if name == "fan" else 1)
    assert _bytes(P.hx) == s.tobytes()


# ------------------------------------------------------------------------------------------------ 3: determinism
def test_two_calls_give_the_same_bytes_on_large(pol):
    mesh, dhat = _mesh(pol, "large")
    prox = mesh.proximity(dhat)
    x = rh.direction(mesh.nv, 1)
    grad = _bytes(mesh.barrier(prox, dhat, KAPPA).grad)
    for psd in (False, True):
        A, B = (mesh.barrier_hessian_product(prox, dhat, KAPPA, x, psd=psd) for _ in range(2))
        assert _bytes(A.hx) == _bytes(B.hx) and _bytes(A.pair_terms) == _bytes(B.pair_terms)
        prox._incidence = None
        C = mesh.barrier_hessian_product(prox, dhat, KAPPA, x, psd=psd)
        assert _bytes(C.hx) == _bytes(A.hx) and _bytes(C.pair_terms) == _bytes(A.pair_terms)
        assert _bytes(mesh.barrier(prox, dhat, KAPPA).grad) == grad
    print("HESSIAN determinism[large]: %d PT, %d EE pairs, %d vertices with a product" %
          (len(prox.pt_pairs), len(prox.ee_pairs), (np.abs(_np(A.hx)).max(axis=1) > 0).sum()))
    assert len(prox.pt_pairs) > 1000 and len(prox.ee_pairs) > 1000 and np.abs(_np(A.hx)).max() > 0 and A.zero_distance == (0, 0)


# ------------------------------------------------------------------------------------------------ 4: exact algebra
@pytest.mark.parametrize("psd", [False, True])
def test_the_product_is_exactly_homogeneous(pol, psd):
    mesh, dhat = _mesh(pol, "sheets")
    prox = mesh.proximity(dhat)
    x = rh.direction(mesh.nv, 1)
    H = lambda z: mesh.barrier_hessian_product(prox, dhat, KAPPA, z, psd=psd)
    one, two, neg, nil = H(x), H(np.float32(2) * x), H(-x), H(np.zeros_like(x))
    assert (_np(nil.hx).view(np.uint32) & 0x7fffffff == 0).all() and (_np(nil.pair_terms).view(np.uint32) & 0x7fffffff == 0).all()
    assert np.abs(_np(one.hx)).max() > 0
    for k in ("hx", "pair_terms"):        # scaling by 2 and by -1 is exact in every operation of a chain that is linear in x
        assert (np.float32(2) * _np(getattr(one, k))).tobytes() == _bytes(getattr(two, k)), k
        assert np.array_equal(-_np(getattr(one, k)), _np(getattr(neg, k))), k
        assert ((-_np(getattr(one, k))).view(np.uint32) << 1 == _np(getattr(neg, k)).view(np.uint32) << 1).all(), k


# ------------------------------------------------------------------------------------------------ 5: invariants on the device output
# (scenes whose vertex bounds are all finite: between the nearly parallel edges of `torus` and `regular` the two-parameter candidate is unbounded)
@pytest.mark.parametrize("name", ["sheets", "fan"])
def test_the_invariants_hold_within_the_vertex_bounds(pol, name):
    mesh, dhat = _mesh(pol, name)
    v, t, e, _, rest2 = _scene(name)
    prox = mesh.proximity(dhat)
    pt, ee = _np(prox.pt_pairs), _np(prox.ee_pairs)
    x, y = rh.direction(len(v), 1), rh.direction(len(v), 2)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    an = lambda z: np.linalg.norm(z, axis=1)
    dev = lambda z, **kw: _np(mesh.barrier_hessian_product(prox, dhat, KAPPA, z, **kw).hx).astype(np.float64)
    ref = lambda z, mollify=True, psd=False: rh.Reference(v, t, pt, ee, dhat, KAPPA, z, rest2 if mollify else None, e, psd=psd)
    for psd in (False, True):
        hx, hy, Rx, Ry = dev(x, psd=psd), dev(y, psd=psd), ref(x, psd=psd), ref(y, psd=psd)
        yx, xy = (y64 * hx).sum(), (x64 * hy).sum()
        slack = (Rx.vbound * an(y64)).sum() + (Ry.vbound * an(x64)).sum()
        print("HESSIAN symmetry[%s, psd %s]: y^T H x %.6e, x^T H y %.6e, difference %.2e, bound %.2e" % (name, psd, yx, xy, abs(yx - xy), slack))
        assert np.isfinite(slack) and abs(yx - xy) <= slack
        if psd:
            assert (x64 * hx).sum() >= -(Rx.vbound * an(x64)).sum()
    shift = np.broadcast_to(np.array([0.3, -1.1, 0.7], np.float32), x.shape).copy()
    ht, Rt = dev(shift), ref(shift)
    assert (an(ht) <= an(Rt.hx) + Rt.vbound).all() and an(Rt.hx).max() <= 1e-9 * an(ref(x).hx).max()
    plus, exact, Rp, Re = dev(x, mollify=False, psd=True), dev(x, mollify=False), ref(x, False, True), ref(x, False, False)
    assert (x64 * plus).sum() - (x64 * exact).sum() >= -((Rp.vbound + Re.vbound) * an(x64)).sum()
    assert (x64 * plus).sum() > (x64 * exact).sum()


# ------------------------------------------------------------------------------------------------ 6: trial positions
def test_trial_positions_equal_a_second_mesh_at_those_positions(pol):
    from zpc_amd.mesh import TriMesh, Proximity
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _, rest2 = _scene("sheets")
    prox = mesh.proximity(dhat)
    moved = (v + 2e-3 * (np.random.default_rng(7).random(v.shape) - 0.5)).astype(np.float32)
    x = rh.direction(len(v), 1)
    other = TriMesh(pol, moved, t)
    other.set_rest(v)
    lists = Proximity()
    lists.pt_pairs, lists.ee_pairs = prox.pt_pairs, prox.ee_pairs
    for psd in (False, True):
        A = mesh.barrier_hessian_product(prox, dhat, KAPPA, x, verts=moved, psd=psd)
        B = other.barrier_hessian_product(lists, dhat, KAPPA, x, psd=psd)
        assert _bytes(A.hx) == _bytes(B.hx) and _bytes(A.pair_terms) == _bytes(B.pair_terms)
        assert _bytes(A.hx) != _bytes(mesh.barrier_hessian_product(prox, dhat, KAPPA, x, psd=psd).hx)
    R = rh.Reference(moved, t, _np(prox.pt_pairs), _np(prox.ee_pairs), dhat, KAPPA, x, rest2, e, psd=True)
    _compare("sheets, trial positions (psd)", A, R, len(v), len(prox.pt_pairs))


# ------------------------------------------------------------------------------------------------ 7: zero distance
def test_a_pair_at_zero_distance_is_counted_and_adds_nothing(pol):
    from zpc_amd.mesh import TriMesh
    v = np.array([[0.3, 0.3, 0.5], [0.5, 0.3, 0.5], [0.3, 0.5, 0.5], [0.35, 0.35, 0.5], [0.45, 0.4, 0.56], [0.4, 0.45, 0.56]], np.float32)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    prox = mesh.proximity(0.05)
    pairs = _np(prox.pt_pairs).tolist()
    assert [3, 0] in pairs
    x = rh.direction(len(v), 1)
    for mollify in (True, False):
        for psd in (False, True):
            P = mesh.barrier_hessian_product(prox, 0.05, KAPPA, x, mollify=mollify, psd=psd)
            assert P.zero_distance == (1, 0)
            assert (_np(P.pair_terms)[pairs.index([3, 0])].view(np.uint32) == 0).all() and np.abs(_np(P.pair_terms)).max() > 0
            R = rh.Reference(v, t, _np(prox.pt_pairs), _np(prox.ee_pairs), 0.05, KAPPA, x, rb.rest_len2(v, rp.edges(t)) if mollify else None, psd=psd)
            assert R.zero == (1, 0)
            _compare("zero distance (mollify %s, psd %s)" % (mollify, psd), P, R, len(v), len(pairs))


# ------------------------------------------------------------------------------------------------ 8: arguments
def test_arguments(pol):
    from zpc_amd import lib
    from zpc_amd.mesh import TriMesh
    v, t, _, dhat, _ = _scene("sheets")
    mesh = TriMesh(pol, v, t)
    prox = mesh.proximity(dhat)
    x = rh.direction(len(v), 1)
    with pytest.raises(ValueError):
        mesh.barrier_hessian_product(prox, dhat, KAPPA, x)                      # mollify=True before set_rest
    plain = mesh.barrier_hessian_product(prox, dhat, KAPPA, x, mollify=False)   # ... which the unmollified product does not need
    mesh.set_rest()
    for bad in (0.0, -0.01, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError):
            mesh.barrier_hessian_product(prox, bad, KAPPA, x)
        with pytest.raises(ValueError):
            mesh.barrier_hessian_product(prox, dhat, bad, x)
    for bad in (x[:-1], x[:, :2], np.zeros(3, np.float32)):
        with pytest.raises(ValueError):
            mesh.barrier_hessian_product(prox, dhat, KAPPA, bad)
    with pytest.raises(ValueError):
        mesh.barrier_hessian_product(prox, dhat, KAPPA, x, verts=v[:-1])
    with pytest.raises(ValueError):
        mesh.barrier_hessian_product(None, dhat, KAPPA, x)
    # the C entry: -1 and nothing written
    L = lib()
    npt, nee = len(prox.pt_pairs), len(prox.ee_pairs)
    starts, entries, nscratch = prox._incidence
    scratch = torch.empty(nscratch, dtype=torch.float32, device="cuda")
    hx = torch.full((mesh.nv, 3), 7.0, dtype=torch.float32, device="cuda")
    xd = torch.from_numpy(x).cuda()
    fresh = TriMesh(pol, v, t)

    def call(m, d, k, mol, xp=xd.data_ptr(), hp=hx.data_ptr()):
        return L.zs_rocm_mesh_barrier_hessian_product(pol.handle, m, None, prox.pt_pairs.data_ptr(), npt, prox.ee_pairs.data_ptr(), nee, d, k, mol, 0,
                                                      xp, starts.data_ptr(), entries.data_ptr(), scratch.data_ptr(), hp, None)
    assert call(None, dhat, KAPPA, 0) == -1 and call(fresh.handle, dhat, KAPPA, 1) == -1
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(mesh.handle, bad, KAPPA, 1) == -1 and call(mesh.handle, dhat, bad, 1) == -1
    assert call(mesh.handle, dhat, KAPPA, 1, xp=None) == -1 and call(mesh.handle, dhat, KAPPA, 1, hp=None) == -1
    pol.syncCtx()
    assert (hx == 7).all()
    assert call(mesh.handle, dhat, KAPPA, 1) == 0
    pol.syncCtx()
    assert _bytes(hx) == _bytes(mesh.barrier_hessian_product(prox, dhat, KAPPA, x).hx)
    # a Proximity with one side None: that side is skipped, and the two sides add up (per pair exactly)
    full = mesh.barrier_hessian_product(prox, dhat, KAPPA, x)
    only_pt, only_ee = mesh.proximity(dhat, ee=False), mesh.proximity(dhat, pt=False)
    A, B = mesh.barrier_hessian_product(only_pt, dhat, KAPPA, x), mesh.barrier_hessian_product(only_ee, dhat, KAPPA, x)
    assert _bytes(A.pair_terms) == _np(full.pair_terms)[:npt].tobytes() and _bytes(B.pair_terms) == _np(full.pair_terms)[npt:].tobytes()
    assert _np(plain.pair_terms)[:npt].tobytes() == _np(full.pair_terms)[:npt].tobytes()      # PT pairs do not depend on the mollifier
