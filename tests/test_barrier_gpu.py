"""Mesh barrier potential on the GPU (zpc_amd/csrc/mesh_barrier.hip, TriMesh.set_rest / TriMesh.barrier) against the float64 reference and
the derived bounds of tests/ref64_barrier.py: energies per pair, the float64 total and the gradient per vertex on every scene of
ref64_proximity.SCENES, mollified and not; runs of more than 64 incidences; determinism on `large`; trial positions; a pair at zero
distance; the invariants; the argument checks; lists with indices outside the mesh.  The constraint sets are the lists TriMesh.proximity
returns; the reference evaluates the same lists.  No pair and no vertex is left out of a comparison: where a bound is infinite (an interval
of distances that reaches zero) the line printed says how many.  Prints one `BARRIER <what> ...` line per check.

Measured on an MI355X: worst vertex gradient 0.012 of its bound mollified (stack) and 0.34 unmollified (torus), worst pair energy 0.044
(torus, EE); 4 pairs and 16 vertices of `stack` have an infinite bound; most incidences at one vertex 821 (fan); the file runs in 2.7 s."""
import functools

import numpy as np
import pytest

import ref64_barrier as rb
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


def _total_is_the_replay(B):
    """the float64 total of a Barrier is the reduction of tests/ref64_terms.py over its float32 energies, PT then EE, bit for bit"""
    own = [a for a in (_np(B.pt_energy), _np(B.ee_energy)) if a is not None]
    assert _np(B.energy).tobytes() == np.float64(rt.total(np.concatenate(own))).tobytes()


def _compare(what, B, R, nv):
    """the checks of one Barrier against one Reference; returns the per-vertex ratio"""
    pe, ee, g = _np(B.pt_energy), _np(B.ee_energy), _np(B.grad)
    worst = {}
    for k, got, want, bound in (("pt", pe, R.pt_e, R.pt_be), ("ee", ee, R.ee_e, R.ee_be)):
        assert got.dtype == np.float32 and got.shape == want.shape
        err = np.where(got.astype(np.float64) == want, 0.0, np.abs(got.astype(np.float64) - want))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where((err == 0) | np.isinf(bound), 0.0, err / bound)
        worst[k] = r.max() if len(r) else 0.0
        assert (r <= 1).all(), (what, k)
    total = float(B.energy.item())
    assert B.energy.dtype == torch.float64
    # the float64 sum of the float32 energies: their bounds, and the rounding of the sum itself
    tb = R.energy_bound + 1e-15 * (np.abs(R.pt_e).sum() + np.abs(R.ee_e).sum())
    assert np.isinf(tb) or abs(total - R.energy) <= tb, (what, total, R.energy, tb)
    own = float(pe.astype(np.float64).sum() + ee.astype(np.float64).sum())      # the total is the sum of the energies it returns
    assert total == own or abs(total - own) <= 1e-13 * own
    _total_is_the_replay(B)
    assert g.shape == (nv, 3) and g.dtype == np.float32 and np.isfinite(g).all()
    err = np.linalg.norm(g.astype(np.float64) - R.grad, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rv = np.where((err == 0) | np.isinf(R.vbound), 0.0, err / R.vbound)
    assert (g[R.ninc == 0] == 0).all()
    print("BARRIER %s: %d PT, %d EE pairs, energy %.6e (float64 %.6e); worst pair energy %.3f / %.3f, worst vertex gradient %.3f of the bound; "
          "most incidences at one vertex %d; unbounded: %d pairs, %d vertices" %
          (what, len(pe), len(ee), total, R.energy, worst["pt"], worst["ee"], rv.max() if len(rv) else 0.0, R.ninc.max() if nv else 0,
           np.isinf(R.pt_be).sum() + np.isinf(R.ee_be).sum(), np.isinf(R.vbound).sum()))
    assert (rv <= 1).all(), what
    return rv


# ------------------------------------------------------------------------------------------------ 1: against the float64 reference
# unmollified without `regular`: between its exactly parallel edges the gradient of d2 is set-valued, only the mollified potential defines it
@pytest.mark.parametrize("name,mollify", [(n, True) for n in rp.SCENES] + [(n, False) for n in rp.SCENES if n != "regular"])
def test_energy_and_gradient_against_the_float64_reference(pol, name, mollify):
    mesh, dhat = _mesh(pol, name)
    v, t, e, _, rest2 = _scene(name)
    prox = mesh.proximity(dhat)
    B = mesh.barrier(prox, dhat, KAPPA, mollify=mollify)
    R = rb.Reference(v, t, _np(prox.pt_pairs), _np(prox.ee_pairs), dhat, KAPPA, rest2 if mollify else None, e)
    _compare("%s (mollify %s)" % (name, mollify), B, R, len(v))
    assert B.zero_distance == (0, 0) and R.zero == (0, 0)
    if name == "tiny0":
        assert float(B.energy.item()) == 0.0 and (_np(B.grad) == 0).all() and len(B.pt_energy) == 0 and len(B.ee_energy) == 0
    if name == "tiny1":
        assert len(B.ee_energy) == 0 and len(B.pt_energy) > 0
    if name in ("fan", "stack"):      # runs longer than a wave, and runs that cross wave boundaries of the sorted incidence
        assert R.ninc.max() > 64
    if name == "stack":
        assert np.sort(R.ninc)[len(R.ninc) // 2] > 64
        # the total's two arrays meet inside a chunk of 4096, off a multiple of 256
        assert len(B.pt_energy) + len(B.ee_energy) > 4096 and len(B.pt_energy) % 256 != 0 and len(B.pt_energy) % 4096 != 0
    if name in ("sheets", "regular", "torus", "fan", "stack"):
        assert float(B.energy.item()) > 0 and np.abs(_np(B.grad)).max() > 0
    if name == "sheets" and mollify:
        contact = R.ninc > 0
        med = float(np.median(R.vbound[contact] / np.linalg.norm(R.grad[contact], axis=1)))
        print("BARRIER vacuity[sheets]: bound / |g| median %.3e, the reference's own %.3e" % (med, rb.SHEETS_MEDIAN_BOUND_OVER_G))
        assert med < 4 * rb.SHEETS_MEDIAN_BOUND_OVER_G


def test_rest_lengths_and_the_mollified_pairs_of_regular(pol):
    mesh, dhat = _mesh(pol, "regular")
    v, t, e, _, rest2 = _scene("regular")
    got = _np(mesh.rest()).astype(np.float64)
    assert (np.abs(got - rest2) <= 6 * rb.U * rest2).all()      # differences 1, squares 1 (+ 2), their sum 2 roundings
    moved = v * np.float32(1.5)
    mesh.set_rest(moved)
    assert (np.abs(_np(mesh.rest()).astype(np.float64) - rb.rest_len2(moved, e)) <= 6 * rb.U * rb.rest_len2(moved, e)).all()


# ------------------------------------------------------------------------------------------------ 2: determinism
def test_two_calls_give_the_same_bytes_on_large(pol):
    mesh, dhat = _mesh(pol, "large")
    prox = mesh.proximity(dhat)
    A, B = mesh.barrier(prox, dhat, KAPPA), mesh.barrier(prox, dhat, KAPPA)
    E = mesh.barrier(prox, dhat, KAPPA, gradient=False)
    assert E.grad is None
    for k in ("energy", "pt_energy", "ee_energy"):
        a = _np(getattr(A, k)).tobytes()
        assert a == _np(getattr(B, k)).tobytes() and a == _np(getattr(E, k)).tobytes(), k
    assert _np(A.grad).tobytes() == _np(B.grad).tobytes()
    first = [x.cpu().numpy().tobytes() for x in prox._incidence[:2]]
    prox._incidence = None
    C = mesh.barrier(prox, dhat, KAPPA)
    assert [x.cpu().numpy().tobytes() for x in prox._incidence[:2]] == first
    assert _np(C.grad).tobytes() == _np(A.grad).tobytes()
    g = _np(A.grad)
    print("BARRIER determinism[large]: %d PT, %d EE pairs, energy %.6e, %d vertices with a gradient" %
          (len(prox.pt_pairs), len(prox.ee_pairs), float(A.energy.item()), (np.abs(g).max(axis=1) > 0).sum()))
    assert len(prox.pt_pairs) > 1000 and len(prox.ee_pairs) > 1000 and float(A.energy.item()) > 0 and A.zero_distance == (0, 0)
    # the order of a vertex's run is the list's: the incidence entries of every vertex ascend
    starts, entries = (x.cpu().numpy() for x in prox._incidence[:2])
    assert starts[0] == 0 and starts[-1] == 4 * (len(prox.pt_pairs) + len(prox.ee_pairs)) and (np.diff(starts) >= 0).all()
    inside = np.ones(len(entries), bool)
    inside[starts[1:-1][starts[1:-1] < len(entries)]] = False
    assert (np.diff(entries)[inside[1:]] > 0).all()


# ------------------------------------------------------------------------------------------------ 3: trial positions
def test_trial_positions_are_evaluated_on_the_list_of_the_unmoved_mesh(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, e, _, rest2 = _scene("sheets")
    prox = mesh.proximity(dhat)
    before = [_np(prox.pt_pairs).copy(), _np(prox.ee_pairs).copy()]
    moved = (v + 2e-3 * (np.random.default_rng(7).random(v.shape) - 0.5)).astype(np.float32)
    B = mesh.barrier(prox, dhat, KAPPA, verts=moved)
    R = rb.Reference(moved, t, before[0], before[1], dhat, KAPPA, rest2, e)
    _compare("sheets, trial positions", B, R, len(v))
    own = mesh.barrier(prox, dhat, KAPPA)
    assert _np(own.grad).tobytes() != _np(B.grad).tobytes()
    assert np.array_equal(_np(prox.pt_pairs), before[0]) and np.array_equal(_np(prox.ee_pairs), before[1])
    assert np.array_equal(_np(mesh.proximity(dhat).pt_pairs), before[0])      # the mesh itself has not moved


def test_sheets_pulled_apart_beyond_dhat_give_exactly_zero(pol):
    mesh, dhat = _mesh(pol, "regular")      # no pairs inside a sheet: its grid spacing is 2.5 dHat
    v = _scene("regular")[0]
    prox = mesh.proximity(dhat)
    assert float(mesh.barrier(prox, dhat, KAPPA).energy.item()) > 0
    apart = v.copy()
    apart[len(v) // 2:, 2] += np.float32(0.02)      # the gap grows from 0.02 to 0.04 > dHat = 0.03
    for gradient in (True, False):
        B = mesh.barrier(prox, dhat, KAPPA, verts=apart, gradient=gradient)
        assert float(B.energy.item()) == 0.0 and (_np(B.pt_energy) == 0).all() and (_np(B.ee_energy) == 0).all()
        assert B.zero_distance == (0, 0)
    B = mesh.barrier(prox, dhat, KAPPA, verts=torch.from_numpy(apart).cuda())
    assert (_np(B.grad).view(np.uint32) & 0x7fffffff == 0).all()


# ------------------------------------------------------------------------------------------------ 4: zero distance
def test_a_vertex_in_the_plane_of_a_triangle_is_counted_and_adds_no_gradient(pol):
    from zpc_amd.mesh import TriMesh
    v = np.array([[0.3, 0.3, 0.5], [0.5, 0.3, 0.5], [0.3, 0.5, 0.5], [0.35, 0.35, 0.5], [0.45, 0.4, 0.56], [0.4, 0.45, 0.56]], np.float32)
    t = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    prox = mesh.proximity(0.05)
    assert [3, 0] in _np(prox.pt_pairs).tolist()
    for mollify in (True, False):
        B = mesh.barrier(prox, 0.05, KAPPA, mollify=mollify)
        assert B.zero_distance == (1, 0)
        assert float(B.energy.item()) == float("inf") and np.isinf(_np(B.pt_energy)).sum() == 1 and np.isfinite(_np(B.ee_energy)).all()
        g = _np(B.grad)
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        R = rb.Reference(v, t, _np(prox.pt_pairs), _np(prox.ee_pairs), 0.05, KAPPA, rb.rest_len2(v, rp.edges(t)) if mollify else None)
        assert R.zero == (1, 0)
        err = np.linalg.norm(g.astype(np.float64) - R.grad, axis=1)
        print("BARRIER zero distance (mollify %s): %d PT, %d EE pairs, gradient %.3f of the bound" % (mollify, len(prox.pt_pairs), len(prox.ee_pairs),
                                                                                                   (err / R.vbound).max()))
        assert (err <= R.vbound).all()
        E = mesh.barrier(prox, 0.05, KAPPA, mollify=mollify, gradient=False)
        assert E.zero_distance == (1, 0) and float(E.energy.item()) == float("inf")


# ------------------------------------------------------------------------------------------------ 5: invariants
@pytest.mark.parametrize("name", ["sheets", "torus"])
def test_the_gradient_sums_to_zero_within_the_bounds(pol, name):
    mesh, dhat = _mesh(pol, name)
    v, t, e, _, rest2 = _scene(name)
    prox = mesh.proximity(dhat)
    B = mesh.barrier(prox, dhat, KAPPA)
    R = rb.Reference(v, t, _np(prox.pt_pairs), _np(prox.ee_pairs), dhat, KAPPA, rest2, e)
    s = np.linalg.norm(_np(B.grad).astype(np.float64).sum(axis=0))
    print("BARRIER net force[%s]: |sum g| %.3e, sum of the vertex bounds %.3e, sum |g| %.3e" % (name, s, R.vbound.sum(),
                                                                                              np.linalg.norm(_np(B.grad), axis=1).sum()))
    assert s <= R.vbound.sum()


# ------------------------------------------------------------------------------------------------ 6: arguments
def test_arguments(pol):
    from zpc_amd import lib
    from zpc_amd.mesh import TriMesh
    v, t, _, dhat, _ = _scene("sheets")
    mesh = TriMesh(pol, v, t)
    prox = mesh.proximity(dhat)
    with pytest.raises(ValueError):
        mesh.barrier(prox, dhat, KAPPA)                      # mollify=True before set_rest
    with pytest.raises(ValueError):
        mesh.rest()
    plain = mesh.barrier(prox, dhat, KAPPA, mollify=False)   # ... which the unmollified potential does not need
    mesh.set_rest()
    for bad in (0.0, -0.01, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError):
            mesh.barrier(prox, bad, KAPPA)
        with pytest.raises(ValueError):
            mesh.barrier(prox, dhat, bad)
    with pytest.raises(ValueError):
        mesh.barrier(prox, dhat, KAPPA, verts=v[:-1])
    with pytest.raises(ValueError):
        mesh.barrier(None, dhat, KAPPA)
    with pytest.raises(ValueError):
        mesh.set_rest(v[:-1])
    # the C entries: -1 and nothing written
    L = lib()
    npt, nee = len(prox.pt_pairs), len(prox.ee_pairs)
    total = torch.full((), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full((mesh.nv, 3), 7.0, dtype=torch.float32, device="cuda")
    starts, entries, nscratch = prox._incidence
    scratch = torch.empty(nscratch, dtype=torch.float32, device="cuda")
    fresh = TriMesh(pol, v, t)

    def energy(m, d, k, mol):
        return L.zs_rocm_mesh_barrier_energy(pol.handle, m, None, prox.pt_pairs.data_ptr(), npt, prox.ee_pairs.data_ptr(), nee, d, k, mol, None, None,
                                             total.data_ptr(), None)

    def gradient(m, d, k, mol):
        return L.zs_rocm_mesh_barrier_gradient(pol.handle, m, None, prox.pt_pairs.data_ptr(), npt, prox.ee_pairs.data_ptr(), nee, d, k, mol,
                                               starts.data_ptr(), entries.data_ptr(), scratch.data_ptr(), None, None, total.data_ptr(),
                                               grad.data_ptr(), None)
    for fn in (energy, gradient):
        assert fn(None, dhat, KAPPA, 0) == -1 and fn(fresh.handle, dhat, KAPPA, 1) == -1
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert fn(mesh.handle, bad, KAPPA, 1) == -1 and fn(mesh.handle, dhat, bad, 1) == -1
    sizes = (__import__("ctypes").c_size_t * 3)()
    assert L.zs_rocm_mesh_barrier_sizes(None, npt, nee, sizes) == -1 and L.zs_rocm_mesh_set_rest(pol.handle, None, None) == -1
    assert L.zs_rocm_mesh_barrier_sizes(mesh.handle, npt, nee, sizes) == 0 and list(sizes) == [mesh.nv + 1, 4 * (npt + nee), 12 * (npt + nee)]
    assert L.zs_rocm_mesh_barrier_incidence(pol.handle, None, prox.pt_pairs.data_ptr(), npt, prox.ee_pairs.data_ptr(), nee, starts.data_ptr(),
                                            entries.data_ptr()) == -1
    pol.syncCtx()
    assert float(total.item()) == 7.0 and (grad == 7).all()
    # a Proximity with one side None: that side is skipped
    full = mesh.barrier(prox, dhat, KAPPA)
    only_pt, only_ee = mesh.proximity(dhat, ee=False), mesh.proximity(dhat, pt=False)
    P, E = mesh.barrier(only_pt, dhat, KAPPA), mesh.barrier(only_ee, dhat, KAPPA)
    assert P.ee_energy is None and E.pt_energy is None and len(P.pt_energy) > 0 and len(E.ee_energy) > 0
    _total_is_the_replay(P), _total_is_the_replay(E)
    assert _np(P.pt_energy).tobytes() == _np(full.pt_energy).tobytes() and _np(E.ee_energy).tobytes() == _np(full.ee_energy).tobytes()
    both = float(P.energy.item()) + float(E.energy.item())
    assert abs(both - float(full.energy.item())) <= 1e-14 * both and both > 0
    # unmollified EE energies are at least the mollified ones (m <= 1), PT energies do not depend on the mollifier
    assert _np(plain.pt_energy).tobytes() == _np(full.pt_energy).tobytes() and (_np(plain.ee_energy) >= _np(full.ee_energy)).all()


# ------------------------------------------------------------------------------------------------ 7: indices outside the mesh
def _spliced(pairs, bad):
    """pairs with the four rows of bad at positions 0, 255, 256 and last (the ends of the first workgroup, the start of the second, the
    ragged last one); returns the list and the mask of the rows that came from pairs"""
    n = len(pairs) + 4
    at = [0, 255, 256, n - 1]
    keep = np.ones(n, bool)
    keep[at] = False
    out = np.empty((n, 2), np.int32)
    out[at], out[keep] = bad, pairs
    return out, keep


def test_pairs_with_indices_outside_the_mesh_are_inactive(pol):
    from zpc_amd import lib
    from zpc_amd.mesh import Proximity
    import ref64_barrier_hessian as rh
    mesh, dhat = _mesh(pol, "sheets")
    nv, nt, ne = mesh.nv, mesh.nt, mesh.num_edges
    clean = mesh.proximity(dhat)
    assert len(clean.pt_pairs) > 512 and len(clean.ee_pairs) > 512      # the bad rows fall into three different workgroups per kind
    pt, kpt = _spliced(_np(clean.pt_pairs), [(-1, 0), (nv, 0), (0, -1), (0, nt)])
    ee, kee = _spliced(_np(clean.ee_pairs), [(-1, 0), (ne, 0), (0, -1), (0, ne)])
    keep = np.concatenate([kpt, kee])
    dirty = Proximity()
    dirty.pt_pairs, dirty.ee_pairs = torch.from_numpy(pt).cuda(), torch.from_numpy(ee).cuda()

    def same(what, zero, rows, out):
        """zero_distance, the per-pair rows (PT then EE) and the per-vertex or total output, each as (clean, dirty)"""
        assert zero[1] == zero[0], what
        c, d = (r.reshape(len(r), -1).view(np.uint32) for r in rows)
        assert len(d) == len(keep) and (d[~keep] == 0).all(), what
        assert np.array_equal(d[keep], c), what
        assert out[1].tobytes() == out[0].tobytes(), what

    def records(p):
        """the [4][3] records of the gradient call, which TriMesh.barrier does not return: the C entry on the incidence kept on p"""
        starts, entries, nscratch = p._incidence
        scratch = torch.empty(nscratch, dtype=torch.float32, device="cuda")
        grad = torch.empty(nv, 3, dtype=torch.float32, device="cuda")
        assert lib().zs_rocm_mesh_barrier_gradient(pol.handle, mesh.handle, None, p.pt_pairs.data_ptr(), len(p.pt_pairs), p.ee_pairs.data_ptr(),
                                                   len(p.ee_pairs), dhat, KAPPA, 1, starts.data_ptr(), entries.data_ptr(), scratch.data_ptr(),
                                                   None, None, None, grad.data_ptr(), None) == 0
        pol.syncCtx()
        return _np(scratch).reshape(-1, 4, 3), _np(grad)

    B = [mesh.barrier(p, dhat, KAPPA) for p in (clean, dirty)]
    energies = [np.concatenate([_np(b.pt_energy), _np(b.ee_energy)]) for b in B]
    same("energy", [b.zero_distance for b in B], energies, [_np(b.energy) for b in B])
    assert float(B[0].energy.item()) > 0
    recs = [records(p) for p in (clean, dirty)]
    same("gradient", [b.zero_distance for b in B], [r[0] for r in recs], [_np(b.grad) for b in B])
    assert recs[1][1].tobytes() == _np(B[1].grad).tobytes() and np.abs(_np(B[0].grad)).max() > 0
    E = mesh.barrier(dirty, dhat, KAPPA, gradient=False)      # the energy-only kernels decide the same
    assert np.concatenate([_np(E.pt_energy), _np(E.ee_energy)]).tobytes() == energies[1].tobytes()
    assert _np(E.energy).tobytes() == _np(B[1].energy).tobytes() and E.zero_distance == B[1].zero_distance
    x = rh.direction(nv, 1)
    for psd in (False, True):
        P = [mesh.barrier_hessian_product(p, dhat, KAPPA, x, psd=psd) for p in (clean, dirty)]
        same("product, psd %s" % psd, [p.zero_distance for p in P], [_np(p.pair_terms) for p in P], [_np(p.hx) for p in P])
        assert np.abs(_np(P[0].hx)).max() > 0
    print("BARRIER indices outside the mesh: %d + 4 PT, %d + 4 EE pairs; the 8 bad rows are zero, every other row, the total, grad and hx are "
          "those of the clean lists" % (len(clean.pt_pairs), len(clean.ee_pairs)))
