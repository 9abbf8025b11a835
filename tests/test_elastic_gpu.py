"""Mesh elasticity on the GPU (zpc_amd/csrc/mesh_elastic.hip, TriMesh.set_rest_shape / rest_shape / elastic / elastic_hessian_product) against
tests/ref64_elastic.py on every scene of ref64_proximity.SCENES and on grid strips whose triangle and hinge counts sit at the 256-lane
workgroup edge: the rest records, the hinge list and the vertex areas bit for bit with the float32 replay; per-element energies, gradient
and product terms (exact and psd), the float64 total, grad and hx bit for bit with the replay (the gather replayed in run order) at trial
positions 1e-3, 1e-1 and 1 mean edge length from rest and under uniform compression to one half; grad and hx against float64 within the
derived bounds, no element and no vertex left out; determinism on `large`; zero stiffness; indices outside the mesh; a rest-degenerate
triangle and a non-manifold edge; the argument checks; and that set_rest_shape leaves rest() and a barrier gradient alone.  Prints one
`ELASTIC <what> ...` line per check.

Measured on an MI355X: every bit-for-bit comparison holds; against float64 the worst error over bound is 0.016 (a hinge energy on
strip8x16), 0.015 for grad (strip2x52) and 0.017 for hx (strip1x128, psd strip2x52), every bound finite; median bound / |force| on `sheets`
1.8e-2, 8.1e-3, 3.7e-3 and 1.2e-2 at 1e-3, 1e-1, 1 edge length and under compression; the file's 92 tests run in 2.9 s."""
import functools

import numpy as np
import pytest

import ref64_elastic as rl
import ref64_proximity as rp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MU, LAM, KB = rl.MU, rl.LAM, rl.KB
# a x b cells: 2 a b triangles, 3 a b - a - b hinges.  254 / 253, 256 / 255, 258 / 257, 256 / 360, 208 / 258, 204 / 253 (no grid has 254 or
# 256 hinges: 3 a b - a - b is even only for even a and b, and 6 k l - k - l is neither 127 nor 128)
STRIPS = ((1, 127), (1, 128), (1, 129), (8, 16), (2, 52), (2, 51))
NAMES = rp.SCENES + tuple("strip%dx%d" % s for s in STRIPS)
POSITIONS = ("1e-3", "1e-1", "1", "half")


def strip(a, b, seed=5):
    """(a + 1) x (b + 1) vertices, spacing 0.004, jittered in all three coordinates; two triangles per cell"""
    h = 0.004
    i, j = np.meshgrid(np.arange(a + 1), np.arange(b + 1), indexing="ij")
    v = np.stack([0.2 + h * i, 0.2 + h * j, np.full(i.shape, 0.5)], axis=-1).reshape(-1, 3)
    v = v + 0.4 * h * (np.random.default_rng(seed).random(v.shape) - 0.5)
    idx = lambda p, q: p * (b + 1) + q
    t = []
    for p in range(a):
        for q in range(b):
            t += [(idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)), (idx(p, q), idx(p + 1, q + 1), idx(p, q + 1))]
    return v.astype(np.float32), np.array(t, np.int32)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name.startswith("strip"):
        v, t = strip(*map(int, name[5:].split("x")))
    else:
        v, t, _ = rp.scene(name)
    return v, np.asarray(t, np.int32).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _rest(name, dtype):
    v, t = _scene(name)
    return rl.Rest(v, t, np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _position(name, which):
    v, t = _scene(name)
    return rl.compressed(v, 0.5) if which == "half" else rl.displaced(v, t, 1, float(which))


@functools.lru_cache(maxsize=None)
def _direction(name):
    return np.random.default_rng(77).standard_normal(_scene(name)[0].shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(name, which, dtype, psd):
    """(T, H, grad, hx) of the replay (float32) or the reference (float64), computed once and shared"""
    return _rest(name, dtype).evaluate(_position(name, which), MU, LAM, KB, _direction(name), psd)


def _mesh(pol, name):
    from zpc_amd.mesh import TriMesh
    v, t = _scene(name)
    mesh = TriMesh(pol, v, t)
    counts = mesh.set_rest_shape()
    return mesh, counts


def _np(x):
    return None if x is None else x.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1: the rest shape
@pytest.mark.parametrize("name", NAMES)
def test_the_rest_shape_bit_for_bit_with_the_replay(pol, name):
    mesh, counts = _mesh(pol, name)
    R = _rest(name, "float32")
    rec, hinges, hrec, area = (_np(x) for x in mesh.rest_shape())
    assert counts == R.counts and mesh.num_hinges == len(R.hinges)
    assert np.array_equal(hinges, R.hinges.astype(np.int32).reshape(-1, 4))
    assert _same(rec, R.tri_record) and _same(hrec, R.hinge_record) and _same(area, R.vertex_area)
    if len(hinges):      # the edge of a hinge is a row of edges(), in that order
        e = _np(mesh.edges())
        row = np.searchsorted(e[:, 0].astype(np.int64) * mesh.nv + e[:, 1], hinges[:, 0].astype(np.int64) * mesh.nv + hinges[:, 1])
        assert np.array_equal(e[row], hinges[:, :2]) and (np.diff(row) > 0).all()
    # a second call with other rest positions: new records on the same hinges; and back
    v, t = _scene(name)
    other = rl.compressed(v, 0.8)
    assert mesh.set_rest_shape(other) == rl.Rest(other, t, np.float32).counts
    rec2, hinges2, _, area2 = (_np(x) for x in mesh.rest_shape())
    R2 = rl.Rest(other, t, np.float32)
    assert _same(rec2, R2.tri_record) and np.array_equal(hinges2, hinges) and _same(area2, R2.vertex_area)
    assert mesh.set_rest_shape(torch.from_numpy(v).cuda()) == counts and _same(_np(mesh.rest_shape()[0]), rec)
    print("ELASTIC rest[%s]: %d triangles, %d hinges, %d vertices, counts %s; records, hinges and vertex areas bit for bit with the replay; "
          "total rest area %.6e" % (name, mesh.nt, len(hinges), mesh.nv, counts, float(area.astype(np.float64).sum())))
    if name == "torus":
        assert len(hinges) == mesh.num_edges      # closed: every edge is a hinge
    if name == "stack" or name.startswith("tiny"):
        assert len(hinges) == 0
    if name == "strip1x128":
        assert (mesh.nt, len(hinges)) == (256, 255)
    if name == "strip1x129":
        assert (mesh.nt, len(hinges)) == (258, 257)


# ------------------------------------------------------------------------------------------------ 2: elements, sums and totals: the bits
@pytest.mark.parametrize("which", POSITIONS)
@pytest.mark.parametrize("name", NAMES)
def test_elements_gradient_and_products_bit_for_bit_with_the_replay(pol, name, which):
    mesh, _ = _mesh(pol, name)
    pos, z = _position(name, which), _direction(name)
    T, H, grad, hx = _reference(name, which, "float32", False)
    Tp, Hp, _, hpx = _reference(name, which, "float32", True)
    E = mesh.elastic(MU, LAM, KB, verts=pos)
    assert E.overflow == (0, 0)
    assert _same(_np(E.tri_energy), T["eg"]) and _same(_np(E.hinge_energy), H["eg"])
    assert _same(_np(E.tri_terms), T["g"]) and _same(_np(E.hinge_terms), H["g"]) and _same(_np(E.grad), grad)
    want = rl.total(np.concatenate([T["eg"], H["eg"]]))
    assert float(E.energy.item()) == want
    E0 = mesh.elastic(MU, LAM, KB, verts=pos, gradient=False)
    assert E0.grad is None and E0.elem_terms is None and _same(_np(E0.tri_energy), T["e"]) and _same(_np(E0.hinge_energy), H["e"])
    assert float(E0.energy.item()) == rl.total(np.concatenate([T["e"], H["e"]]))
    P = mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos)
    Pp = mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos, psd=True)
    assert P.overflow == (0, 0) and Pp.overflow == (0, 0)
    assert _same(_np(P.tri_terms), T["h"]) and _same(_np(P.hinge_terms), H["h"]) and _same(_np(P.hx), hx)
    assert _same(_np(Pp.tri_terms), Tp["h"]) and _same(_np(Pp.hinge_terms), Hp["h"]) and _same(_np(Pp.hx), hpx)
    differ = int((_bits(Tp["h"]) != _bits(T["h"])).any(axis=(1, 2)).sum()) if mesh.nt else 0
    print("ELASTIC bits[%s, %s]: energies, gradient terms, product terms (exact and psd), the total %.9e, grad and hx bit for bit with the "
          "replay; %d of %d triangles with a projected stress" % (name, which, want, differ, mesh.nt))
    if which == "half" and mesh.nt and name != "stack":
        assert differ == mesh.nt      # compressed everywhere
    if name == "tiny0":
        assert want == 0.0 and (_np(E.grad) == 0).all() and (_np(P.hx) == 0).all() and E.elem_terms.numel() == 0


def test_the_mesh_own_positions_are_the_default(pol):
    mesh, _ = _mesh(pol, "sheets")
    v, _ = _scene("sheets")
    a, b = mesh.elastic(MU, LAM, KB), mesh.elastic(MU, LAM, KB, verts=v)
    assert _same(_np(a.grad), _np(b.grad)) and float(a.energy.item()) == float(b.energy.item())
    z = _direction("sheets")
    assert _same(_np(mesh.elastic_hessian_product(MU, LAM, KB, z).hx), _np(mesh.elastic_hessian_product(MU, LAM, KB, z, verts=v).hx))


# ------------------------------------------------------------------------------------------------ 3: against float64 within the bounds
def _ratio(err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0, 0.0, err / bound)


@pytest.mark.parametrize("name", NAMES)
def test_grad_and_hx_against_float64_within_the_bounds(pol, name):
    mesh, _ = _mesh(pol, name)
    R, z = _rest(name, "float64"), _direction(name)
    X = R.X[R.tris]
    worst, med = {}, {}
    for which in POSITIONS:
        pos = _position(name, which)
        T, H, grad, hx = _reference(name, which, "float64", False)
        Tp, Hp, _, hpx = _reference(name, which, "float64", True)
        bg, bh = R.vertex_bounds(pos, MU, LAM, KB, T, H, z)
        _, bhp = R.vertex_bounds(pos, MU, LAM, KB, Tp, Hp, z)
        x64 = pos.astype(np.float64)
        be, _, _ = rl.tri_bounds(X, x64[R.tris], R.tri_record, MU, LAM)
        he, _, _ = rl.hinge_bounds(R.X[R.hinges], x64[R.hinges], KB)
        assert np.isfinite(bg).all() and np.isfinite(bh).all() and np.isfinite(bhp).all() and np.isfinite(be).all() and np.isfinite(he).all()
        E = mesh.elastic(MU, LAM, KB, verts=pos)
        P, Pp = mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos), mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos, psd=True)
        top = lambda r: float(r.max()) if len(r) else 0.0
        worst[which] = (top(_ratio(np.abs(_np(E.tri_energy) - T["e"]), be)), top(_ratio(np.abs(_np(E.hinge_energy) - H["e"]), he)),
                        top(_ratio(rl._norm(_np(E.grad) - grad), bg)), top(_ratio(rl._norm(_np(P.hx) - hx), bh)),
                        top(_ratio(rl._norm(_np(Pp.hx) - hpx), bhp)))
        size = np.linalg.norm(grad, axis=1)
        med[which] = float(np.median(bg[size > 0] / size[size > 0])) if (size > 0).any() else 0.0
        total64 = T["e"].sum() + H["e"].sum()
        assert abs(float(E.energy.item()) - total64) <= be.sum() + he.sum() + 1e-12 * abs(total64)
    print("ELASTIC float64[%s]: %d vertices, all bounds finite; worst error over bound (triangle energy, hinge energy, grad, hx, psd hx): %s; "
          "median bound / |force| %s" % (name, mesh.nv, "; ".join("%s: %s" % (k, " ".join("%.3f" % x for x in w)) for k, w in worst.items()),
                                         " ".join("%.2e" % med[k] for k in POSITIONS)))
    assert max(max(w) for w in worst.values()) <= 1
    if name == "sheets":
        assert med["1e-1"] <= 2 * rl.SHEETS_MEDIAN_BOUND_OVER_G


# ------------------------------------------------------------------------------------------------ 4: determinism, zero stiffness
def test_two_calls_on_large_give_the_same_bytes(pol):
    from zpc_amd.mesh import TriMesh
    v, t, _ = rp.scene("large")
    mesh = TriMesh(pol, v, t)
    assert mesh.set_rest_shape() == (0, 0, 0)
    pos = rl.displaced(v, t, 1, 1e-1)
    z = np.random.default_rng(5).standard_normal(v.shape).astype(np.float32)
    a, b = mesh.elastic(MU, LAM, KB, verts=pos), mesh.elastic(MU, LAM, KB, verts=pos)
    p, q = mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos, psd=True), mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos, psd=True)
    assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)) and torch.equal(a.energy.view(torch.int64), b.energy.view(torch.int64))
    assert torch.equal(p.hx.view(torch.int32), q.hx.view(torch.int32)) and torch.equal(p.elem_terms.view(torch.int32), q.elem_terms.view(torch.int32))
    r1, r2 = mesh.rest_shape(), (mesh.set_rest_shape(), mesh.rest_shape())[1]
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    print("ELASTIC determinism[large]: %d triangles, %d hinges; energy %.9e; two calls, the same bytes" % (mesh.nt, mesh.num_hinges, float(a.energy.item())))
    assert mesh.num_hinges == mesh.num_edges - 2 * 4 * 95 and float(a.energy.item()) > 0 and (a.grad != 0).any()


def test_zero_stiffness_gives_exact_zeros(pol):
    mesh, _ = _mesh(pol, "sheets")
    pos, z = _position("sheets", "1e-1"), _direction("sheets")
    nt = mesh.nt
    full = mesh.elastic(MU, LAM, KB, verts=pos)
    m = mesh.elastic(MU, LAM, 0.0, verts=pos)
    b = mesh.elastic(0.0, 0.0, KB, verts=pos)
    assert (_bits(_np(m.hinge_energy)) == 0).all() and (_bits(_np(m.hinge_terms)) == 0).all() and _same(_np(m.tri_terms), _np(full.tri_terms))
    assert (_bits(_np(b.tri_energy)) == 0).all() and (_bits(_np(b.tri_terms)) == 0).all() and _same(_np(b.hinge_terms), _np(full.hinge_terms))
    none = mesh.elastic(0.0, 0.0, 0.0, verts=pos)
    assert float(none.energy.item()) == 0.0 and (_bits(_np(none.grad)) == 0).all() and (_bits(_np(none.elem_terms)) == 0).all()
    hm, hb = mesh.elastic_hessian_product(MU, LAM, 0.0, z, verts=pos), mesh.elastic_hessian_product(0.0, 0.0, KB, z, verts=pos, psd=True)
    hf = mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos)
    assert (_bits(_np(hm.hinge_terms)) == 0).all() and _same(_np(hm.tri_terms), _np(hf.tri_terms))
    assert (_bits(_np(hb.tri_terms)) == 0).all() and _same(_np(hb.hinge_terms), _np(hf.hinge_terms))
    assert (_bits(_np(mesh.elastic_hessian_product(0.0, 0.0, 0.0, z, verts=pos).hx)) == 0).all()
    # mu = 0 alone is an ordinary input
    T, H, grad, _ = _rest("sheets", "float32").evaluate(pos, 0.0, LAM, KB)
    assert _same(_np(mesh.elastic(0.0, LAM, KB, verts=pos).grad), grad)
    print("ELASTIC zero stiffness[sheets]: mu = lam = 0 and kb = 0 give zero bytes, %d triangles, %d hinges" % (nt, mesh.num_hinges))


# ------------------------------------------------------------------------------------------------ 5: degenerate input
def test_indices_outside_the_mesh_are_rejected(pol):
    from zpc_amd.mesh import TriMesh
    v, t = _scene("tiny2")
    for bad in (-1, len(v)):
        t2 = t.copy()
        t2[1, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            TriMesh(pol, v, t2)


def test_a_degenerate_triangle_and_a_nonmanifold_edge_are_counted_and_contribute_zero(pol):
    from zpc_amd.mesh import TriMesh
    v, t = strip(2, 3)
    v, t = v.copy(), t.copy()
    nv = len(v)
    # triangle 0 collapsed at rest: its vertex 0 moved onto the opposite edge's first vertex; a third triangle on the edge (5, 6)
    v[t[0, 0]] = v[t[0, 1]]
    fin = np.concatenate([v, [[0.21, 0.21, 0.52]]]).astype(np.float32)
    t = np.concatenate([t, [[5, 6, nv]]]).astype(np.int32)
    assert sum(1 for tri in t.tolist() if 5 in tri and 6 in tri) == 3
    mesh = TriMesh(pol, fin, t)
    counts = mesh.set_rest_shape()
    R = rl.Rest(fin, t, np.float32)
    assert counts == R.counts and counts[0] == 1 and counts[1] >= 1 and counts[2] == 1
    rec, hinges, hrec, area = (_np(x) for x in mesh.rest_shape())
    assert _same(rec, R.tri_record) and np.array_equal(hinges, R.hinges) and _same(hrec, R.hinge_record) and _same(area, R.vertex_area)
    assert (_bits(rec[0]) == 0).all() and not ((hinges[:, 0] == 5) & (hinges[:, 1] == 6)).any()
    pos, z = rl.displaced(fin, t, 2, 1e-1), np.random.default_rng(9).standard_normal(fin.shape).astype(np.float32)
    T, H, grad, hx = R.evaluate(pos, MU, LAM, KB, z)
    E, P = mesh.elastic(MU, LAM, KB, verts=pos), mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos)
    dead = (_bits(hrec) == 0).all(axis=1)
    assert (_bits(_np(E.tri_terms)[0]) == 0).all() and _np(E.tri_energy)[0] == 0 and (_bits(_np(P.tri_terms)[0]) == 0).all()
    assert dead.sum() == counts[1] and (_bits(_np(E.hinge_terms)[dead]) == 0).all() and (_bits(_np(P.hinge_terms)[dead]) == 0).all()
    assert _same(_np(E.grad), grad) and _same(_np(P.hx), hx) and E.overflow == (0, 0) and np.isfinite(_np(E.grad)).all()
    print("ELASTIC degenerate: counts %s (degenerate triangles, degenerate hinges, non-manifold edges); they contribute zero bytes" % (counts,))


def test_overflow_is_counted_and_contributes_zero(pol):
    mesh, _ = _mesh(pol, "strip2x51")
    v, t = _scene("strip2x51")
    pos = v.copy()
    pos[0] = 1e15      # the corner vertex of triangles 0 and 1: their strain overflows; no hinge term does (kb w stays finite)
    z = _direction("strip2x51")
    R = _rest("strip2x51", "float32")
    T, H, grad, hx = R.evaluate(pos, MU, LAM, KB, z)
    E = mesh.elastic(MU, LAM, KB, verts=pos)
    want = (int((T["st_g"] == rl.OVERFLOW).sum()), int((H["st_g"] == rl.OVERFLOW).sum()))
    assert E.overflow == want and want[0] == 2
    assert _same(_np(E.grad), grad) and _same(_np(E.tri_energy), T["eg"]) and np.isfinite(_np(E.grad)).all() and np.isfinite(float(E.energy.item()))
    P = mesh.elastic_hessian_product(MU, LAM, KB, z, verts=pos)
    assert P.overflow == (int((T["st_h"] == rl.OVERFLOW).sum()), int((H["st_h"] == rl.OVERFLOW).sum())) and _same(_np(P.hx), hx)
    print("ELASTIC overflow: %s triangles and hinges counted by the gradient, %s by the product; no NaN" % (E.overflow, P.overflow))


# ------------------------------------------------------------------------------------------------ 6: arguments, and the contact side
def test_the_argument_checks(pol, hiplib):
    from zpc_amd.mesh import TriMesh
    v, t = _scene("tiny2")
    mesh = TriMesh(pol, v, t)
    z = np.zeros_like(v)
    with pytest.raises(ValueError, match="set_rest_shape first"):
        mesh.elastic(MU, LAM, KB)
    with pytest.raises(ValueError, match="set_rest_shape first"):
        mesh.elastic_hessian_product(MU, LAM, KB, z)
    with pytest.raises(ValueError, match="set_rest_shape first"):
        mesh.rest_shape()
    h, f32 = mesh.handle, np.float32
    sizes = (__import__("ctypes").c_size_t * 7)()
    assert hiplib.zs_rocm_mesh_rest_shape_sizes(h, sizes) == -1
    assert hiplib.zs_rocm_mesh_elastic_energy(pol.handle, h, None, MU, LAM, KB, None, None, None, None) == -1      # no rest shape
    with pytest.raises(ValueError, match="same topology"):
        mesh.set_rest_shape(v[:-1])
    mesh.set_rest_shape()
    for bad in (-1.0, float("nan"), float("inf"), 1e39):
        for args in ((bad, LAM, KB), (MU, bad, KB), (MU, LAM, bad)):
            with pytest.raises(ValueError, match="finite and not negative"):
                mesh.elastic(*args)
            with pytest.raises(ValueError, match="finite and not negative"):
                mesh.elastic_hessian_product(*args, z)
    with pytest.raises(ValueError, match="same topology"):
        mesh.elastic(MU, LAM, KB, verts=v[:-1])
    with pytest.raises(ValueError, match="direction"):
        mesh.elastic_hessian_product(MU, LAM, KB, z[:-1])
    out = torch.zeros(mesh.nv, 3, device="cuda")
    scratch = torch.zeros(9 * mesh.nt + 12 * mesh.num_hinges, device="cuda")
    x = torch.zeros(mesh.nv, 3, device="cuda")
    E, G, P = hiplib.zs_rocm_mesh_elastic_energy, hiplib.zs_rocm_mesh_elastic_gradient, hiplib.zs_rocm_mesh_elastic_hessian_product
    assert E(None, h, None, MU, LAM, KB, None, None, None, None) == -1 and E(pol.handle, None, None, MU, LAM, KB, None, None, None, None) == -1
    assert E(pol.handle, h, None, -1.0, LAM, KB, None, None, None, None) == -1 and E(pol.handle, h, None, MU, float("nan"), KB, None, None, None, None) == -1
    assert E(pol.handle, h, None, MU, LAM, float("inf"), None, None, None, None) == -1
    assert G(pol.handle, h, None, MU, LAM, KB, scratch.data_ptr(), None, None, None, None, None) == -1      # no grad
    assert G(pol.handle, h, None, MU, LAM, KB, None, None, None, None, out.data_ptr(), None) == -1          # no scratch
    assert P(pol.handle, h, None, MU, LAM, KB, 0, None, scratch.data_ptr(), out.data_ptr(), None) == -1     # no x
    assert P(pol.handle, h, None, MU, LAM, KB, 0, x.data_ptr(), scratch.data_ptr(), None, None) == -1       # no hx
    assert P(pol.handle, h, None, MU, LAM, KB, 0, x.data_ptr(), None, out.data_ptr(), None) == -1           # no scratch
    assert hiplib.zs_rocm_mesh_set_rest_shape(pol.handle, None, None) == -1 and hiplib.zs_rocm_mesh_rest_shape(pol.handle, None, None, None, None, None) == -1
    assert (out == 0).all()      # nothing written
    assert E(pol.handle, h, None, MU, LAM, KB, None, None, None, None) == 0      # every output may be NULL
    assert G(pol.handle, h, None, MU, LAM, KB, scratch.data_ptr(), None, None, None, out.data_ptr(), None) == 0
    pol.syncCtx()
    assert _same(_np(out), _np(mesh.elastic(MU, LAM, KB).grad))


def test_set_rest_shape_leaves_rest_and_the_barrier_alone(pol):
    from zpc_amd.mesh import TriMesh
    v, t, dhat = rp.scene("sheets")
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    prox = mesh.proximity(dhat)
    rest0, b0 = mesh.rest().clone(), mesh.barrier(prox, dhat, 1.0)
    mesh.set_rest_shape(rl.compressed(v, 0.9))
    mesh.elastic(MU, LAM, KB)
    rest1, b1 = mesh.rest(), mesh.barrier(prox, dhat, 1.0)
    assert torch.equal(rest0.view(torch.int32), rest1.view(torch.int32)) and torch.equal(b0.grad.view(torch.int32), b1.grad.view(torch.int32))
    assert torch.equal(b0.energy.view(torch.int64), b1.energy.view(torch.int64)) and (b0.grad != 0).any()
    p1 = mesh.proximity(dhat)
    assert torch.equal(prox.pt_pairs, p1.pt_pairs) and torch.equal(prox.ee_pairs, p1.ee_pairs)
