"""The float64 restatement of the mesh queries (tests/ref64_mesh.py) against closed forms, its bound against a float32 replay of the
device chain in numpy, the adjacency statistics, and the host logic of SparseLevelSet.from_mesh.  No GPU."""
import numpy as np
import pytest

import ref64_mesh as rm

BOX_LO, BOX_HI = (0.2, 0.3, 0.25), (0.8, 0.7, 0.75)   # 0.6 x 0.4 x 0.5


def test_box_mesh_equals_the_analytic_box_distance():
    """pins the vertex and edge pseudonormals: a face-normal sign is wrong in the vertex and edge regions"""
    v, t = rm.box_mesh(BOX_LO, BOX_HI)
    m = rm.Mesh64(v, t)
    assert m.stats == dict(boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0, zero_area_triangles=0, bad_indices=0)
    p = (np.random.default_rng(3).random((20000, 3)) * 1.2 - 0.1).astype(np.float32)
    r = m.query(p)
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    want = rm.box_sdf(p.astype(np.float64), lo, hi)
    side = tuple(np.unique(np.sign(np.round((p > lo).astype(int) + (p > hi).astype(int) - 1)), axis=0).shape)
    assert side == (27, 3)          # points on all 27 sides of the box
    assert set(np.unique(r["feature"])) == set(range(7))
    assert np.abs(r["sdf"] - want).max() <= 1e-15
    assert (want < 0).sum() > 1000 and (want > 0).sum() > 1000


def test_icosphere_lies_between_its_two_spheres():
    R = 0.4
    v, t = rm.icosphere(3, R)
    m = rm.Mesh64(v, t)
    assert len(t) == 1280 and m.stats["boundary_edges"] == 0 and m.stats["inconsistent_edges"] == 0
    e = m.longest_edge
    p = (np.random.default_rng(4).random((5000, 3)) * 1.2 - 0.6).astype(np.float32)
    r = m.query(p)
    diff = r["sdf"] - (np.linalg.norm(p.astype(np.float64), axis=1) - R)
    slack = 4 * rm.U * R              # the float32 vertices lie within u R of the sphere
    assert diff.min() >= -slack and diff.max() <= R - np.sqrt(R * R - e * e / 3) + slack


def test_adjacency_statistics():
    v, t = rm.icosphere(1)
    assert rm.Mesh64(v, t).stats["boundary_edges"] == 0
    s = rm.Mesh64(v, t[1:]).stats
    assert (s["boundary_edges"], s["nonmanifold_edges"], s["inconsistent_edges"]) == (3, 0, 0)
    f = t.copy()
    f[5] = f[5, ::-1]
    s = rm.Mesh64(v, f).stats
    assert (s["boundary_edges"], s["nonmanifold_edges"], s["inconsistent_edges"]) == (0, 0, 3)
    s = rm.Mesh64(v, np.concatenate([t, t[:1]])).stats
    assert (s["boundary_edges"], s["nonmanifold_edges"]) == (0, 3)
    z = np.concatenate([t, [[0, 0, 1]]])
    assert rm.Mesh64(v, z).stats["zero_area_triangles"] == 1


@pytest.mark.parametrize("shape", ["box", "icosphere", "torus", "degenerate"])
def test_float32_replay_of_the_device_chain_stays_within_the_bound(shape):
    """the same operations in numpy float32 (no fused multiply-adds): every per-triangle distance within b of the float64 one -- the
    evidence for the constant of the bound, from the CPU alone"""
    g = np.random.default_rng(7)
    if shape == "box":
        v, t = rm.box_mesh(BOX_LO, BOX_HI)
    elif shape == "icosphere":
        v, t = rm.icosphere(2, 0.4, (0.5, 0.5, 0.5))
    elif shape == "torus":
        v, t = rm.torus(16, 8, centre=(0.5, 0.5, 0.5))
    else:
        v, t = rm.icosphere(1, 0.4, (0.5, 0.5, 0.5))
        t = np.concatenate([t, [[0, 0, 0], [0, 1, 1], [2, 3, 2]], [[5, 6, 6]]]).astype(np.int32)
        v = np.concatenate([v, 0.5 * (v[[0]] + v[[1]])]).astype(np.float32)
        t = np.concatenate([t, [[0, len(v) - 1, 1]]]).astype(np.int32)       # three collinear vertices
    m = rm.Mesh64(v, t)
    p = (g.random((4000, 3)) * 1.4 - 0.2).astype(np.float32)
    worst = 0.0
    for i0, i1, i2 in t.tolist():
        d2, cp, bary, f = rm.tri_closest(p, v[i0], v[i1], v[i2], rm.DEGENERATE32)
        assert d2.dtype == np.float32 and np.isfinite(d2).all() and np.isfinite(cp).all() and np.isfinite(bary).all()
        e2, _, _, _ = rm.tri_closest(p.astype(np.float64), m.v[i0], m.v[i1], m.v[i2])
        b = m.bound(p, np.sqrt(e2))
        worst = max(worst, float((np.abs(np.sqrt(d2.astype(np.float64)) - np.sqrt(e2)) / b).max()))
        rec = sum(bary[:, k, None].astype(np.float64) * m.v[[i0, i1, i2][k]] for k in range(3))
        assert (np.linalg.norm(rec - cp, axis=1) <= b).all()
    print("MESH replay32[%s]: worst |d32 - d64| = %.3f of the bound" % (shape, worst))
    assert worst <= 1.0


def test_from_mesh_host_logic():
    from zpc_amd.mesh import default_origin, candidate_capacity
    o = default_origin((0.2, -0.31, 0.0), 1.0 / 64, 3.0 / 64)
    assert all(abs(x * 64 - round(x * 64)) < 1e-9 for x in o)
    assert all(a <= b - 3.0 / 64 + 1e-12 and a > b - 4.0 / 64 - 1e-12 for a, b in zip(o, (0.2, -0.31, 0.0)))
    cap = candidate_capacity(10 ** 9, (0.2, 0.2, 0.2), (0.8, 0.8, 0.8), o, 1.0 / 64, 3.0 / 64)
    assert 6 ** 3 <= cap <= 9 ** 3
    assert candidate_capacity(5, (0.2, 0.2, 0.2), (0.8, 0.8, 0.8), o, 1.0 / 64, 3.0 / 64) == 5
