"""Triangle-mesh colliders on the GPU (include/zensim_rocm/distance_device.hpp, mesh_device.hpp, zpc_amd/csrc/mesh.hip, zpc_amd/mesh.py,
SparseLevelSet.from_mesh): closest point and signed distance against the float64 brute force with per-point bounds
(tests/ref64_mesh.py), determinism, refit, mesh -> level set against from_dense of the reference's dense field, the boundary pass end to
end, the per-lane fallback, open meshes and the C++ face.  Prints one `MESH <what> ...` line per check."""
import os
import subprocess

import numpy as np
import pytest

import ref64_mesh as rm
import ref64_levelset as rl
from util import make_cloud, rng

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = rm.U
BOX_LO, BOX_HI = (0.213, 0.307, 0.251), (0.813, 0.707, 0.751)   # 0.6 x 0.4 x 0.5, off every lattice used here


def _vel_of(v):
    v = np.asarray(v, np.float64)
    return np.stack([0.3 * v[:, 1], -0.2 * v[:, 2] + 0.1, 0.25 * v[:, 0]], axis=-1).astype(np.float32)


VEL_A = np.array([[0, 0.3, 0], [0, 0, -0.2], [0.25, 0, 0]])   # _vel_of is x -> VEL_A x + (0, 0.1, 0)


def _shape(name):
    if name == "box":
        return rm.box_mesh(BOX_LO, BOX_HI)
    if name == "icosphere":
        return rm.icosphere(3, 0.31, (0.5, 0.47, 0.53))
    if name == "torus":
        return rm.torus(24, 12, 0.3, 0.11, (0.5, 0.5, 0.5))
    v, t = rm.icosphere(2, 0.31, (0.5, 0.47, 0.53))      # "degenerate": zero-area triangles mixed in
    nv = len(v)
    v = np.concatenate([v, [[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [0.75, 0.75, 0.75]]]).astype(np.float32)   # exactly collinear
    extra = [[0, 0, 0], [3, 4, 4], [7, 9, 7], [nv, nv + 1, nv + 2], [5, 5, 5]]
    g = rng(5)
    t = np.concatenate([t, extra]).astype(np.int32)
    return v, t[g.permutation(len(t))]


def _points(v, n, seed, pad=0.15):
    lo, hi = v.min(0) - pad, v.max(0) + pad
    return (lo + rng(seed).random((n, 3)) * (hi - lo)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1: closest point
@pytest.mark.parametrize("shape", ["box", "icosphere", "torus", "degenerate"])
def test_closest_point_against_the_float64_brute_force(pol, shape):
    from zpc_amd.mesh import TriMesh
    v, t = _shape(shape)
    mesh, ref = TriMesh(pol, v, t), rm.Mesh64(v, t)
    assert mesh.stats() == ref.stats
    p = _points(v, 20000, 21)
    r = ref.query(p)
    dist, tri, feat, bary = (x.cpu().numpy() for x in mesh.closest_point(p))
    assert np.isfinite(dist).all() and np.isfinite(bary).all() and (tri >= 0).all() and (tri < len(t)).all()
    ratio = np.abs(dist - r["d"]) / r["b"]
    other = tri != r["tri"]
    d_other = ref.tri_distance(p[other], tri[other])
    cp = sum(bary[:, k, None].astype(np.float64) * ref.v[ref.t[tri, k]] for k in range(3))
    rcp = np.abs(np.linalg.norm(p - cp, axis=1) - r["d"]) / r["b"]
    # the feature names where the barycentrics put the point
    on_vertex, on_edge = feat < 3, (feat >= 3) & (feat < 6)
    assert (bary[on_vertex].max(axis=1) == 1).all() and ((bary[on_edge] == 0).sum(axis=1) >= 1).all()
    print("MESH closest[%s]: %d triangles, dist %.3f of the bound, closest point %.3f, %d other triangles (worst %.3f), features %s"
          % (shape, len(t), ratio.max(), rcp.max(), other.sum(), ((d_other - r["d"][other]) / r["b"][other]).max() if other.any() else 0.0,
             np.bincount(feat, minlength=7).tolist()))
    assert (ratio <= 1).all() and (rcp <= 1).all()
    assert (d_other - r["d"][other] <= r["b"][other]).all()
    # cap: points farther than cap return cap and -1
    cap = float(np.median(r["d"]))
    dc, tc, fc, _ = (x.cpu().numpy() for x in mesh.closest_point(p, cap=cap))
    far, near = r["d"] > cap + r["b"], r["d"] < cap - r["b"]
    assert far.sum() > 1000 and near.sum() > 1000
    assert (dc[far] == np.float32(cap)).all() and (tc[far] == -1).all() and (fc[far] == -1).all()
    assert np.array_equal(dc[near].view(np.uint32), dist[near].view(np.uint32)) and (tc[near] >= 0).all()


@pytest.mark.parametrize("nt", [0, 1, 2])
def test_small_meshes_take_the_small_tree_path(pol, nt):
    from zpc_amd.mesh import TriMesh, FLT_MAX
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float32)
    t = np.array([[0, 1, 2], [1, 3, 2]], np.int32)[:nt]
    mesh = TriMesh(pol, v, t)
    p = _points(v, 3000, 3, 0.5)
    dist, tri, feat, bary = (x.cpu().numpy() for x in mesh.closest_point(p))
    if nt == 0:
        assert (dist == np.float32(FLT_MAX)).all() and (tri == -1).all()
        return
    r = rm.Mesh64(v, t).query(p)
    assert (np.abs(dist - r["d"]) <= r["b"]).all() and (tri >= 0).all() and (tri < nt).all()
    sdf, _ = mesh.signed_distance(p, allow_open=True)
    assert (np.abs(np.abs(sdf.cpu().numpy()) - r["d"]) <= r["b"]).all()


# ------------------------------------------------------------------------------------------------ 2: signed distance
@pytest.mark.parametrize("shape", ["box", "icosphere", "torus"])
def test_signed_distance_and_velocity(pol, shape):
    from zpc_amd.mesh import TriMesh
    v, t = _shape(shape)
    mesh, ref = TriMesh(pol, v, t, _vel_of(v)), rm.Mesh64(v, t, _vel_of(v))
    p = _points(v, 20000, 22)
    r = ref.query(p, ambiguity=True)
    sdf, vel = (x.cpu().numpy() for x in mesh.signed_distance(p))
    sure = np.abs(r["sdf"]) > r["b"]
    share = 1 - sure.mean()
    ratio = np.abs(np.abs(sdf) - r["d"]) / r["b"]
    # the vertex velocities are a linear field x -> VEL_A x + c, which interpolation reproduces: the velocity moves with the closest point,
    # and a result inside the bound may take its closest point from any triangle within 2 b of the minimum (amb, from the reference alone)
    bv = np.linalg.norm(VEL_A, 2) * (r["amb"] + r["b"]) + 8 * U * np.abs(ref.vel).max() + 1e-37
    rv = np.abs(vel - r["vel"]).max(axis=1) / bv
    print("MESH signed[%s]: %d inside, %d excluded (share %.2e), |sdf| %.3f of the bound, velocity %.3f of its bound (%d points with an ambiguous "
          "closest point)" % (shape, (r["sdf"] < 0).sum(), (~sure).sum(), share, ratio.max(), rv.max(), (r["amb"] > r["b"]).sum()))
    assert share <= 0.01 and (r["sdf"] < 0).sum() > 500
    assert np.array_equal(sdf[sure] < 0, r["sdf"][sure] < 0)
    assert (ratio <= 1).all() and (rv <= 1).all()
    assert (r["amb"] <= r["b"]).mean() > 0.9      # the velocity check is sharp on most points
    if shape == "box":
        want_box = rm.box_sdf(p.astype(np.float64), ref.v.min(0), ref.v.max(0))
        assert (np.abs(sdf - want_box) <= r["b"]).all()


# ------------------------------------------------------------------------------------------------ 3: determinism and refit
def _state(mesh, p):
    out = [x.cpu().numpy() for x in mesh.closest_point(p)] + [x.cpu().numpy() for x in mesh.signed_distance(p, allow_open=True) if x is not None]
    return list(mesh.normals()) + out


def test_the_same_mesh_gives_the_same_bits_and_refit_equals_a_fresh_mesh(pol):
    from zpc_amd.mesh import TriMesh
    v, t = _shape("icosphere")
    p = _points(v, 30000, 23)
    a, b = TriMesh(pol, v, t, _vel_of(v)), TriMesh(pol, v, t, _vel_of(v))
    for x, y in zip(_state(a, p), _state(b, p)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    g = rng(9)
    moved = (v * np.float32(1.07) + np.float32(0.03) + 0.004 * g.standard_normal(v.shape)).astype(np.float32)
    a.refit(moved, _vel_of(moved))
    fresh = TriMesh(pol, moved, t, _vel_of(moved))
    assert a.stats() == fresh.stats()
    nf, nvn, ne = a.normals()
    assert np.abs(np.linalg.norm(nf, axis=1) - 1).max() < 1e-5
    # (the tree is refitted, not rebuilt: its boxes are the same set unions, so the nearest triangle and with it every output agrees)
    for x, y in zip(_state(a, p), _state(fresh, p)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    print("MESH determinism / refit: %d triangles, %d points, bit-equal" % (len(t), len(p)))


# ------------------------------------------------------------------------------------------------ 4: mesh -> level set
def _dense_reference(ref, origin, voxel, lo_idx, hi_idx):
    idx = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo_idx, hi_idx)], indexing="ij"), axis=-1)
    x = np.asarray(origin, np.float64) + voxel * idx
    return ref.query(x.reshape(-1, 3).astype(np.float32), ambiguity=True), idx.shape[:3]


@pytest.mark.parametrize("shape", ["box", "icosphere", "torus"])
def test_from_mesh_against_from_dense_of_the_reference_field(pol, shape):
    from zpc_amd.mesh import TriMesh
    from zpc_amd.levelset import SparseLevelSet, select_blocks
    v, t = _shape(shape)
    if shape == "icosphere":
        v, t = rm.icosphere(2, 0.31, (0.5, 0.47, 0.53))
    voxel, band = 1.0 / 48, 3.0 / 48
    mesh, ref = TriMesh(pol, v, t, _vel_of(v)), rm.Mesh64(v, t, _vel_of(v))
    ls = SparseLevelSet.from_mesh(pol, mesh, voxel, band)
    origin = np.array(ls.origin)
    assert (origin <= v.min(0) - band + 1e-6).all() and (origin > v.min(0) - band - voxel - 1e-6).all()
    n = (np.ceil((v.max(0) + band - origin) / voxel).astype(int) + 1 + 7) // 8 * 8
    r, shape3 = _dense_reference(ref, np.float32(origin), np.float32(voxel), (0, 0, 0), n)
    sdf64, b = r["sdf"].reshape(shape3), r["b"].reshape(shape3)
    want_keys, want_cells = select_blocks(sdf64.astype(np.float32), band, band)
    got = {tuple(k): i for i, k in enumerate(ls.keys.tolist())}
    want = {tuple(k) for k in want_keys.tolist()}
    # a block whose decision hangs on a cell with ||sdf64| - band| <= b may go either way
    blocks = np.abs(sdf64).reshape(n[0] // 8, 8, n[1] // 8, 8, n[2] // 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(n[0] // 8, n[1] // 8, n[2] // 8, 512)
    bb = b.reshape(n[0] // 8, 8, n[1] // 8, 8, n[2] // 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(n[0] // 8, n[1] // 8, n[2] // 8, 512)
    surely_in, surely_out = (blocks < band - bb).any(-1), (blocks >= band + bb).all(-1)
    unsure = sorted(set(got) ^ want)
    for k in unsure:
        i = tuple(np.array(k) // 8)
        assert not surely_in[i] and not surely_out[i], k
    assert len(unsure) <= 0.01 * len(want)
    assert set(got) - want <= {k for k in got if all(0 <= c < m for c, m in zip(k, n))}
    # numbering: lexicographic
    assert ls.keys.tolist() == sorted(ls.keys.tolist()) and ls.nblocks == len(got)
    # every cell of every common block: sdf within b, "v" within the bound its closest point's ambiguity allows
    dense = ls.to_dense((0, 0, 0), n)
    common = np.zeros(shape3, bool)
    for k in set(got) & want:
        common[k[0]:k[0] + 8, k[1]:k[1] + 8, k[2]:k[2] + 8] = True
    ratio = (np.abs(dense[..., 0] - sdf64) / b)[common]
    vref = r["vel"].reshape(shape3 + (3,))
    bv = np.linalg.norm(VEL_A, 2) * (r["amb"].reshape(shape3) + b) + 8 * U * np.abs(ref.vel).max()
    rv = (np.abs(dense[..., 1:4] - vref).max(-1) / bv)[common]
    stats = ls.build_stats
    print("MESH from_mesh[%s]: %d blocks (%d undecided: %s), candidates rejected / staged / per-lane / kept %s, sdf %.3f of the bound, v %.3f"
          % (shape, ls.nblocks, len(unsure), unsure[:4], stats.tolist(), ratio.max(), rv.max()))
    assert common.sum() >= 512 * 0.99 * len(want) and (ratio <= 1).all() and (rv <= 1).all()
    assert stats[3] == ls.nblocks and stats[1] > 0
    # absent blocks read as background; to_dense round trip through from_dense
    absent = np.ones(shape3, bool)
    for k in got:
        absent[k[0]:k[0] + 8, k[1]:k[1] + 8, k[2]:k[2] + 8] = False
    assert (dense[absent] == np.float32(band)).all()
    again = SparseLevelSet.from_dense(pol, dense[..., 0], origin, voxel, band, vel=dense[..., 1:4])
    assert again.keys.tolist() == ls.keys.tolist()
    assert np.array_equal(again.to_dense((0, 0, 0), n).view(np.uint32), dense.view(np.uint32))
    # update_from_mesh after a translation == a fresh from_mesh with the same origin
    moved = (v + np.float32(0.013)).astype(np.float32)
    mesh.refit(moved, _vel_of(moved))
    ls.update_from_mesh(mesh)
    fresh = SparseLevelSet.from_mesh(pol, TriMesh(pol, moved, t, _vel_of(moved)), voxel, band, origin=origin)
    assert fresh.keys.tolist() == ls.keys.tolist() and ls.nblocks > 0
    assert np.array_equal(fresh.to_dense((0, 0, 0), n).view(np.uint32), ls.to_dense((0, 0, 0), n).view(np.uint32))


def test_blocks_over_the_stage_fall_back_to_the_per_lane_walk(pol):
    """a dense cluster of small triangles in one block: more candidates than the LDS list holds"""
    from zpc_amd.mesh import TriMesh
    from zpc_amd.levelset import SparseLevelSet
    v, t = rm.icosphere(2, 0.31, (0.5, 0.47, 0.53))
    cv, ct = rm.icosphere(3, 0.02, (0.5, 0.47, 0.53 + 0.4))      # 1280 triangles inside 0.04: two voxels
    v2, t2 = np.concatenate([v, cv]).astype(np.float32), np.concatenate([t, ct + len(v)]).astype(np.int32)
    voxel, band = 1.0 / 48, 3.0 / 48
    mesh, ref = TriMesh(pol, v2, t2), rm.Mesh64(v2, t2)
    assert mesh.is_closed()
    ls = SparseLevelSet.from_mesh(pol, mesh, voxel, band)
    stats = ls.build_stats
    assert stats[2] > 0 and stats[1] > 0 and stats[3] == ls.nblocks
    # the blocks around the cluster against the reference
    centre = np.array([0.5, 0.47, 0.93])
    lo = (np.floor((centre - 0.1 - np.array(ls.origin)) / voxel).astype(int) // 8) * 8
    hi = lo + 16
    r, shape3 = _dense_reference(ref, np.float32(ls.origin), np.float32(voxel), lo, hi)
    dense = ls.to_dense(lo, hi)[..., 0]
    stored = dense != np.float32(band)
    ratio = (np.abs(dense - r["sdf"].reshape(shape3)) / r["b"].reshape(shape3))[stored]
    print("MESH fallback: candidates rejected / staged / per-lane / kept %s, %d cells checked, sdf %.3f of the bound"
          % (stats.tolist(), stored.sum(), ratio.max()))
    assert stored.sum() >= 512 and (ratio <= 1).all()


# ------------------------------------------------------------------------------------------------ 5: the boundary pass, end to end
@pytest.mark.parametrize("ctype", [0, 1, 2])
def test_apply_boundary_with_a_level_set_from_a_mesh(pol, ctype):
    """MpmTransfer.apply_boundary(levelset=from_mesh(box mesh)) and apply_boundary(levelset=from_dense(analytic box sdf)) on the same
    lattice, both against tests/ref64_levelset.py on the analytic cells with every sdf sample's bound widened by `pert`, the largest
    per-cell difference the mesh path may show (the bound b of ref64_mesh on the lattice plus the float32 rounding of the two stored
    values; asserted cell by cell below).  ref64_levelset carries that through the central differences, the per-node gradient length,
    the normal and the response.  Left out: nodes whose reference distance lies within its widened bound of zero, at most 1 % of the
    touched nodes; every other node with mass is compared.  band = 7 cells covers the whole interior of the box (half extent 6.03
    cells), so no node samples the background from inside."""
    from zpc_amd.mesh import TriMesh
    from zpc_amd.levelset import SparseLevelSet, select_blocks
    from zpc_amd.mpm import MpmTransfer, make_levelset_collider
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(10, dx, 4, seed=11)
    pos = (pos - pos.mean(0)).astype(np.float32) * np.float32(1.5)
    mt = MpmTransfer(pol, pos.shape[0], dx, dt, model=0, side=8, volume=dx ** 3 / 4)
    mt.upload(mass, pos, vel, Cm, F)
    mt.build_partition(4096)
    mt.rebin()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    pol.syncCtx()
    blo, bhi = (-0.0731, -0.1513, -0.0417), (0.2119, 0.0371, 0.1893)     # off the lattice; the cloud straddles its faces
    v, t = rm.box_mesh(blo, bhi)
    voxel, band = dx, 7 * dx
    ls_mesh = SparseLevelSet.from_mesh(pol, TriMesh(pol, v, t), voxel, band)
    origin = np.array(ls_mesh.origin)
    n = (np.ceil((v.max(0) + band - origin) / voxel).astype(int) + 1 + 7) // 8 * 8
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), axis=-1)
    x = (np.float32(origin) + np.float32(voxel) * idx.astype(np.float32)).astype(np.float64)
    field = rm.box_sdf(x, v.astype(np.float64).min(0), v.astype(np.float64).max(0))
    ls_dense = SparseLevelSet.from_dense(pol, field, origin, voxel, band)
    keys_d, cells_d = select_blocks(field.astype(np.float32), band, band)
    pert = float(rm.Mesh64(v, t).bound(x.reshape(-1, 3), field.reshape(-1)).max() + 2 * U * np.abs(field).max())
    # the premises, from the reference alone and then cell by cell: no block's membership hangs on the bound, the two level sets store the
    # same blocks, and no cell differs by more than pert
    assert not (np.abs(np.abs(field) - band) <= pert).any()
    assert ls_mesh.keys.tolist() == ls_dense.keys.tolist() == keys_d.tolist()
    dm, dd = ls_mesh.to_dense((0, 0, 0), n)[..., 0].astype(np.float64), ls_dense.to_dense((0, 0, 0), n)[..., 0].astype(np.float64)
    assert (np.abs(dm - dd) <= pert).all()

    class Perturbed(rl.LevelSet64):
        def sample(self, xs):
            val, bb = super().sample(xs)
            bb[:, 0] += pert
            return val, bb
    ref = Perturbed(keys_d, cells_d, np.float32(origin), voxel, band)
    col = make_levelset_collider(ctype)
    before = mt.grid.clone()
    runs = []
    for ls in (ls_dense, ls_mesh):
        mt.grid.copy_(before)
        mt.apply_boundary(col, levelset=ls)
        pol.syncCtx()
        runs.append(mt.grid.cpu().numpy().reshape(mt.nblocks, 7, 512))
    b0 = before.cpu().numpy().reshape(mt.nblocks, 7, 512)
    has = (b0[:, 0] > 0).reshape(-1)
    flat = lambda g: np.ascontiguousarray(g[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    v0 = flat(b0)
    keys = mt.active_keys().astype(np.int64)
    cc = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    xn = (keys[:, None, :] * 8 + cc[None]).reshape(-1, 3).astype(np.float32) * np.float32(dx)     # as the kernels form it
    inside, sd, bsd, want, bv, grad = rl.resolve64(col, ref, xn, v0)
    near = np.abs(sd) <= bsd
    touched = has & (inside | near)
    sel = has & ~near
    share = (has & near).sum() / max(touched.sum(), 1)
    cmp_ = sel & inside
    ratios = [np.abs(flat(g)[cmp_] - want[cmp_]) / bv[cmp_] for g in runs]
    print("MESH boundary type %d: %d nodes touched, %d within the bound of zero left out (share %.2e), pert %.3g, |v - v64| from_dense %.3f "
          "from_mesh %.3f of the bound, gradient >= %.3f, worst |from_mesh - from_dense| %.3g"
          % (ctype, touched.sum(), (has & near).sum(), share, pert, ratios[0].max(), ratios[1].max(), np.nanmin(grad[cmp_]) if ctype else float("nan"),
             np.abs(flat(runs[1])[cmp_] - flat(runs[0])[cmp_]).max()))
    assert touched.sum() > 500 and share <= 0.01
    if ctype:
        # ref64_levelset's normal bound is first order in b_diff / l.  On the box's inner medial planes the trilinear gradient drops to
        # ~0.35 (two faces pull against each other); with b_diff <= 2 pert / (h / 2) ~ 5e-4 the neglected second-order term is
        # (b_diff / l)^2 <= 1e-5 of the normal at l >= 0.25, a few per mille of the first-order bound itself
        assert np.nanmin(grad[cmp_]) >= 0.25
    for g, ratio in zip(runs, ratios):
        assert (ratio <= 1).all()
        assert np.array_equal(flat(g)[sel & ~inside].view(np.uint32), v0[sel & ~inside].view(np.uint32))
        assert np.array_equal(g[:, [0, 4, 5, 6]], b0[:, [0, 4, 5, 6]])


# ------------------------------------------------------------------------------------------------ 6: open meshes, the C++ face
def test_open_mesh_needs_allow_open(pol):
    from zpc_amd.mesh import TriMesh
    from zpc_amd.levelset import SparseLevelSet
    v, t = rm.icosphere(2, 0.31, (0.5, 0.47, 0.53))
    mesh = TriMesh(pol, v, t[1:])
    assert mesh.stats()["boundary_edges"] == 3 and not mesh.is_closed()
    p = _points(v, 2000, 4)
    with pytest.raises(ValueError, match="not closed"):
        mesh.signed_distance(p)
    with pytest.raises(ValueError, match="not closed"):
        SparseLevelSet.from_mesh(pol, mesh, 1.0 / 32, 3.0 / 32)
    sdf, _ = mesh.signed_distance(p, allow_open=True)
    r = rm.Mesh64(v, t[1:]).query(p)
    assert (np.abs(np.abs(sdf.cpu().numpy()) - r["d"]) <= r["b"]).all()
    unsigned, _ = mesh.signed_distance(p, signed=False)
    assert (unsigned >= 0).all()
    assert SparseLevelSet.from_mesh(pol, mesh, 1.0 / 32, 3.0 / 32, allow_open=True).nblocks > 0
    flipped = t.copy()
    flipped[7] = flipped[7, ::-1]
    assert TriMesh(pol, v, flipped).stats()["inconsistent_edges"] == 3
    assert TriMesh(pol, v, np.concatenate([t, t[:1]])).stats()["nonmanifold_edges"] == 3
    with pytest.raises(ValueError, match="indices"):
        TriMesh(pol, v, np.concatenate([t, [[0, 1, len(v)]]]).astype(np.int32))


def test_cpp_face_mesh_view(pol):
    """tests/cpp/test_mesh.hip: TriMeshView::signed_distance / closest_point in a user lambda == the C ABI's bulk entries, bit for bit"""
    exe = os.path.join(ROOT, "zpc_amd", "lib", "test_mesh")
    if not os.path.exists(exe):
        from zpc_amd import build
        build.build_cpp_test("test_mesh")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mesh cpp face ok" in out.stdout
