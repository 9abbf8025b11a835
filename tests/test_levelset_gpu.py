"""Sparse level-set colliders on the GPU (include/zensim_rocm/levelset_device.hpp, zpc_amd/csrc/levelset.hip, zpc_amd/levelset.py):
sampling and resolveCollision against the float64 restatement with per-point bounds (tests/ref64_levelset.py), the two grid passes
against the bulk point entry bit for bit (staged and fallback path), the tie to the analytic plane, the implicit system, the one-call
step, the C++ face and the dense round trip.  Prints one `LEVELSET <what> ...` line per check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref64_levelset as rl
from util import make_cloud, rng

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = rl.U
CENTRE, RADIUS = np.array([0.5, 0.47, 0.53]), 0.3


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


MOVING = dict(s=1.1, dsdt=0.2, R=_rot((0.2, 1.0, 0.4), 0.3), omega=(0.1, -0.3, 0.2), b=(0.05, -0.08, 0.03), dbdt=(0.4, 0.1, -0.2))


def _vel_field(x):
    return np.stack([0.3 * x[..., 1], -0.2 * x[..., 2] + 0.1, 0.25 * x[..., 0]], axis=-1)


def _build(pol, fn, lo, hi, voxel, band, vel=False, background=None):
    """(SparseLevelSet on the device, LevelSet64 of the same float32 cells)"""
    from zpc_amd.levelset import SparseLevelSet, select_blocks
    lo = np.asarray(lo, np.float64)
    n = [int(np.ceil((h - l) / voxel)) + 1 for l, h in zip(lo, hi)]
    x = lo + voxel * np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), axis=-1)
    background = band if background is None else background
    keys, cells = select_blocks(fn(x).astype(np.float32), band, background, _vel_field(x).astype(np.float32) if vel else None)
    ls = SparseLevelSet(pol, keys, cells, lo, voxel, background)
    ref = rl.LevelSet64(keys, cells, np.asarray(lo, np.float32), voxel, background)
    assert np.array_equal(np.array(ls.view.origin[:], np.float32), ref.origin) and np.float32(ls.view.h) == ref.h
    return ls, ref


def _sphere(pol, voxel, vel=False, centre=CENTRE, radius=RADIUS, band=0.1, lo=(-0.2, -0.2, -0.2), hi=(1.2, 1.2, 1.2)):
    """band < radius: the medial point lies outside the band, where the background is positive -- no normal from a zero gradient"""
    return _build(pol, lambda x: np.linalg.norm(x - centre, axis=-1) - radius, lo, hi, voxel, band, vel)


def _bulk_resolve(pol, col, ls, x, v):
    from zpc_amd import lib
    tx, tv = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    ins = torch.full((x.shape[0],), -1, dtype=torch.int32, device="cuda")
    assert lib().zs_rocm_levelset_collider_resolve(pol.handle, C.byref(col), C.byref(ls.view), tx.data_ptr(), tv.data_ptr(), x.shape[0],
                                                   ins.data_ptr()) == 0
    pol.syncCtx()
    return tv.cpu().numpy(), ins.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1: sampling
@pytest.mark.parametrize("voxel", [1.0 / 48, 1.0 / 32, 1.0 / 100])
def test_sampling_against_the_float64_restatement(pol, voxel):
    from zpc_amd import lib
    ls, ref = _sphere(pol, voxel, vel=True)
    g = rng(int(1 / voxel))
    x = np.concatenate([g.random((60000, 3)), 5.0 + g.random((500, 3)), -3.0 - g.random((500, 3))]).astype(np.float32)
    n = x.shape[0]
    tx = torch.from_numpy(x).cuda()
    sd, nn, vm = (torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda"),
                  torch.empty(n, 3, dtype=torch.float32, device="cuda"))
    assert lib().zs_rocm_levelset_sample(pol.handle, C.byref(ls.view), tx.data_ptr(), n, sd.data_ptr(), nn.data_ptr(), vm.data_ptr()) == 0
    only = torch.empty(n, dtype=torch.float32, device="cuda")   # every output may be NULL
    assert lib().zs_rocm_levelset_sample(pol.handle, C.byref(ls.view), tx.data_ptr(), n, only.data_ptr(), None, None) == 0
    pol.syncCtx()
    sd, nn, vm = sd.cpu().numpy(), nn.cpu().numpy(), vm.cpu().numpy()
    assert np.array_equal(only.cpu().numpy().view(np.uint32), sd.view(np.uint32))
    val, b = ref.sample(x)
    r_s = np.abs(sd - val[:, 0]) / b[:, 0]
    r_v = np.abs(vm - val[:, 1:4]) / b[:, 1:4]
    # which points blend the background: some, not all, of the 8 cells of the stencil lie in stored blocks
    X = (x - ref.origin) / ref.h
    base = np.floor(X).astype(np.int64)
    stored = {tuple(k) for k in ls.keys.tolist()}
    cnt = np.zeros(n, int)
    for o in np.ndindex(2, 2, 2):
        blk = (base + np.array(o)) // 8 * 8
        cnt += np.fromiter((tuple(k) in stored for k in blk.tolist()), bool, n)
    blend, outside = (cnt > 0) & (cnt < 8), cnt == 0
    assert blend.sum() > 200 and outside.sum() > 1000 and (cnt == 8).sum() > 10000
    bg = np.float32(ls.background)
    assert (sd[outside].view(np.uint32) == bg.view(np.uint32)).all() and (vm[outside].view(np.uint32) == bg.view(np.uint32)).all()
    nref, bn, l = ref.normal(x)
    ok = l >= 0.5
    r_n = np.abs(nn[ok] - nref[ok]) / bn[ok]
    print("LEVELSET sample h=1/%d: sdf %.3f (blend %.3f) v %.3f normal %.3f of the bound; %d blend, %d outside, %d normals, worst |dsdf| %.3g |dn| %.3g"
          % (round(1 / voxel), r_s.max(), r_s[blend].max(), r_v.max(), r_n.max(), blend.sum(), outside.sum(), ok.sum(),
             np.abs(sd - val[:, 0]).max(), np.abs(nn[ok] - nref[ok]).max()))
    assert ok.sum() > 10000
    assert (r_s <= 1).all() and (r_v <= 1).all() and (r_n <= 1).all()
    # argument checks: refused with nothing written
    bad = type(ls.view).from_buffer_copy(bytes(ls.view))
    bad.h = 0.0
    sent = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    assert lib().zs_rocm_levelset_sample(pol.handle, C.byref(bad), tx.data_ptr(), n, sent.data_ptr(), None, None) == -1
    pol.syncCtx()
    assert (sent == 7.0).all()


# ------------------------------------------------------------------------------------------------ 2: resolveCollision
@pytest.mark.parametrize("config", ["identity", "moving_v"])
@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("voxel", [1.0 / 48, 1.0 / 32, 1.0 / 100])
def test_resolve_collision_against_the_float64_restatement(pol, voxel, ctype, config):
    """the sphere of radius 0.3 at (0.5, 0.47, 0.53) queried at the 65^3 nodes of dx = 1 / 64; identity transform without "v", and a
    moving transform (s, dsdt, a rotation, omega, b, dbdt) with "v".  inside[] equals the restatement's except where |sdf64| is below the
    point's own bound (at most 0.1 % of the points); velocities within their bounds."""
    from zpc_amd.mpm import make_levelset_collider
    ls, ref = _sphere(pol, voxel, vel=config == "moving_v")
    col = make_levelset_collider(ctype, **(MOVING if config == "moving_v" else {}))
    dx = np.float32(1.0 / 64)
    x = (np.stack(np.meshgrid(*[np.arange(65)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32) * dx)
    v0 = rng(5).standard_normal(x.shape).astype(np.float32)
    got, ins = _bulk_resolve(pol, col, ls, x, v0)
    inside, sd, bsd, want, bv, grad = rl.resolve64(col, ref, x, v0)
    near = np.abs(sd) < bsd
    share = near.sum() / x.shape[0]
    keep = ~near
    both = keep & inside
    ratio = np.abs(got[both] - want[both]) / bv[both]
    print("LEVELSET resolve h=1/%d type %d %s: %d inside, %d excluded (share %.2e), v %.3f of the bound, worst |dv| %.3g, gradient >= %.3f"
          % (round(1 / voxel), ctype, config, inside.sum(), near.sum(), share, ratio.max(), np.abs(got[both] - want[both]).max(),
             np.nanmin(grad) if ctype else float("nan")))
    assert share <= 1e-3
    assert np.array_equal(ins[keep] != 0, inside[keep])
    assert inside.sum() > 5000
    assert np.array_equal(got[~inside & keep].view(np.uint32), v0[~inside & keep].view(np.uint32))
    assert (ratio <= 1).all()


# ------------------------------------------------------------------------------------------------ 3: the grid pass
def _partition(pol, side, origin, seed=11):
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(10, dx, 4, seed=seed)
    pos = (pos - pos.mean(0)).astype(np.float32) * np.float32(1.5)
    n = pos.shape[0]
    mt = MpmTransfer(pol, n, dx, dt, model=0, side=side, volume=dx ** 3 / 4, key_is_origin=origin)
    mt.upload(mass, pos, vel, Cm, F)
    mt.build_partition(4096)
    mt.rebin()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    pol.syncCtx()
    return mt, dx


def _node_positions(mt, dx):
    """(float)node * dx of every node, [nblocks * side^3, 3], as the kernels form it"""
    side = mt.side
    keys = mt.active_keys().astype(np.int64) // (side if mt.key_is_origin else 1)
    cc = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    node = keys[:, None, :] * side + cc[None, :, :]
    return (node.reshape(-1, 3).astype(np.float32) * np.float32(dx))


def _expected_from_bulk(pol, mt, dx, col, ls, grid):
    side = mt.side
    g = grid.reshape(mt.nblocks, 7, side ** 3)
    v = np.ascontiguousarray(g[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    res, ins = _bulk_resolve(pol, col, ls, _node_positions(mt, dx), v)
    has = (g[:, 0] > 0).reshape(-1)
    out = np.where(has[:, None], res, v).reshape(mt.nblocks, side ** 3, 3).transpose(0, 2, 1)
    want = g.copy()
    want[:, 1:4] = out
    return want.reshape(grid.shape), has, ins != 0


GRID_CASES = {"staged": dict(voxel=1.0 / 64, move=dict(R=_rot((0, 0, 1), np.radians(10)), b=(0.003, -0.002, 0.001), dbdt=(0.1, 0.0, -0.1))),
              "fallback": dict(voxel=1.0 / 192, move=dict(R=_rot((1, 1, 1), np.radians(60)), b=(0.003, -0.002, 0.001), omega=(0.2, 0.1, -0.3)))}


@pytest.mark.parametrize("path", ["staged", "fallback"])
@pytest.mark.parametrize("ctype", [1, 2])
@pytest.mark.parametrize("side,origin", [(4, False), (8, False), (8, True)])
def test_apply_boundary_levelset_equals_the_bulk_entry_bit_for_bit(pol, side, origin, ctype, path):
    from zpc_amd.mpm import make_levelset_collider
    mt, dx = _partition(pol, side, origin)
    case = GRID_CASES[path]
    ls, _ = _sphere(pol, case["voxel"], vel=True, centre=np.array([0.02, -0.03, 0.01]), radius=0.09, band=0.04, lo=(-0.3,) * 3, hi=(0.3,) * 3)
    ls.enable_stats()
    col = make_levelset_collider(ctype, **case["move"])
    before = mt.grid.cpu().numpy().copy()
    want, has, ins = _expected_from_bulk(pol, mt, dx, col, ls, before)
    mt.apply_boundary(col, levelset=ls)
    stats = ls.read_stats()
    got = mt.grid.cpu().numpy()
    changed = (got != before).reshape(mt.nblocks, 7, side ** 3)
    print("LEVELSET boundary[%s s%d%s type %d]: blocks culled / staged / direct %s of %d, %d nodes inside, %d values changed"
          % (path, side, " origin" if origin else "", ctype, stats[:3].tolist(), mt.nblocks, (ins & has).sum(), changed.sum()))
    assert stats[:3].sum() == mt.nblocks
    if path == "staged":
        assert stats[2] == 0 and stats[1] > 0 and stats[0] > 0
    else:
        assert stats[2] == mt.nblocks
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert changed[:, 1:4].any() and not changed[:, 0].any() and not changed[:, 4:].any()   # only velocities, and some of them
    assert not changed.transpose(0, 2, 1).reshape(-1, 7)[~has].any()                         # nodes without mass are untouched
    assert (ins & has).sum() > 50 and (~ins & has).sum() > 50


# ------------------------------------------------------------------------------------------------ 4: tie to the analytic path
@pytest.mark.parametrize("ctype", [0, 1, 2])
def test_levelset_of_a_plane_reproduces_the_analytic_plane_collider(pol, ctype):
    """a trilinear field of a linear function is exact up to rounding: the level set sampled from a plane gives apply_boundary's result
    with the analytic plane.  Bound per value: the restatement's own b_v for the level-set side and once more for the analytic side's
    roundings (the same operations after the normal), plus 2 |v - v_object| |n_ls - n_plane| for the normal that reaches the response
    (v' = w - (n . w) n is Lipschitz in n with constant 2 |w|), n_ls from the float64 restatement on the stored float32 samples.  Nodes
    whose |sdf64| is below its bound plus the stored samples' rounding may fall on either side (at most 0.1 %)."""
    from zpc_amd.mpm import make_collider, make_levelset_collider, PLANE
    mt, dx = _partition(pol, 8, False, seed=12)
    nrm = np.array([0.36, 0.8, -0.48])
    org = np.array([0.01, -0.02, 0.015])
    dbdt = (0.3, -0.2, 0.1)
    ls, ref = _build(pol, lambda x: ((x - org) * nrm).sum(-1), (-0.3,) * 3, (0.3,) * 3, dx, band=10.0)
    colA = make_collider(PLANE, ctype, tuple(org) + tuple(nrm), dbdt=dbdt)
    colL = make_levelset_collider(ctype, dbdt=dbdt)
    before = mt.grid.clone()
    mt.apply_boundary(colA)
    pol.syncCtx()
    ana = mt.grid.cpu().numpy().reshape(mt.nblocks, 7, 512)
    mt.grid.copy_(before)
    mt.apply_boundary(colL, levelset=ls)
    pol.syncCtx()
    lev = mt.grid.cpu().numpy().reshape(mt.nblocks, 7, 512)
    b0 = before.cpu().numpy().reshape(mt.nblocks, 7, 512)
    has = (b0[:, 0] > 0).reshape(-1)
    x = _node_positions(mt, dx)
    v0 = np.ascontiguousarray(b0[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    inside, sd, bsd, want, bv, grad = rl.resolve64(colL, ref, x, v0)
    va, vl = ana[:, 1:4].transpose(0, 2, 1).reshape(-1, 3), lev[:, 1:4].transpose(0, 2, 1).reshape(-1, 3)
    sample_rounding = U * (np.abs(sd) + 3 * dx)              # the stored float32 samples of the stencil: u |value| each
    near = np.abs(sd) < bsd + sample_rounding
    sel = has & ~near
    share = (has & near).sum() / has.sum()
    nls, _, _ = ref.normal(rl.to_material32(colL, x)[1][sel & inside]) if ctype else (nrm[None, :], None, None)
    w = np.abs(v0[sel & inside].astype(np.float64) - np.array(dbdt)).sum(1)
    bound = 2 * bv[sel & inside] + (2 * w * np.linalg.norm(nls - nrm, axis=-1))[:, None] if ctype else 2 * bv[sel & inside]
    ratio = np.abs(va[sel & inside].astype(np.float64) - vl[sel & inside]) / bound
    print("LEVELSET plane type %d: %d nodes inside, %d near the surface left out (share %.2e), |analytic - level set| %.3f of the bound, worst %.3g"
          % (ctype, (sel & inside).sum(), (has & near).sum(), share, ratio.max(), np.abs(va[sel & inside] - vl[sel & inside]).max()))
    assert share <= 1e-3 and (sel & inside).sum() > 500
    assert (ratio <= 1).all()
    assert np.array_equal(va[sel & ~inside].view(np.uint32), vl[sel & ~inside].view(np.uint32))
    assert np.array_equal(ana[:, [0, 4, 5, 6]], lev[:, [0, 4, 5, 6]])


# ------------------------------------------------------------------------------------------------ 5: the implicit system
def _implicit_setup(pol, side, model=0, **over):
    import test_implicit_gpu as tig
    mt, x, coords, vin, kw = tig._setup(pol, model, side, "lattice", True, with_mass=True, **over)
    c0 = tig.ri.cloud_centre(x)
    ls, _ = _sphere(pol, tig.DX, centre=np.asarray(c0, np.float64), radius=2.5 * tig.DX, band=2.0 * tig.DX,
                    lo=tuple(c0 - 12 * tig.DX), hi=tuple(c0 + 12 * tig.DX))
    pos = np.ascontiguousarray(coords.astype(np.float32) * np.float32(tig.DX))
    return mt, coords, pos, ls, tig


@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("side", [4, 8])
def test_implicit_project_with_a_levelset(pol, side, ctype):
    from zpc_amd.mpm import make_levelset_collider
    mt, coords, pos, ls, tig = _implicit_setup(pol, side)
    col = make_levelset_collider(ctype, dbdt=(0.1, 0.2, -0.1))
    nn = coords.shape[0]
    v0 = rng(77).standard_normal((nn, 3)).astype(np.float32)
    want, ins = _bulk_resolve(pol, col, ls, pos, v0)
    got = torch.from_numpy(v0).cuda()
    mt.implicit_project(col, got, levelset=ls)
    only_zero = torch.from_numpy(v0).cuda()
    mt.implicit_project(None, only_zero)
    pol.syncCtx()
    has = tig._mass(mt) > 0
    got, only_zero = got.cpu().numpy(), only_zero.cpu().numpy()
    assert (ins[has] != 0).sum() > 20 and (ins[has] == 0).sum() > 20
    assert np.array_equal(got[has].view(np.uint32), want[has].view(np.uint32))
    assert (got[~has] == 0).all() and (~has).sum() > 100
    assert np.array_equal(only_zero[has].view(np.uint32), v0[has].view(np.uint32))
    assert (got[has] != v0[has]).any()


@pytest.mark.parametrize("side,binned", [(8, True), (4, True)])
def test_implicit_solve_with_a_sticky_levelset(pol, side, binned):
    """the solve behind one call equals, bit for bit, the same operation sequence (ConjugateGradient.hpp:72-161) driven from Python
    through implicit_multiply, implicit_project(levelset=), implicit_precondition and the dof operators; every inside node with mass
    is left at v_object (0: identity transform, no "v") and every node without mass at 0"""
    from zpc_amd import lib
    from zpc_amd.mpm import make_levelset_collider, STICKY
    mt, coords, pos, ls, tig = _implicit_setup(pol, side)
    col = make_levelset_collider(STICKY)
    nn = coords.shape[0]
    ne = nn * 3
    has = tig._mass(mt) > 0
    _, ins = _bulk_resolve(pol, col, ls, pos, np.zeros((nn, 3), np.float32))
    stuck = has & (ins != 0)
    assert stuck.sum() > 20 and (has & ~stuck).sum() > 100
    b = (rng(31).standard_normal((nn, 3)) * tig._mass(mt)[:, None]).astype(np.float32)
    tb = torch.from_numpy(b).cuda()
    max_iters, tol, rel_tol = 4, 1e-6, 0.5
    tx = mt.dof_vector()
    iters = mt.implicit_solve(tb, tx, max_iters=max_iters, tol=tol, rel_tol=rel_tol, collider=col, levelset=ls, binned=binned)
    pol.syncCtx()
    got = tx.cpu().numpy()
    assert (got[stuck] == 0).all() and (got[~has] == 0).all() and (got[has & ~stuck] != 0).any()
    # the same solve from Python
    L, h = lib(), pol.handle
    x, r, p, q, temp = (mt.dof_vector() for _ in range(5))
    scalar = torch.zeros(1, dtype=torch.float32, device="cuda")

    def dot(a_, b_):
        L.zs_rocm_dof_dot(h, a_.data_ptr(), b_.data_ptr(), ne, scalar.data_ptr())
        pol.syncCtx()
        return np.float32(scalar.item())

    def combine(m, a_, n_, b_, c_):
        L.zs_rocm_dof_linear_combine(h, float(m), a_.data_ptr(), float(n_), b_.data_ptr(), c_.data_ptr(), ne)

    mt.implicit_multiply(x, temp, binned=binned)
    assert L.zs_rocm_dof_compwise(h, 2, tb.data_ptr(), temp.data_ptr(), r.data_ptr(), ne) == 0
    mt.implicit_project(col, r, levelset=ls)
    L.zs_rocm_dof_assign(h, r.data_ptr(), q.data_ptr(), ne)
    mt.implicit_precondition(r, q)
    L.zs_rocm_dof_assign(h, q.data_ptr(), p.data_ptr(), ne)
    zTrk = dot(r, q)
    res = np.sqrt(zTrk)
    local_tol = min(np.float32(rel_tol) * res, np.float32(tol))
    it = 0
    while it != max_iters:
        if res <= local_tol:
            break
        mt.implicit_multiply(p, temp, binned=binned)
        mt.implicit_project(col, temp, levelset=ls)
        alpha = zTrk / dot(temp, p)
        combine(alpha, p, 1.0, x, x)
        combine(-alpha, temp, 1.0, r, r)
        mt.implicit_precondition(r, q)
        last = zTrk
        zTrk = dot(q, r)
        beta = zTrk / last
        combine(beta, p, 1.0, q, p)
        res = np.sqrt(zTrk)
        it += 1
    pol.syncCtx()
    print("LEVELSET solve[s%d %s]: %d iterations, %d stuck nodes" % (side, "binned" if binned else "particle", iters, stuck.sum()))
    assert iters == it and iters >= 2
    # (binned force operator: one workgroup per grid block, no float atomics, so the two runs form the same sums)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), got.view(np.uint32))
    # argument checks: a level set without a collider is refused with nothing written
    sentinel = rng(23).standard_normal((nn, 3)).astype(np.float32)
    ty = torch.from_numpy(sentinel).cuda()
    itv = C.c_int(-7)
    bs, cc, nb = mt._bins(binned)
    rc = L.zs_rocm_mpm_implicit_solve_levelset(h, C.byref(mt.params), mt.particles(), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, bs, cc, nb,
                                               None, C.byref(ls.view), tb.data_ptr(), ty.data_ptr(), 10, 1e-6, 0.5, C.byref(itv))
    rp = L.zs_rocm_mpm_implicit_project_levelset(h, C.byref(mt.params), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, None, C.byref(ls.view),
                                                 ty.data_ptr())
    pol.syncCtx()
    assert rc == -1 and rp == -1 and itv.value == -7
    assert np.array_equal(ty.cpu().numpy().view(np.uint32), sentinel.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 6: the one-call step
def test_step_slotted_with_a_levelset_equals_step_plus_apply_boundary(pol):
    """One particle every third cell, all with the same stencil base offset: the quadratic stencils (3 nodes wide) do not overlap, every
    grid node receives one non-zero contribution, so its sum does not depend on the order of the float atomics and two runs of the step
    give the same bits (asserted on the positions below).  Run A: the
    step with levelset=; run B: the same step without a boundary, then apply_boundary(levelset=)."""
    from zpc_amd.mpm import MpmTransfer, make_levelset_collider, SLIP
    dx, dt = 1.0 / 64, 1e-4
    idx = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    n = idx.shape[0]
    g = rng(41)
    # x / dx - 0.5 in [c + 0.4, c + 0.6] with c = 20 + 3 i: the stencil's base node floor(x / dx - 0.5) is c for every particle (a particle
    # at a cell centre would sit on the edge between two bases, and neighbouring stencils could then share a node)
    pos = ((20 + 3 * idx + 1.0 + 0.2 * (g.random((n, 3)) - 0.5)) * dx).astype(np.float32)
    base = np.floor(pos / np.float32(dx) - np.float32(0.5)).astype(np.int64)
    assert np.array_equal(base, 20 + 3 * idx)   # stencils base .. base + 2 are disjoint, and 0.3 dt / dx = 0.002 cell of motion keeps them so
    vel = (0.3 * g.standard_normal((n, 3))).astype(np.float32)
    mass = np.full(n, 1e-3, np.float32) * (1 + g.random(n).astype(np.float32))
    Cm = np.zeros((n, 9), np.float32)
    F = np.tile(np.eye(3, dtype=np.float32).reshape(-1), (n, 1))
    centre = pos.astype(np.float64).mean(0)
    ls, _ = _sphere(pol, dx, vel=True, centre=centre, radius=8 * dx, band=4 * dx, lo=tuple(centre - 24 * dx), hi=tuple(centre + 24 * dx))
    ls.enable_stats()
    col = make_levelset_collider(SLIP, dbdt=(0.05, 0.0, -0.02))
    grids = []
    for with_ls in (True, False):
        mt = MpmTransfer(pol, n, dx, dt, model=0, side=8, volume=dx ** 3 / 8, cache_stress=True)
        mt.upload(mass, pos, vel, Cm, F)
        mt.build_partition(n, margin=1)
        mt.rebin()
        mt.update_stress()
        mt.clear_grid()
        mt.p2g()
        mt.grid_update((0.0, -9.8, 0.0))
        mt.slot(K=24, outbox_cap=512)
        if with_ls:
            mt.step_slotted((0.0, -9.8, 0.0), collider=col, levelset=ls)
            stats = ls.read_stats()
        else:
            mt.step_slotted((0.0, -9.8, 0.0))
            pol.syncCtx()
            plain = mt.grid_by_key()
            mt.apply_boundary(col, levelset=ls)
        pol.syncCtx()
        grids.append(mt.grid_by_key())   # (block numbers come from an atomic counter: the two partitions are compared key by key)
        nblocks = mt.nblocks
    assert sorted(grids[0]) == sorted(grids[1]) == sorted(plain)
    keys = sorted(grids[0])
    grids = [np.stack([g[k] for k in keys]) for g in grids]
    plain = np.stack([plain[k] for k in keys])
    changed = (grids[1] != plain).sum()
    differ = grids[0].view(np.uint32) != grids[1].view(np.uint32)
    print("LEVELSET step: %d values differ between the two runs, worst %.3g" % (differ.sum(), np.abs(grids[0] - grids[1]).max()))
    print("LEVELSET step: %d blocks, culled / staged / direct in the step %s, the boundary changed %d values" % (nblocks, stats[:3].tolist(), changed))
    assert stats[:3].sum() == nblocks and stats[1] > 0
    assert changed > 30
    assert np.array_equal(grids[0].view(np.uint32), grids[1].view(np.uint32))
    # a level set without a collider is refused before anything runs
    before = mt.grid.clone()
    with pytest.raises(RuntimeError):
        mt.step_slotted((0.0, -9.8, 0.0), levelset=ls)
    pol.syncCtx()
    assert torch.equal(before.view(torch.int32), mt.grid.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 7: the C++ face
def test_cpp_face_levelset_collider_program_runs():
    """tests/cpp/test_levelset.hip: Collider{sparseGridView, type}.resolveCollision in a user lambda == the C ABI's bulk entry, bit for bit"""
    exe = os.path.join(ROOT, "zpc_amd", "lib", "test_levelset")
    if not os.path.exists(exe):
        from zpc_amd import build
        build.build_cpp_test("test_levelset")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    print(r.stdout.decode()[-1500:])
    assert r.returncode == 0 and b"levelset cpp face ok: 0 mismatches" in r.stdout, r.stdout.decode()[-3000:]


# ------------------------------------------------------------------------------------------------ 8: round trip
@pytest.mark.parametrize("vel", [False, True])
def test_from_dense_to_dense_round_trip(pol, vel):
    from zpc_amd.levelset import SparseLevelSet, select_blocks
    g = rng(9)
    shape = (37, 20, 26)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), axis=-1).astype(np.float64)
    sdf = (np.linalg.norm(idx - np.array([18.0, 9.0, 12.0]), axis=-1) - 7.0 + 0.01 * g.standard_normal(shape)).astype(np.float32)
    vv = g.standard_normal(shape + (3,)).astype(np.float32) if vel else None
    band, bg = 2.0, 3.5
    ls = SparseLevelSet.from_dense(pol, torch.from_numpy(sdf), (0.1, 0.2, 0.3), 0.05, band, vel=vv, background=bg)
    keys, _ = select_blocks(sdf, band, bg, vv)
    assert np.array_equal(ls.keys, keys) and 0 < ls.nblocks < 5 * 3 * 4
    lo, hi = (-8, -3, -8), (48, 27, 35)
    out = ls.to_dense(lo, hi)
    want = np.full(out.shape, np.float32(bg), np.float32)
    full = np.concatenate([sdf[..., None]] + ([vv] if vel else []), axis=-1)
    pad = np.full((40, 24, 32, full.shape[-1]), np.float32(bg), np.float32)
    pad[:37, :20, :26] = full
    for k in keys:
        want[k[0] + 8:k[0] + 16, k[1] + 3:k[1] + 11, k[2] + 8:k[2] + 16] = pad[k[0]:k[0] + 8, k[1]:k[1] + 8, k[2]:k[2] + 8]
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert (out[..., 0] != np.float32(bg)).sum() == (want[..., 0] != np.float32(bg)).sum() > 1000
    d = SparseLevelSet.from_dense(pol, sdf, (0, 0, 0), 0.05, band)
    assert d.background == band and not d.has_velocity
    f = SparseLevelSet.from_function(pol, lambda x: np.linalg.norm(x - 0.5, axis=-1) - 0.3, (0, 0, 0), (1, 1, 1), 1.0 / 16, 0.1)
    c = f.to_dense((0, 0, 0), (17, 17, 17))[..., 0]
    near = np.abs(c) < 0.1
    xs = np.stack(np.meshgrid(*[np.arange(17)] * 3, indexing="ij"), axis=-1) / 16.0
    assert near.sum() > 100 and np.allclose(c[near], (np.linalg.norm(xs - 0.5, axis=-1) - 0.3)[near], atol=1e-6)
