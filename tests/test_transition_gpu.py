"""Keyframed level-set colliders on the GPU (TransitionLevelSetView in include/zensim_rocm/levelset_device.hpp,
zpc_amd/csrc/levelset_transition.hip, zpc_amd.levelset.LevelSetSequence): the bulk point entries against the float64 restatement with
per-point bounds (tests/ref64_transition.py), the degenerate cases and the block kernels bit for bit, the speed reduction, the implicit
solve, the one-call step, the argument checks and the C++ face.  Prints one `TRANSITION <what> ...` line per check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref64_levelset as rl
import ref64_transition as rt
from util import rng

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tlg():
    import test_levelset_gpu as tlg   # its partition, node-position and sphere helpers, and the MOVING parameters
    return tlg


def _upload(pol, frame):
    from zpc_amd.levelset import SparseLevelSet
    keys, cells, origin = frame
    ls = SparseLevelSet(pol, keys, cells, origin, rt.VOXEL, rt.BAND)
    ls.band = rt.BAND
    return ls


def _sequence(pol, levelsets, alpha, step_dt=rt.STEP_DT):
    from zpc_amd.levelset import LevelSetSequence
    seq = LevelSetSequence(pol, step_dt)
    for ls in levelsets:
        seq.push(ls)
    seq.advance(alpha)
    assert float(seq.alpha) == alpha and len(seq) == len(levelsets)
    return seq


def _copy(view, **over):
    v = type(view).from_buffer_copy(bytes(view))
    for k, val in over.items():
        setattr(v, k, val)
    return v


def _sample(pol, entry, view, x):
    n = x.shape[0]
    tx = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    sd, nn, vm = (torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, 3, dtype=torch.float32, device="cuda"),
                  torch.empty(n, 3, dtype=torch.float32, device="cuda"))
    assert entry(pol.handle, C.byref(view), tx.data_ptr(), n, sd.data_ptr(), nn.data_ptr(), vm.data_ptr()) == 0
    pol.syncCtx()
    return sd.cpu().numpy(), nn.cpu().numpy(), vm.cpu().numpy()


def _resolve(pol, entry, col, view, x, v):
    tx, tv = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    ins = torch.full((x.shape[0],), -1, dtype=torch.int32, device="cuda")
    assert entry(pol.handle, C.byref(col), C.byref(view), tx.data_ptr(), tv.data_ptr(), x.shape[0], ins.data_ptr()) == 0
    pol.syncCtx()
    return tv.cpu().numpy(), ins.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def frames():
    """the keyframes of the issue's case, computed once: {(vel_src, vel_dst): [(keys, cells, origin)] * 2}"""
    return {k: rt.keyframes(*k) for k in ((True, True), (False, True), (False, False))}


# ------------------------------------------------------------------------------------------------ 1: the bulk entries
def _check_sample(pol, frames2, alpha):
    from zpc_amd import lib
    seq = _sequence(pol, [_upload(pol, f) for f in frames2], alpha)
    ref = rt.reference(frames2, alpha)
    x = rt.material_points(alpha).astype(np.float32)
    sd, nn, vm = _sample(pol, lib().zs_rocm_levelset_transition_sample, seq.view(), x)
    ws, bs = ref.sdf(x)
    wv, bv = ref.velocity(x)
    wn, bn, l = ref.normal(x)
    ok = l >= 0.5
    r_s, r_v, r_n = np.abs(sd - ws) / bs, np.abs(vm - wv) / bv, np.abs(nn[ok] - wn[ok]) / bn[ok]
    print("TRANSITION sample alpha=%g: sdf %.3f v %.3f normal %.3f of the bound; %d of %d normals, worst |dsdf| %.3g |dn| %.3g"
          % (alpha, r_s.max(), r_v.max(), r_n.max(), ok.sum(), x.shape[0], np.abs(sd - ws).max(), np.abs(nn[ok] - wn[ok]).max()))
    assert ok.mean() >= 0.99
    assert (r_s <= 1).all() and (r_v <= 1).all() and (r_n <= 1).all()


@pytest.mark.parametrize("alpha", rt.ALPHAS)
def test_transition_sample_against_the_float64_restatement(pol, frames, alpha):
    _check_sample(pol, frames[(True, True)], alpha)


@pytest.mark.parametrize("config", ["identity", "moving"])
@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("alpha", rt.ALPHAS)
def test_transition_resolve_against_the_float64_restatement(pol, frames, alpha, ctype, config):
    """4096 points within 2 voxels of the interpolated sphere, in material space, mapped to the world through the collider's transform;
    inside[] equals the restatement's except where |sdf64| is below the point's own bound, velocities within their bounds; points with a
    per-keyframe gradient length below 0.5 (at most 1 %) are left out for the types that use the normal"""
    from zpc_amd import lib
    from zpc_amd.mpm import make_levelset_collider
    tlg = _tlg()
    move = tlg.MOVING if config == "moving" else {}
    col = make_levelset_collider(ctype, **move)
    X = rt.material_points(alpha)
    if move:
        X = float(np.float32(move["s"])) * X @ np.asarray(move["R"], np.float32).astype(np.float64).T + np.asarray(move["b"], np.float32)
    x = X.astype(np.float32)
    v0 = rng(5).standard_normal(x.shape).astype(np.float32)
    f2 = frames[(True, True)]
    seq = _sequence(pol, [_upload(pol, f) for f in f2], alpha)
    got, ins = _resolve(pol, lib().zs_rocm_levelset_transition_collider_resolve, col, seq.view(), x, v0)
    inside, sd, bsd, want, bv, grad = rl.resolve64(col, rt.reference(f2, alpha), x, v0)
    near = np.abs(sd) < bsd
    keep = ~near
    flat = inside & (grad < 0.5) if ctype else np.zeros_like(inside)
    both = keep & inside & ~flat
    ratio = np.abs(got[both] - want[both]) / bv[both]
    print("TRANSITION resolve alpha=%g type %d %s: %d inside, %d near the surface, %d flat, v %.3f of the bound, worst |dv| %.3g"
          % (alpha, ctype, config, inside.sum(), near.sum(), flat.sum(), ratio.max(), np.abs(got[both] - want[both]).max()))
    assert near.mean() <= 1e-3 and flat.sum() <= 0.01 * inside.sum()
    assert np.array_equal(ins[keep] != 0, inside[keep])
    assert inside.sum() > 1000 and (~inside).sum() > 1000
    assert np.array_equal(_bits(got[~inside & keep]), _bits(v0[~inside & keep]))
    assert (ratio <= 1).all()


# ------------------------------------------------------------------------------------------------ 2: degenerate cases
@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_one_keyframe_without_velocity_equals_the_single_level_set(pol, frames, alpha):
    """src is dst and no "v": x0 = x1 = x, and (1 - alpha) a + alpha a is a itself for alpha = 0 (a + 0) and alpha = 0.5 (a / 2 twice,
    exact): the bits of zs_rocm_levelset_sample and zs_rocm_levelset_collider_resolve"""
    from zpc_amd import lib
    from zpc_amd.mpm import make_levelset_collider
    ls = _upload(pol, frames[(False, False)][0])
    seq = _sequence(pol, [ls], alpha)
    view = seq.view()
    assert bytes(view.src)[:C.sizeof(type(view.src)) - 8] == bytes(view.dst)[:C.sizeof(type(view.dst)) - 8]   # (all but `stats`)
    x = rt.material_points(0.0, seed=1).astype(np.float32)
    a = _sample(pol, lib().zs_rocm_levelset_transition_sample, view, x)
    b = _sample(pol, lib().zs_rocm_levelset_sample, ls.view, x)
    for p, q in zip(a, b):
        assert np.array_equal(_bits(p), _bits(q))
    assert (a[0] < 0).sum() > 1000 and (a[2] == 0).all()
    tlg = _tlg()
    for ctype in (0, 1, 2):
        col = make_levelset_collider(ctype, **tlg.MOVING)
        X = float(np.float32(tlg.MOVING["s"])) * rt.material_points(0.0, seed=1) @ np.asarray(tlg.MOVING["R"]).T + np.asarray(tlg.MOVING["b"])
        xw = X.astype(np.float32)
        v0 = rng(6).standard_normal(xw.shape).astype(np.float32)
        ga, ia = _resolve(pol, lib().zs_rocm_levelset_transition_collider_resolve, col, view, xw, v0)
        gb, ib = _resolve(pol, lib().zs_rocm_levelset_collider_resolve, col, ls.view, xw, v0)
        assert np.array_equal(ia, ib) and np.array_equal(_bits(ga), _bits(gb)) and (ia != 0).sum() > 1000


def test_alpha_zero_equals_the_source_keyframe(pol, frames):
    """alpha = 0 with "v": x0 = x - 0 v = x, and 1 a + 0 b = a for finite b: src alone, bit for bit"""
    from zpc_amd import lib
    from zpc_amd.mpm import make_levelset_collider
    lss = [_upload(pol, f) for f in frames[(True, True)]]
    view = _sequence(pol, lss, 0.0).view()
    x = rt.material_points(0.0, seed=2).astype(np.float32)
    a = _sample(pol, lib().zs_rocm_levelset_transition_sample, view, x)
    b = _sample(pol, lib().zs_rocm_levelset_sample, lss[0].view, x)
    c = _sample(pol, lib().zs_rocm_levelset_sample, lss[1].view, x)
    for p, q in zip(a, b):
        assert np.array_equal(_bits(p), _bits(q))
    assert not np.array_equal(_bits(b[0]), _bits(c[0]))
    v0 = rng(7).standard_normal(x.shape).astype(np.float32)
    for ctype in (0, 1, 2):
        col = make_levelset_collider(ctype, dbdt=(0.1, 0.0, -0.2))
        ga, ia = _resolve(pol, lib().zs_rocm_levelset_transition_collider_resolve, col, view, x, v0)
        gb, ib = _resolve(pol, lib().zs_rocm_levelset_collider_resolve, col, lss[0].view, x, v0)
        assert np.array_equal(ia, ib) and np.array_equal(_bits(ga), _bits(gb)) and (ia != 0).sum() > 1000


@pytest.mark.parametrize("alpha", [0.25, 0.96875])
def test_a_keyframe_without_velocity_contributes_zero(pol, frames, alpha):
    """src without "v": its term of v and of the velocity blend is 0 -- against the restatement, which forms the formula that way"""
    _check_sample(pol, frames[(False, True)], alpha)


# ------------------------------------------------------------------------------------------------ 3: the block kernels
BLOCK_CASES = {
    # 10 degrees, h = dx: side 4 stages all four channels of both level sets, side 8 both sdf boxes and the "v" box of src only
    "staged": dict(voxel=1.0 / 64, centre=(0.02, -0.03, 0.01), lo=-0.3, hi=0.3, move=dict(b=(0.003, -0.002, 0.001), dbdt=(0.1, 0.0, -0.1)),
                   angle=(0, 0, 1, 10)),
    # no rotation, h = dx: 13^3 cells per level set at the smallest widening -- with maxSpeed = 0 all eight boxes fit, also for side 8
    "aligned": dict(voxel=1.0 / 64, centre=(0.02, -0.03, 0.01), lo=-0.3, hi=0.3, move=dict(b=(0.003, -0.002, 0.001), dbdt=(0.1, 0.0, -0.1)),
                    angle=(0, 0, 1, 0)),
    # h = dx / 4 under 60 degrees about (1, 1, 1): footprints of 25 cells and more per axis, over the budget
    "direct": dict(voxel=1.0 / 256, centre=(0.02, -0.03, 0.01), lo=-0.2, hi=0.2, move=dict(b=(0.003, -0.002, 0.001), omega=(0.2, 0.1, -0.3)),
                   angle=(1, 1, 1, 60)),
    # a collider two units away from every block (its "v" is larger out there: a shorter keyframe spacing keeps the sdf boxes in budget)
    "culled": dict(step_dt=0.02, voxel=1.0 / 64, centre=(2.0, 2.0, 2.0), lo=1.7, hi=2.3, move=dict(dbdt=(0.1, 0.0, -0.1)), angle=(0, 0, 1, 10)),
}


@pytest.mark.parametrize("path", ["staged", "aligned", "direct", "culled"])
@pytest.mark.parametrize("side,origin", [(4, False), (8, False), (8, True)])
def test_block_kernels_equal_the_bulk_entry_bit_for_bit(pol, side, origin, path):
    """apply_boundary and implicit_project with a sequence on a partition of a few dozen blocks: every node with mass gets the bits of
    zs_rocm_levelset_transition_collider_resolve at its position; stats show the path; maxSpeed = 0 (narrower staged boxes, the
    displaced reads fall outside and go to the grid) gives the same bits"""
    from zpc_amd import lib
    from zpc_amd.mpm import make_levelset_collider, SLIP
    tlg = _tlg()
    mt, dx = tlg._partition(pol, side, origin)
    case = BLOCK_CASES[path]
    c0 = np.array(case["centre"])
    kw = dict(vel=True, radius=0.09, band=0.04, lo=(case["lo"],) * 3, hi=(case["hi"],) * 3)
    lss = [tlg._sphere(pol, case["voxel"], centre=c, **kw)[0] for c in (c0, c0 + np.array([0.6, -0.48, 0.64]) / 64)]
    seq = _sequence(pol, lss, 0.25, step_dt=case.get("step_dt", 0.1))
    seq.enable_stats()
    ax = case["angle"]
    col = make_levelset_collider(SLIP, R=tlg._rot(ax[:3], np.radians(ax[3])), **case["move"])
    view = seq.view()
    assert view.maxSpeed > 0.1 and view.stepDt * 0.75 * view.maxSpeed / view.src.h > 0.5      # the widening is at work
    nodes = tlg._node_positions(mt, dx)
    before = mt.grid.cpu().numpy().copy()
    g = before.reshape(mt.nblocks, 7, side ** 3)
    has = (g[:, 0] > 0).reshape(-1)
    v = np.ascontiguousarray(g[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    res, ins = _resolve(pol, lib().zs_rocm_levelset_transition_collider_resolve, col, view, nodes, v)
    want = g.copy()
    want[:, 1:4] = np.where(has[:, None], res, v).reshape(mt.nblocks, side ** 3, 3).transpose(0, 2, 1)
    want = want.reshape(before.shape)
    dof0 = rng(3).standard_normal((nodes.shape[0], 3)).astype(np.float32)
    pres, _ = _resolve(pol, lib().zs_rocm_levelset_transition_collider_resolve, col, view, nodes, dof0)
    pwant = np.where(has[:, None], pres, np.float32(0))
    results = []
    for lev in (seq, _copy(view, maxSpeed=0.0)):
        mt.grid.copy_(torch.from_numpy(before).cuda())
        dof = torch.from_numpy(dof0).cuda()
        mt.implicit_project(col, dof, levelset=lev)
        mt.apply_boundary(col, levelset=lev)
        stats = seq.read_stats()
        results.append((mt.grid.cpu().numpy(), dof.cpu().numpy(), stats))
    (got, pgot, stats), (got0, pgot0, stats0) = results
    inside = (ins != 0) & has
    print("TRANSITION blocks[%s s%d%s]: culled / staged / direct / v-direct %s (maxSpeed 0: %s) of 2 x %d, %d nodes inside"
          % (path, side, " origin" if origin else "", stats.tolist(), stats0.tolist(), mt.nblocks, inside.sum()))
    assert stats[:3].sum() == 2 * mt.nblocks and stats0[:3].sum() == 2 * mt.nblocks
    if path in ("staged", "aligned"):
        assert stats[2] == 0 and stats[1] > 0 and stats[0] > 0
        assert stats[3] == (0 if side == 4 else stats[1])      # side 8: a "v" box of 15^3 or 16^3 cells no longer fits next to the rest
        if path == "aligned":
            assert stats0[1] > 0 and stats0[3] == 0            # 13^3 cells: everything from LDS
        assert inside.sum() > 50 and (~(ins != 0) & has).sum() > 50
    elif path == "direct":
        assert stats[2] == 2 * mt.nblocks and inside.sum() > 50
    else:
        assert stats[0] == 2 * mt.nblocks and inside.sum() == 0
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(pgot), _bits(pwant))
    assert np.array_equal(_bits(got0), _bits(got)) and np.array_equal(_bits(pgot0), _bits(pgot))
    assert (got != before).any() == (path != "culled")


# ------------------------------------------------------------------------------------------------ 4: max_speed
def test_max_speed_is_the_largest_velocity_component_of_the_stored_cells(pol):
    from zpc_amd.levelset import SparseLevelSet, select_blocks
    g = rng(17)
    shape = (40, 33, 27)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), axis=-1).astype(np.float64)
    sdf = (np.linalg.norm(idx - np.array([19.0, 15.0, 12.0]), axis=-1) - 9.0).astype(np.float32)
    vel = g.standard_normal(shape + (3,)).astype(np.float32)
    vel[20, 9, 4, 1] = -7.25          # the largest magnitude is a negative component inside the band (|sdf| = 1.77)
    keys, cells = select_blocks(sdf, 2.0, 3.0, vel)
    ls = SparseLevelSet(pol, keys, cells, (0, 0, 0), 0.05, 3.0)
    want = np.abs(cells[:, 1:4]).max()
    assert ls.nblocks > 10 and want == np.float32(7.25)
    assert np.float32(ls.max_speed()) == want
    plain = SparseLevelSet(pol, *select_blocks(sdf, 2.0, 3.0), (0, 0, 0), 0.05, 3.0)
    assert plain.max_speed() == 0.0
    assert SparseLevelSet(pol, np.zeros((0, 3), np.int32), np.zeros((0, 4), np.float32), (0, 0, 0), 0.05, 3.0).max_speed() == 0.0


# ------------------------------------------------------------------------------------------------ 5: the implicit solve
@pytest.mark.parametrize("side", [8, 4])
def test_implicit_solve_with_a_sticky_sequence(pol, side):
    """the shape of test_implicit_solve_with_a_sticky_levelset: the solve behind one call equals, bit for bit and in its iteration
    count, the same operation sequence driven from Python through implicit_multiply, implicit_project(levelset=sequence),
    implicit_precondition and the dof operators"""
    from zpc_amd import lib
    from zpc_amd.mpm import make_levelset_collider, STICKY
    import test_implicit_gpu as tig
    tlg = _tlg()
    mt, x, coords, vin, kw = tig._setup(pol, 0, side, "lattice", True, with_mass=True)
    c0 = np.asarray(tig.ri.cloud_centre(x), np.float64)
    lss = [tlg._sphere(pol, tig.DX, centre=c, radius=2.5 * tig.DX, band=2.0 * tig.DX, lo=tuple(c0 - 12 * tig.DX),
                       hi=tuple(c0 + 12 * tig.DX))[0] for c in (c0, c0 + np.array([0.6, -0.48, 0.64]) * tig.DX)]
    seq = _sequence(pol, lss, 0.25)
    col = make_levelset_collider(STICKY)
    pos = np.ascontiguousarray(coords.astype(np.float32) * np.float32(tig.DX))
    nn = coords.shape[0]
    ne = nn * 3
    has = tig._mass(mt) > 0
    _, ins = _resolve(pol, lib().zs_rocm_levelset_transition_collider_resolve, col, seq.view(), pos, np.zeros((nn, 3), np.float32))
    stuck = has & (ins != 0)
    assert stuck.sum() > 20 and (has & ~stuck).sum() > 100
    b = (rng(31).standard_normal((nn, 3)) * tig._mass(mt)[:, None]).astype(np.float32)
    tb = torch.from_numpy(b).cuda()
    max_iters, tol, rel_tol = 4, 1e-6, 0.5
    tx = mt.dof_vector()
    iters = mt.implicit_solve(tb, tx, max_iters=max_iters, tol=tol, rel_tol=rel_tol, collider=col, levelset=seq, binned=True)
    pol.syncCtx()
    got = tx.cpu().numpy()
    assert (got[stuck] == 0).all() and (got[~has] == 0).all() and (got[has & ~stuck] != 0).any()
    L, h = lib(), pol.handle
    xv, r, p, q, temp = (mt.dof_vector() for _ in range(5))
    scalar = torch.zeros(1, dtype=torch.float32, device="cuda")

    def dot(a_, b_):
        L.zs_rocm_dof_dot(h, a_.data_ptr(), b_.data_ptr(), ne, scalar.data_ptr())
        pol.syncCtx()
        return np.float32(scalar.item())

    def combine(m, a_, n_, b_, c_):
        L.zs_rocm_dof_linear_combine(h, float(m), a_.data_ptr(), float(n_), b_.data_ptr(), c_.data_ptr(), ne)

    mt.implicit_multiply(xv, temp, binned=True)
    assert L.zs_rocm_dof_compwise(h, 2, tb.data_ptr(), temp.data_ptr(), r.data_ptr(), ne) == 0
    mt.implicit_project(col, r, levelset=seq)
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
        mt.implicit_multiply(p, temp, binned=True)
        mt.implicit_project(col, temp, levelset=seq)
        alpha = zTrk / dot(temp, p)
        combine(alpha, p, 1.0, xv, xv)
        combine(-alpha, temp, 1.0, r, r)
        mt.implicit_precondition(r, q)
        last = zTrk
        zTrk = dot(q, r)
        beta = zTrk / last
        combine(beta, p, 1.0, q, p)
        res = np.sqrt(zTrk)
        it += 1
    pol.syncCtx()
    print("TRANSITION solve[s%d]: %d iterations, %d stuck nodes" % (side, iters, stuck.sum()))
    assert iters == it and iters >= 2
    assert np.array_equal(_bits(xv.cpu().numpy()), _bits(got))


# ------------------------------------------------------------------------------------------------ 6: the one-call step
def test_step_slotted_with_a_sequence_equals_step_plus_apply_boundary(pol):
    """the particle layout of test_step_slotted_with_a_levelset_equals_step_plus_apply_boundary (disjoint stencils: the float atomics'
    order does not reach the sums), 13^3 particles.  Run A: step_slotted(levelset=sequence); run B: the step without a boundary, then
    apply_boundary(sequence); run C: run A after the sequence has advanced across a keyframe pop -- another pair of keyframes, another
    grid."""
    from zpc_amd.mpm import MpmTransfer, make_levelset_collider, SLIP
    tlg = _tlg()
    dx, dt = 1.0 / 64, 1e-4
    idx = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    n = idx.shape[0]
    g = rng(41)
    pos = ((8 + 3 * idx + 1.0 + 0.2 * (g.random((n, 3)) - 0.5)) * dx).astype(np.float32)
    assert np.array_equal(np.floor(pos / np.float32(dx) - np.float32(0.5)).astype(np.int64), 8 + 3 * idx)
    vel = (0.3 * g.standard_normal((n, 3))).astype(np.float32)
    mass = np.full(n, 1e-3, np.float32) * (1 + g.random(n).astype(np.float32))
    Cm = np.zeros((n, 9), np.float32)
    F = np.tile(np.eye(3, dtype=np.float32).reshape(-1), (n, 1))
    centre = pos.astype(np.float64).mean(0)
    shift = np.array([0.6, -0.48, 0.64]) * dx
    lss = [tlg._sphere(pol, dx, vel=True, centre=centre + k * shift, radius=8 * dx, band=4 * dx, lo=tuple(centre - 24 * dx),
                       hi=tuple(centre + 24 * dx))[0] for k in range(3)]
    col = make_levelset_collider(SLIP, dbdt=(0.05, 0.0, -0.02))
    grids = {}
    for run in "ABC":
        seq = _sequence(pol, lss, 0.25, step_dt=0.05)
        if run == "C":
            seq.advance(1.0)
            assert len(seq) == 2 and float(seq.alpha) == 0.25
        mt = MpmTransfer(pol, n, dx, dt, model=0, side=8, volume=dx ** 3 / 8, cache_stress=True)
        mt.upload(mass, pos, vel, Cm, F)
        mt.build_partition(n, margin=1)
        mt.rebin()
        mt.update_stress()
        mt.clear_grid()
        mt.p2g()
        mt.grid_update((0.0, -9.8, 0.0))
        mt.slot(K=24, outbox_cap=512)
        if run == "B":
            mt.step_slotted((0.0, -9.8, 0.0))
            pol.syncCtx()
            plain = mt.grid_by_key()
            mt.apply_boundary(col, levelset=seq)
        else:
            mt.step_slotted((0.0, -9.8, 0.0), collider=col, levelset=seq)
        pol.syncCtx()
        grids[run] = mt.grid_by_key()
    keys = sorted(grids["A"])
    assert keys == sorted(grids["B"]) == sorted(grids["C"]) == sorted(plain)
    A, B, Cg, P = (np.stack([d[k] for k in keys]) for d in (grids["A"], grids["B"], grids["C"], plain))
    print("TRANSITION step: %d blocks, the boundary changed %d values, the pop changed %d values"
          % (len(keys), (B != P).sum(), (Cg != A).sum()))
    assert (B != P).sum() > 30
    assert np.array_equal(_bits(A), _bits(B))
    assert (Cg != A).sum() > 30
    with pytest.raises(RuntimeError):
        mt.step_slotted((0.0, -9.8, 0.0), levelset=seq)      # a sequence without a collider is refused before anything runs


# ------------------------------------------------------------------------------------------------ 7: argument checks
def test_invalid_arguments_are_refused_with_nothing_written(pol, frames):
    from zpc_amd import lib
    from zpc_amd.mpm import make_levelset_collider, SLIP
    import test_implicit_gpu as tig
    L, h = lib(), pol.handle
    lss = [_upload(pol, f) for f in frames[(True, True)]]
    good = _sequence(pol, lss, 0.25).view()
    bad_ls = _copy(lss[0].view, h=0.0)
    nan, inf = float("nan"), float("inf")
    bad = {"src": _copy(good, src=bad_ls), "dst": _copy(good, dst=bad_ls)}
    for name, vals in (("alpha", (-0.125, 1.5, nan)), ("stepDt", (-1.0, inf, nan)), ("maxSpeed", (-1.0, inf, nan))):
        for k, val in enumerate(vals):
            bad["%s%d" % (name, k)] = _copy(good, **{name: val})
    col = make_levelset_collider(SLIP)
    mt, xs, coords, vin, kw = tig._setup(pol, 0, 4, "lattice", True, with_mass=True)
    n = 256
    x = torch.from_numpy(rt.material_points(0.25)[:n].astype(np.float32)).cuda()
    sent = lambda *shape: torch.full(shape, 7.0, dtype=torch.float32, device="cuda")
    out = sent(n, 7)
    word = sent(1)
    assert L.zs_rocm_levelset_max_speed(h, C.byref(bad_ls), word.data_ptr()) == -1
    assert L.zs_rocm_levelset_max_speed(h, C.byref(lss[0].view), None) == -1
    grid0 = mt.grid.clone()
    dof, b = sent(mt.nblocks * 64, 3), sent(mt.nblocks * 64, 3)
    bs, cc, nb = mt._bins(True)
    itv = C.c_int(-7)
    for name, t in bad.items():
        rc = [L.zs_rocm_levelset_transition_sample(h, C.byref(t), x.data_ptr(), n, out.data_ptr(), out.data_ptr() + 4 * n, out.data_ptr() + 16 * n),
              L.zs_rocm_levelset_transition_collider_resolve(h, C.byref(col), C.byref(t), x.data_ptr(), out.data_ptr(), n, None),
              L.zs_rocm_mpm_apply_boundary_transition(h, C.byref(mt.params), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, C.byref(col), C.byref(t)),
              L.zs_rocm_mpm_implicit_project_transition(h, C.byref(mt.params), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, C.byref(col),
                                                        C.byref(t), dof.data_ptr()),
              L.zs_rocm_mpm_implicit_solve_transition(h, C.byref(mt.params), mt.particles(), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, bs, cc,
                                                      nb, C.byref(col), C.byref(t), b.data_ptr(), dof.data_ptr(), 10, 1e-6, 0.5, C.byref(itv))]
        assert rc == [-1] * 5, (name, rc)
    # a transition without a collider, and no transition at all
    assert L.zs_rocm_levelset_transition_collider_resolve(h, None, C.byref(good), x.data_ptr(), out.data_ptr(), n, None) == -1
    assert L.zs_rocm_mpm_apply_boundary_transition(h, C.byref(mt.params), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, None, C.byref(good)) == -1
    assert L.zs_rocm_mpm_implicit_project_transition(h, C.byref(mt.params), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, C.byref(col), None,
                                                     dof.data_ptr()) == -1
    assert L.zs_rocm_mpm_implicit_solve_transition(h, C.byref(mt.params), mt.particles(), mt.table.handle, mt.grid.data_ptr(), mt.nblocks, bs, cc,
                                                   nb, None, C.byref(good), b.data_ptr(), dof.data_ptr(), 10, 1e-6, 0.5, C.byref(itv)) == -1
    pol.syncCtx()
    assert (out == 7.0).all() and (word == 7.0).all() and (dof == 7.0).all() and itv.value == -7
    assert torch.equal(grid0.view(torch.int32), mt.grid.view(torch.int32))
    # and the good ones are taken
    assert L.zs_rocm_levelset_transition_sample(h, C.byref(good), x.data_ptr(), n, out.data_ptr(), None, None) == 0
    assert L.zs_rocm_levelset_transition_sample(h, C.byref(_copy(good, alpha=1.0)), x.data_ptr(), n, out.data_ptr(), None, None) == 0
    pol.syncCtx()
    assert (out.reshape(-1)[:n] != 7.0).all()


# ------------------------------------------------------------------------------------------------ 8: the C++ face
def test_cpp_face_transition_program_runs():
    """tests/cpp/test_transition.hip: TransitionLevelSetView{src, dst, stepDt, alpha} and Collider over it in a user lambda == the C ABI's
    bulk entries, bit for bit"""
    exe = os.path.join(ROOT, "zpc_amd", "lib", "test_transition")
    if not os.path.exists(exe):
        from zpc_amd import build
        build.build_cpp_test("test_transition")
    r = subprocess.run(["timeout", "-k", "10", "240", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(r.stdout.decode()[-1500:])
    assert r.returncode == 0 and b"transition cpp face ok: 0 mismatches" in r.stdout, r.stdout.decode()[-3000:]
