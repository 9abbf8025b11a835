"""tests/ref64.py (float64 transfers with node-local bounds) validated against a real float32 implementation, the CPU oracle
(oracle/mpm.c): the oracle passes the bound on every model, block side and cloud, and the bound rejects small, local mistakes.

Negative controls, each against the oracle's own grid or particles (model 0, the jittered lattice unless stated):
  drop      one particle's lowest-weight node term (W >= 1e-3) is missing from all 7 channels
  shift     one particle's 27 terms land one node further along x
  stale_x   one particle is scattered from its position before a 0.05-cell move
  light     one particle of the 1e-3 m slab of the mixed-mass cloud has 1 % more mass
  stress    one particle's off-diagonal stress components xy and xz are swapped (P F^T vol is symmetric, so a transposition is a
            no-op: a mis-indexed pair is the form that mistake takes on the 6-component cached stress)
  stale_v   one particle's G2P reads the velocity of one stencil node (W ~ 0.03) from before the grid update (without g dt)
The channel-max checks of the GPU suite (_compare_grids(..., 2e-4) on grids, 2e-4 max|v| on G2P) accept light and stale_v, and accept
drop on the mass channel (1.04e-3 m against ~8 m per node); they catch drop only through its momentum.  test_negative_controls asserts
that too, so the gap this closes is measured, not assumed."""
import ctypes as C

import numpy as np
import pytest

import ref64
from util import make_cloud, make_mixed_cloud, make_edge_cloud, make_drifting_cloud, make_uneven_cloud, OracleMpm, oracle_stress, rng, ptr

DX, DT, G = 1.0 / 64, 1e-4, (0.0, -9.8, 0.0)
CLOUDS = ["lattice", "mixed", "edge", "drifting", "uneven"]


def cloud(name):
    if name == "lattice":
        return make_cloud(6, DX, 2, seed=3)
    if name == "mixed":
        return make_mixed_cloud(6, DX)
    if name == "edge":
        return make_edge_cloud(DX)
    if name == "drifting":
        return make_drifting_cloud()
    m, x, v, Cm, F, _ = make_uneven_cloud(7, ncell=6)
    return m, x, v, Cm, F


def model_kw(model):
    return dict(yield_stress=200.0) if model == 2 else dict(beta=0.5) if model == 3 else {}


def state(model, F, n):
    if model == 4:   # the fluid carries J in component 0 of the F slot
        F = F.copy()
        F[:, 0] = (1.0 + 0.01 * rng(11).standard_normal(n)).astype(np.float32)
    lj = (0.01 * rng(33).standard_normal(n)).astype(np.float32)
    return F, lj


def oracle_grid(om, side):
    return ref64.world_nodes(om.keys, om.grid, side, side)


def old_grid_check(got, want, rtol=2e-4):
    """_compare_grids of test_mpm_gpu.py on world-node arrays: err <= rtol * max |channel| on every channel"""
    s = np.abs(want).max(0) + 1e-30
    return bool((np.abs(got - want).max(0) <= rtol * s).all())


@pytest.mark.parametrize("cloud_name", CLOUDS)
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
def test_oracle_within_ref64_bounds(oracle, model, side, cloud_name):
    """P2G (all 7 channels, force from the oracle's own P F^T vol), grid update and G2P (x, v, C, F or J) of the float32 oracle are within
    the float64 reference's node-local / particle-local bounds"""
    mass, pos, vel, Cm, F = cloud(cloud_name)
    n = pos.shape[0]
    F, lj = state(model, F, n)
    om = OracleMpm(oracle, model, DX, DT, side, DX ** 3 / 8, **model_kw(model))
    om.build_partition(pos, n)
    PF = oracle_stress(oracle, om, Cm, F, lj)
    om.p2g(mass, pos, vel, Cm, F, lj.copy())
    ref = ref64.p2g64(mass, pos, vel, Cm, DX, DT, PF=PF)
    world = oracle_grid(om, side)
    ref64.check_grid(ref, world, what="oracle P2G")
    pre = world[1].copy()
    mx = om.grid_update(G)
    world = oracle_grid(om, side)
    has = pre[:, 0] != 0
    v, bv = ref64.grid_update64(pre[has, 0], pre[has, 1:4], DT, G)
    ref64.check_particles(world[1][has, 1:4], v, bv, "oracle grid update")
    vsq = (world[1][has, 1:4] ** 2).sum(1).max()
    assert abs(mx - vsq) <= 4 * ref64.U * vsq
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    om.g2p(po, vo, Co, Fo)
    r = ref64.g2p64((world[0], world[1][:, 1:4]), pos, DX, DT, F=None if model == 4 else F, J=F[:, 0] if model == 4 else None)
    ref64.check_particles(po, r["x"], r["b_x"], "oracle G2P x")
    ref64.check_particles(vo, r["v"], r["b_v"], "oracle G2P v")
    ref64.check_particles(Co, r["C"], r["b_C"], "oracle G2P C")
    if model == 4:
        ref64.check_particles(Fo[:, 0], r["J"], r["b_J"], "oracle G2P J")
    else:
        ref64.check_particles(Fo, r["F"], r["b_F"], "oracle G2P F")


def test_arena_decisions_follow_the_oracle(oracle):
    """Every discrete decision of arena32 (base node, lpn, d0 -- the 1.5 quirk included) agrees with the oracle's orc_arena on the edge
    cloud.  The oracle divides by dx, the kernels multiply by 1/dx: for a power-of-two dx both are exact and agree."""
    mass, pos, vel, Cm, F = make_edge_cloud(DX)
    corner, lpn, d0 = ref64.arena32(pos, DX)
    c = np.zeros(3, np.int32)
    lp, w = np.zeros(3, np.float32), np.zeros(9, np.float32)
    quirk = 0
    for i in range(pos.shape[0]):
        oracle.orc_arena(C.c_float(DX), ptr(np.ascontiguousarray(pos[i])), ptr(c), ptr(lp), ptr(w))
        assert np.array_equal(c, corner[i]) and np.array_equal(lp, lpn[i] * np.float32(DX)), i
        assert np.abs(w.reshape(3, 3) - ref64.weights64(d0[i])).max() <= 4 * ref64.U, i
        quirk += int(((lpn[i] >= 1.5) | (lpn[i] < 0.5)).any())
    assert quirk >= 9   # the cloud does reach the reference's quirk
    zero_w = (ref64.weights64(d0) == 0).any(axis=(1, 2))
    assert zero_w.sum() >= 8


def _single(mass, pos, vel, Cm, PF, i):
    return ref64.p2g64(mass[i:i + 1], pos[i:i + 1], vel[i:i + 1], Cm[i:i + 1], DX, DT, PF=PF[i:i + 1])


def _add(world, g, sign=1.0, shift=(0, 0, 0)):
    """add (sign = -1: remove) the nodes of a Grid64 to world-node values, optionally displaced by `shift` nodes"""
    coords, vals = world
    k = ref64.node_key(coords)
    o = np.argsort(k)
    idx = o[np.searchsorted(k[o], ref64.node_key(g.coords + np.asarray(shift)))]
    vals = vals.copy()
    np.add.at(vals, idx, sign * g.val)
    return coords, vals


def _interior(pos, lo_cells=1.5):
    lo, hi = pos.min(0) + lo_cells * DX, pos.max(0) - lo_cells * DX
    return np.nonzero(((pos > lo) & (pos < hi)).all(1))[0]


def test_negative_controls(oracle):
    side = 4
    mass, pos, vel, Cm, F = make_cloud(6, DX, 2, seed=3)
    n = pos.shape[0]
    om = OracleMpm(oracle, 0, DX, DT, side, DX ** 3 / 8)
    om.build_partition(pos, n)
    PF = oracle_stress(oracle, om, Cm, F)
    om.p2g(mass, pos, vel, Cm, F)
    good = oracle_grid(om, side)
    ref = ref64.p2g64(mass, pos, vel, Cm, DX, DT, PF=PF)
    ref64.check_grid(ref, good)
    inner = _interior(pos)
    old = {}

    def rejected(world, name, r=ref):
        with pytest.raises(AssertionError):
            ref64.check_grid(r, world, what=name)
        rows = r.lookup(world[0])
        have = rows >= 0
        got, want = world[1][have], r.val[rows[have]]
        old[name] = old_grid_check(got, want, 2e-4)

    # drop: an interior particle loses its lowest-weight node term among those with W >= 1e-3
    i = inner[len(inner) // 2]
    one = _single(mass, pos, vel, Cm, PF, i)
    w = one.val[:, 0] / mass[i]
    k = int(np.argmin(np.where(w >= 1e-3, w, np.inf)))
    assert 1e-3 <= w[k] < 1e-2
    drop = ref64.Grid64(one.coords[k:k + 1], one.val[k:k + 1], one.T[k:k + 1], one.N[k:k + 1], one.ein[k:k + 1], one.c)
    rejected(_add(good, drop, -1.0), "drop")
    # shift: one node along x
    rejected(_add(_add(good, one, -1.0), one, 1.0, (1, 0, 0)), "shift")
    # stale_x: scattered from the position before a 0.05-cell move
    pos2 = pos.copy()
    pos2[i, 0] -= np.float32(0.05 * DX)
    om.grid[:] = 0
    om.p2g(mass, pos2, vel, Cm, F)
    rejected(oracle_grid(om, side), "stale_x")
    # stress: xy and xz of one particle swapped
    PFs = PF.copy()
    PFs[i, [3, 6]] = PF[i, [6, 3]]
    PFs[i, [1, 2]] = PF[i, [2, 1]]
    assert abs(PF[i, 3] - PF[i, 6]) > 0.1 * np.abs(PF[i]).max()
    bad = _single(mass, pos, vel, Cm, PFs, i)
    rejected(_add(_add(good, one, -1.0), bad, 1.0), "stress")
    # light: mixed-mass cloud, one particle of the 1e-3 m slab (away from the other slabs) with 1 % more mass
    mm, xm, vm, Cmm, Fm = make_mixed_cloud(6, DX)
    omm = OracleMpm(oracle, 0, DX, DT, side, DX ** 3 / 8)
    omm.build_partition(xm, xm.shape[0])
    PFm = oracle_stress(oracle, omm, Cmm, Fm)
    refm = ref64.p2g64(mm, xm, vm, Cmm, DX, DT, PF=PFm)
    cand = np.nonzero((mm < 2e-3 * mm.max()) & (mm > 2e-4 * mm.max()))[0]
    mid = np.median(xm[cand, 0])
    j = cand[np.argmin(np.abs(xm[cand] - np.array([mid, np.median(xm[:, 1]), np.median(xm[:, 2])])).sum(1))]
    mm2 = mm.copy()
    mm2[j] *= np.float32(1.01)
    omm.p2g(mm2, xm, vm, Cmm, Fm)
    rejected(oracle_grid(omm, side), "light", refm)
    # stale_v: G2P with one stencil node's velocity from before the grid update
    om.grid[:] = 0
    om.p2g(mass, pos, vel, Cm, F)
    pre = oracle_grid(om, side)[1]
    om.grid_update(G)
    coords, vals = oracle_grid(om, side)
    has = pre[:, 0] != 0
    r = ref64.g2p64((coords[has], vals[has, 1:4]), pos, DX, DT)
    nodes, W, _, _ = ref64.stencil(pos[i:i + 1], DX)
    kk = int(np.argmin(np.abs(W[0] - 0.03)))
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    om.g2p(po, vo, Co, Fo)
    b, c = om.grid_by_key(), nodes[0, kk]
    blk = tuple(int(x) for x in np.floor_divide(c, side))
    loc = c - np.asarray(blk) * side
    b[blk][1:4, (loc[0] * side + loc[1]) * side + loc[2]] -= np.asarray(G, np.float32) * np.float32(DT)
    ps, vs, Cs, Fs = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    om.g2p(ps, vs, Cs, Fs)
    vo[i] = vs[i]                     # only particle i read the stale node
    with pytest.raises(AssertionError):
        ref64.check_particles(vo, r["v"], r["b_v"], "stale_v")
    old["stale_v"] = bool(np.abs(vo - r["v"]).max() < 2e-4 * np.abs(r["v"]).max())
    assert old == dict(drop=False, shift=False, stale_x=False, stress=False, light=True, stale_v=True), old
    # the dropped term alone is below the old bar on the mass channel (it is caught there only through the momentum channel)
    dropped = _add(good, drop, -1.0)
    rows = ref.lookup(dropped[0])
    assert old_grid_check(dropped[1][rows >= 0][:, :1], ref.val[rows[rows >= 0]][:, :1])
