"""tests/ref64_c2.py (float64 P2C2G / G2C2P with node-local and particle-local bounds) validated against a real float32
implementation, the CPU oracle (oracle/mpm.c orc_mpm_p2c2g, orc_mpm_g2c2p, orc_mpm_post_g2c2p): the oracle passes the bound on every
kind, model, block side and scene of util.c2_scene without a single node or particle excluded, and the bound rejects small, local
mistakes.

Negative controls, each against the oracle's own output (jittered lattice, side 4, FixedCorotated unless stated):
  a  low_weight  one particle is missing from the one cell where its weight is smallest but >= 1e-3
  b  octant      one particle is missing from one cell at weight >= 0.1 (a particle sorted into the wrong octant)
  c  light       one particle of the 1e-3 m slab of the mixed-mass cloud is 1 % heavier
  d  stale_x     one particle is scattered from its position before a 0.05-cell move
  e  node        one cell's v_c (and vx_c) is built without one of its present nodes
  f  neighbour   one particle's B is formed with x_p of its neighbour
  g  twice       logJp of one NACC particle (the one of median hardening) is advanced twice; the check is the 1e-4 of
                 test_c2_ref64_gpu.py on logJp, under which 98.4 % of the scene's hardening particles do not fit a second time
The channel-max checks of tests/test_c2_gpu.py (_cmp at 2e-4 on the grid; 2e-4 max|v|, 2e-4 max|B| + 1e-9 on the particles; 2e-3 on NACC's
logJp) accept c, and accept a on the mass channel (they catch it only through its momentum); they reject b, d, e, f and g as placed
here (the median hardening step, 6e-3, is over 2e-3; a step between 1e-4 and 2e-3 is not): OLD_ACCEPTS, asserted by
test_negative_controls, so the gap closed is measured, not assumed."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref64_c2 as r2
from util import c2_scene, c2_lone_pos, C2_SCENES, OracleMpm, oracle_stress, rng, ptr

DX, DT, G = 1.0 / 64, 1e-4, (0.0, -9.8, 0.0)
VOL = DX ** 3 / 8
LOGJP_TOL = 1e-4
OLD_ACCEPTS = dict(low_weight=False, low_weight_mass=True, octant=False, light=True, stale_x=False, node=False, neighbour=False, twice=False)
_PF = {}


def model_kw(model):
    return dict(yield_stress=200.0) if model == 2 else dict(beta=0.5) if model == 3 else {}


def setup(oracle, scene, side, model):
    """the oracle with the scene's partition and buckets; the scene with `Fin` = the model's deformation state in the F slot"""
    s = c2_scene(scene, DX)
    om = OracleMpm(oracle, model, DX, DT, side, VOL, **model_kw(model))
    if s["block"] is not None:
        s["pos"] = c2_lone_pos(s["block"], side, DX)
        om.adopt_partition(np.array([s["block"]], np.int32))
    else:
        om.build_partition(s["pos"], s["pos"].shape[0])
    om.build_buckets(s["pos"])
    s["Fin"] = s["F"].copy()
    if model == 4:
        s["Fin"][:, 0] = s["J"][:, 0]
    return om, s


def stress(oracle, om, s, scene, side):
    key = (scene, om.p.model, side if s["block"] is not None else 0)
    if key not in _PF:
        _PF[key] = oracle_stress(oracle, om, s["B"], s["Fin"], s["logJp"])
    return _PF[key]


def world(om):
    return ref64.world_nodes(om.keys, om.grid, om.side, om.side)


def old_grid_check(got, want, rtol=2e-4, chans=range(4)):
    """_cmp of test_c2_gpu.py on world-node arrays: err <= rtol * max |channel|"""
    return all(np.abs(got[:, ch] - want[:, ch]).max() <= rtol * (np.abs(want[:, ch]).max() + 1e-30) for ch in chans)


def old_particle_check(v, B, vo, Bo):
    """test_g2c2p_vs_oracle's bars on v and B"""
    return bool(np.abs(v - vo).max() < 2e-4 * np.abs(vo).max() and np.abs(B - Bo).max() < 2e-4 * np.abs(Bo).max() + 1e-9)


def check_g2c2p(r, x, v, B, F, model, what):
    ref64.check_particles(v, r["v"], r["b_v"], what + " v")
    ref64.check_particles(B, r["B"], r["b_B"], what + " B")
    ref64.check_particles(x, r["x"], r["b_x"], what + " x")
    if model == 4:
        ref64.check_particles(F[:, 0], r["J"], r["b_J"], what + " J")
    else:
        ref64.check_particles(F, r["F"], r["b_F"], what + " F")


@pytest.mark.parametrize("scene", C2_SCENES)
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
def test_oracle_within_ref64_c2_bounds(oracle, model, side, scene):
    """P2C2G kinds 0, 1, 2 (channels 0-3, the force part from the oracle's own P F^T vol, so to rounding), then grid update and G2C2P +
    Post (v, B, x, F or J), and the bare accumulate entry on non-zero v0, B0"""
    om, s = setup(oracle, scene, side, model)
    mass, pos, vel, B, Fin, lj = s["mass"], s["pos"], s["vel"], s["B"], s["Fin"], s["logJp"]
    n = len(mass)
    PF = stress(oracle, om, s, scene, side)
    keys = om.keys
    origin = s["key_is_origin"]          # the oracle has block keys only: the reference must give the same from the block origins
    rkeys = keys * side if origin else keys
    for kind in (0, 1, 2):
        om.grid[:] = 0
        lj1 = om.p2c2g(kind, mass, pos, vel, B, Fin, lj.copy())
        ref = r2.p2c2g64(kind, rkeys, side, mass, pos, vel, B, DX, DT, PF=PF, key_is_origin=origin)
        w = world(om)
        ref64.check_grid(ref, w, range(4), "oracle P2C2G kind %d" % kind)
        assert not w[1][:, 4:].any()
        if kind == 2:
            assert not w[1][:, 0].any()
        if kind == 1 or model not in (1, 3):
            assert np.array_equal(lj1, lj)
    om.grid[:] = 0
    om.p2c2g(0, mass, pos, vel, B, Fin, lj.copy())
    om.grid_update(G)
    w = world(om)
    nodes = (w[0], w[1][:, 1:4])
    st = dict(F=None if model == 4 else Fin, J=Fin[:, 0] if model == 4 else None)
    po, vo, Bo, Fo = pos.copy(), vel.copy(), B.copy(), Fin.copy()
    om.g2c2p(po, vo, Bo, Fo)
    check_g2c2p(r2.g2c2p64(rkeys, side, nodes, pos, DX, DT, key_is_origin=origin, **st), po, vo, Bo, Fo, model, "oracle G2C2P")
    g = rng(5)
    v0, B0 = (0.3 * g.standard_normal((n, 3))).astype(np.float32), (1e-5 * g.standard_normal((n, 9))).astype(np.float32)
    va, Ba = v0.copy(), B0.copy()
    oracle.orc_mpm_g2c2p(C.byref(om.p), om.table, om.buckets, om._ib[1], om._ib[2], ptr(pos), ptr(va), ptr(Ba), ptr(om.grid))
    r = r2.g2c2p64(rkeys, side, nodes, pos, DX, DT, v0=v0, B0=B0, key_is_origin=origin)
    ref64.check_particles(va, r["v"], r["b_v"], "oracle G2C2P accumulate v")
    ref64.check_particles(Ba, r["B"], r["b_B"], "oracle G2C2P accumulate B")


def test_scenes_are_what_they_claim():
    """the per-cell counts of `faces` and `counts`, the octants of the two 255-particle cells, the exact positions of `faces`"""
    cnt = lambda pos: np.unique(np.floor(pos.astype(np.float64) / DX).astype(int), axis=0, return_counts=True)
    s = c2_scene("faces", DX)
    cells, k = cnt(s["pos"])
    assert len(cells) == 8 and ((k >= 22) & (k <= 255)).all(), k
    X = s["pos"].astype(np.float64) / DX
    fr = X - np.floor(X)
    assert (fr == 0).all(1).any() and (fr == 0.5).all(1).any() and (fr == 0).any() and ((fr > 0.5) & (fr < 0.5 + 1e-5)).any()
    s = c2_scene("counts", DX)
    cells, k = cnt(s["pos"])
    assert sorted(k[k != 8].tolist()) == [21, 22, 255, 255, 256] and len(cells) == 125
    X = s["pos"].astype(np.float64) / DX
    for c in cells[k == 255]:
        f = (X - np.floor(X))[(np.floor(X).astype(int) == c).all(1)]
        assert (f < 0.5).all() or (f >= 0.5).all()
    assert c2_scene("far", DX)["pos"].min(0).tolist() != c2_scene("lattice", DX)["pos"].min(0).tolist()
    s = c2_scene("edge", DX)
    assert (s["pos"] < 0).any(0).all() and (s["pos"] > 0).any(0).all()


def _add(wld, g, sign=1.0):
    """add (sign = -1: remove) the nodes of a Grid64 to world-node values"""
    coords, vals = wld
    k = ref64.node_key(coords)
    o = np.argsort(k)
    idx = o[np.searchsorted(k[o], ref64.node_key(g.coords))]
    vals = vals.copy()
    np.add.at(vals, idx, sign * g.val)
    return coords, vals


def test_negative_controls(oracle):
    side = 4
    old = {}
    om, s = setup(oracle, "lattice", side, 0)
    mass, pos, vel, B, F = s["mass"], s["pos"], s["vel"], s["B"], s["Fin"]
    PF = oracle_stress(oracle, om, B, F)
    om.p2c2g(0, mass, pos, vel, B, F)
    good = world(om)
    ref = r2.p2c2g64(0, om.keys, side, mass, pos, vel, B, DX, DT, PF=PF)
    ref64.check_grid(ref, good, range(4))

    def rejected(wld, name, r=ref, want=good):
        with pytest.raises(AssertionError):
            ref64.check_grid(r, wld, range(4), what=name)
        old[name] = old_grid_check(wld[1], want[1])

    lo, hi = pos.min(0) + 1.5 * DX, pos.max(0) - 1.5 * DX
    inner = np.nonzero(((pos > lo) & (pos < hi)).all(1))[0]
    i = inner[len(inner) // 2]
    cells = r2.partition_cells(om.keys, side)
    _, c, W, _ = r2.pairs(pos[i:i + 1], cells, DX)
    one = lambda cell: r2.p2c2g64(0, om.keys, side, mass[i:i + 1], pos[i:i + 1], vel[i:i + 1], B[i:i + 1], DX, DT, PF=PF[i:i + 1],
                                  only_cells=cells[cell][None])
    # a, b: one (particle, cell) term is missing
    ka = int(np.argmin(np.where(W >= 1e-3, W, np.inf)))
    assert 1e-3 <= W[ka] < 0.1
    low = _add(good, one(c[ka]), -1.0)
    rejected(low, "low_weight")
    old["low_weight_mass"] = old_grid_check(low[1], good[1], chans=[0])
    kb = int(np.argmin(np.where(W >= 0.1, W, np.inf)))
    assert 0.1 <= W[kb] < 0.5
    rejected(_add(good, one(c[kb]), -1.0), "octant")
    # d: scattered from the position before a 0.05-cell move
    pos2 = pos.copy()
    pos2[i, 0] -= np.float32(0.05 * DX)
    om.build_buckets(pos2)
    om.grid[:] = 0
    om.p2c2g(0, mass, pos2, vel, B, F)
    rejected(world(om), "stale_x")
    # c: mixed-mass cloud, one particle of the 1e-3 m slab (away from the other slabs) with 1 % more mass
    omm, sm = setup(oracle, "mixed", side, 0)
    mm, xm = sm["mass"], sm["pos"]
    PFm = oracle_stress(oracle, omm, sm["B"], sm["Fin"])
    omm.p2c2g(0, mm, xm, sm["vel"], sm["B"], sm["Fin"])
    goodm = world(omm)
    refm = r2.p2c2g64(0, omm.keys, side, mm, xm, sm["vel"], sm["B"], DX, DT, PF=PFm)
    ref64.check_grid(refm, goodm, range(4))
    cand = np.nonzero((mm < 2e-3 * mm.max()) & (mm > 2e-4 * mm.max()))[0]
    mid = np.array([np.median(xm[cand, 0]), np.median(xm[:, 1]), np.median(xm[:, 2])])
    j = cand[np.argmin(np.abs(xm[cand] - mid).sum(1))]
    mm2 = mm.copy()
    mm2[j] *= np.float32(1.01)
    omm.grid[:] = 0
    omm.p2c2g(0, mm2, xm, sm["vel"], sm["B"], sm["Fin"])
    rejected(world(omm), "light", refm, goodm)
    # e, f: G2C2P
    om.build_buckets(pos)
    om.grid[:] = 0
    om.p2c2g(0, mass, pos, vel, B, F)
    om.grid_update(G)
    w = world(om)
    nodes = (w[0], w[1][:, 1:4])
    po, vo, Bo, Fo = pos.copy(), vel.copy(), B.copy(), F.copy()
    om.g2c2p(po, vo, Bo, Fo)
    r = r2.g2c2p64(om.keys, side, nodes, pos, DX, DT, F=F)
    check_g2c2p(r, po, vo, Bo, Fo, 0, "oracle")

    def rejected_particles(v, Bm, name):
        with pytest.raises(AssertionError):
            ref64.check_particles(v, r["v"], r["b_v"], name + " v")
            ref64.check_particles(Bm, r["B"], r["b_B"], name + " B")
        old[name] = old_particle_check(v, Bm, vo, Bo)

    cell = cells[c[kb]]
    k = int(np.nonzero((w[0] == cell + 1).all(1))[0][0])          # the cell's node + (1, 1, 1)
    assert np.abs(w[1][k, 1:4]).min() > 1e-3
    d = r2.g2c2p64(om.keys, side, (w[0][k:k + 1], w[1][k:k + 1, 1:4]), pos, DX, DT, only_cells=cell[None])
    assert (np.abs(d["v"]).max(1) > 0).sum() > 8                # every particle within dx of the cell reads the short v_c
    rejected_particles(vo - d["v"], Bo - d["B"], "node")
    q = int(np.argsort(np.abs(pos - pos[i]).sum(1))[1])           # the nearest other particle
    Bf = Bo.astype(np.float64)
    Bf[i] += (vo[i].astype(np.float64)[:, None] * (pos[i] - pos[q]).astype(np.float64)[None, :]).T.reshape(9)   # [r + 3 j]
    rejected_particles(vo, Bf, "neighbour")
    # g: NACC, logJp advanced twice; the check is |logJp - entry's logJp| <= 1e-4, the entry being the same stress on the same input
    on, sn = setup(oracle, "lattice", side, 3)
    lj1 = on.p2c2g(0, sn["mass"], sn["pos"], sn["vel"], sn["B"], sn["Fin"], sn["logJp"].copy())
    on.grid[:] = 0
    lj2 = on.p2c2g(0, sn["mass"], sn["pos"], sn["vel"], sn["B"], sn["Fin"], lj1.copy())
    hard = np.nonzero(lj1 != sn["logJp"])[0]
    assert len(hard) > len(lj1) // 2                             # the scene does harden
    gap = np.abs(lj2 - lj1)[hard]
    # a second application does not fit under the bar: measured, 98.4 % of the hardening particles move by more than 1e-4 again (median
    # 6e-3); the others sit next to the yield surface, where the second step is as small as the first
    assert (gap > LOGJP_TOL).mean() > 0.95 and np.median(gap) > 30 * LOGJP_TOL, ((gap > LOGJP_TOL).mean(), np.median(gap))
    t = hard[np.argsort(gap)[len(gap) // 2]]
    bad = lj1.copy()
    bad[t] = lj2[t]
    assert np.abs(lj1 - lj1).max() <= LOGJP_TOL and not np.abs(bad - lj1).max() <= LOGJP_TOL
    old["twice"] = bool(np.abs(bad - lj1).max() < 2e-3)
    assert old == OLD_ACCEPTS, old
