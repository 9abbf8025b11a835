"""The bin end of the 8^3 block kernel of the slotted step (blk_consumer, zpc_amd/csrc/mpm_slotblk.hip): a bin's 8^3 arena reaches the grid
as its dense 6^3 core (4 passes) plus the 8 x 8 faces of its shell that the bin's mover lists flagged, every pass writes zero over what it
read, and the arena is cleared once per workgroup instead of once per bin.

The cloud (shell_cloud): one 8^3 block (cells 32..39 per axis, all 8 bins populated, a few hundred particles) in a velocity field that
carries particles placed within 0.02 cell of bin faces out of their bins -- through each of the 6 faces, across edges and corners, into
another bin of the block and into the neighbouring blocks -- so that every face of the shell is written by a list and flushed.  The grid
of every step is checked node by node against the float64 reference of tests/ref64.py exactly as tests/test_mpm_ref64_gpu.py checks
zs_rocm_mpm_step_slotted (mass and force channels against p2g64 of the stored particles, the updated velocities against grid_update64);
check_grid also demands an exact 0 at every node the reference does not touch, which is where a node flushed twice, a stale shell value of
an earlier bin or a node missed by the face passes would show."""
import os

import numpy as np
import pytest

import ref64
from util import rng, tag_masses, OracleMpm, oracle_stress

DX = 1.0 / 64
DT = 1e-3
G = (0.0, -9.8, 0.0)
VOL = DX ** 3 / 8
ORG = 32          # the block's first cell on every axis
MASS_SUM_RTOL = 1.4e-8   # see test_zero_on_flush_carries_across_bins_and_steps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slot_block_flush_at_rest.npz")


def _field(p):
    """the velocity field's factor at coordinate p (cells from the block's origin): +1 on the block's faces (0, 8), -1 on the face
    between its bins (4)"""
    return np.cos(0.25 * np.pi * p)


def shell_cloud(at_rest=False, seed=20):
    """(mass, pos, vel, C, F, cls): coordinates p = X - 0.5 - ORG in cells from the block's origin (base node = floor(p)).  The velocity
    is a smooth field of the position, v_d = a * _field(p_e), e = (d + 1) % 3, a = 0.12 cell per step (smooth: P2G and G2P hand a
    particle back nearly its own velocity).  A particle within 0.02 cell of a bin face on axis d leaves through it when the field there
    points outward, which its coordinate on axis e decides: positive near p_e = 0 and 8, negative near p_e = 4.  cls: 0 stayers anywhere
    in the block, 1 face, 2 edge, 3 corner movers.  at_rest: the same positions, v = 0."""
    g = rng(seed)

    def free():                       # any cell, well inside it
        return g.integers(0, 8) + 0.25 + 0.5 * g.random()

    def near(sign, mid=None):         # just inside a bin face and about to leave through it; mid: the face between the bins (p = 4)
        mid = g.random() < 0.5 if mid is None else mid
        eps = 0.004 + 0.016 * g.random()
        return (4 if mid else 8) - eps if sign > 0 else (4 if mid else 0) + eps

    def steer(sign):                  # a coordinate inside a cell at which the field has this sign, |field| >= 0.83
        return g.choice([0, 7] if sign > 0 else [3, 4]) + 0.25 + 0.5 * g.random()

    P, cls = [], []
    for d in range(3):
        e, f = (d + 1) % 3, (d + 2) % 3
        for s in (+1, -1):
            for _ in range(20):       # through the face (d, s)
                p = np.zeros(3)
                p[d], p[e], p[f] = near(s), steer(s), free()
                P.append(p), cls.append(1)
            for mid in (False, True):
                for _ in range(8):    # across an edge of the faces of axes d and e: p_e on a bin face decides the sign on axis d
                    p = np.zeros(3)
                    p[d], p[e], p[f] = near(-1 if mid else +1), near(s, mid), steer(s)
                    P.append(p), cls.append(2)
    for t in range(8):                # across the 8 kinds of corner: axis d sits on the middle face (bit d of t) or on an outer one
        mid = [(t >> d) & 1 == 1 for d in range(3)]
        for _ in range(10):
            P.append(np.array([near(-1 if mid[(d + 1) % 3] else +1, mid[d]) for d in range(3)])), cls.append(3)
    for _ in range(150):
        P.append(np.array([free(), free(), free()])), cls.append(0)
    P = np.asarray(P)
    n = P.shape[0]
    pos = ((P + 0.5 + ORG) * DX).astype(np.float32)
    a = 0.12 * DX / DT
    vel = np.zeros((n, 3), np.float32) if at_rest else np.ascontiguousarray(a * _field(P[:, [1, 2, 0]]), np.float32)
    Cm = (0.01 * g.standard_normal((n, 9))).astype(np.float32)
    F = (np.eye(3).reshape(1, 9) + 1e-3 * g.standard_normal((n, 9))).astype(np.float32)
    mass = tag_masses(np.full(n, 1000.0 * VOL, np.float32))
    return mass, pos, vel, Cm, F, np.asarray(cls)


def crossings(x0, x1):
    """what the movers of a step did, from the positions before and after it: per face of a 4^3 bin (2 d + s) the movers that left
    their bin through it, movers that changed bin on 2 / 3 axes, movers into another bin of their block / into another block"""
    c0, c1 = ref64.arena32(x0, DX)[0], ref64.arena32(x1, DX)[0]
    b0, b1 = c0 >> 2, c1 >> 2
    out = {"face%d" % (2 * d + s): int((b1[:, d] - b0[:, d] == (1 if s else -1)).sum()) for d in range(3) for s in (0, 1)}
    nax = (b0 != b1).sum(1)
    other_block = ((c0 >> 3) != (c1 >> 3)).any(1)
    out.update(edge=int((nax == 2).sum()), corner=int((nax == 3).sum()), in_block=int(((nax > 0) & ~other_block).sum()),
               cross_block=int(other_block.sum()), cell=int((c0 != c1).any(1).sum()))
    return out


def _covered(cr):
    return all(cr["face%d" % f] >= 5 for f in range(6)) and cr["edge"] >= 5 and cr["corner"] >= 3 and cr["in_block"] >= 20 and cr["cross_block"] >= 20


def test_shell_cloud_on_the_cpu_oracle_crosses_every_face_and_its_reference_passes_its_own_bounds(oracle):
    """No GPU: one step of the float32 CPU oracle on the cloud.  Its movers leave bins through all 6 faces, across edges and corners, into
    the same block and into its neighbours; the oracle's P2G of the moved particles is within the float64 reference's node-local bounds
    (the reference alone passes on this input, near-face positions included); at rest no particle changes its cell."""
    for at_rest in (False, True):
        mass, pos, vel, Cm, F, _ = shell_cloud(at_rest)
        n = pos.shape[0]
        assert len(np.unique((ref64.arena32(pos, DX)[0] - ORG) >> 2, axis=0)) == 8   # all 8 bins of the one block
        assert ((ref64.arena32(pos, DX)[0] - ORG) >> 3 == 0).all()
        om = OracleMpm(oracle, 0, DX, DT, 8, VOL)
        keys = np.stack(np.meshgrid(*[np.arange(ORG // 8 - 1, ORG // 8 + 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
        om.adopt_partition(keys)
        om.p2g(mass, pos, vel, Cm, F)
        om.grid_update(G)
        po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
        om.g2p(po, vo, Co, Fo)
        cr = crossings(pos, po)
        if at_rest:
            assert cr["cell"] == 0, cr
            continue
        assert _covered(cr), cr
        om.grid[:] = 0
        PF = oracle_stress(oracle, om, Co, Fo)
        om.p2g(mass, po, vo, Co, Fo)
        ref = ref64.p2g64(mass, po, vo, Co, DX, DT, PF=PF)
        ref64.check_grid(ref, ref64.world_nodes(om.keys, om.grid, 8, 8), what="oracle P2G of the moved shell cloud")


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _helpers():
    import test_mpm_ref64_gpu as t   # the checked step of zs_rocm_mpm_step_slotted, as that module does it
    return t


def _slotted(pol, cloud, margin=1):
    from zpc_amd.mpm import MpmTransfer
    mass, pos, vel, Cm, F = cloud[:5]
    n = pos.shape[0]
    mt = MpmTransfer(pol, n, DX, DT, model=0, side=8, volume=VOL, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, None)
    mt.build_partition(n, margin=margin)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update(G)
    mt.slot(K=32, outbox_cap=512)
    return mt


def _checked_step(path, mt, om, write_all):
    """one zs_rocm_mpm_step_slotted: the G2P half per particle, then all 7 channels of the new grid -- mass and force against p2g64 of
    the stored particles, the updated velocities against grid_update64 with the P2G bounds propagated.  Returns (before, after, world,
    bound): bound [nodes, 7] = the bound every node of `world` was held to (mass, velocity x 3, force x 3; 0 at untouched nodes)."""
    t = _helpers()
    grid = ref64.to_world_nodes(mt)
    has = grid[1][:, 0] != 0
    before = t._by_mass(t._fields(t._read_all(mt), mt))
    mt.step_slotted(G, write_all=write_all)
    mt.pol.syncCtx()
    st = mt.check_slots()
    assert st[5] == st[6], st
    after = t._by_mass(t._fields(t._read_all(mt), mt))
    assert np.array_equal(after["m"], before["m"])
    x_after = after["x"].copy()
    if not write_all:
        del after["v"], after["C"]
    r = t._g2p_checked(path, grid, has, before, after, DT, 0)
    v, Cm, ev, eC = (after["v"], after["C"], None, None) if write_all else (r["v"], r["C"], r["b_v"], r["b_C"])
    PF, ePF = t._fc_oracle_stress(om, after, write_all)
    ref = ref64.p2g64(after["m"], after["x"], v, Cm, DX, DT, PF=PF, ev=ev, eC=eC, ePF=ePF)
    world = ref64.to_world_nodes(mt)
    t._report(path + " step m, force", ref64.check_grid(ref, world, [0, 4, 5, 6], path))
    vg, bv = ref64.grid_update64(ref.val[:, 0], ref.val[:, 1:4], DT, G, ref.bound()[:, 0], ref.bound()[:, 1:4])
    rows = ref.lookup(world[0])
    sel = rows >= 0
    assert (world[1][~sel][:, 1:4] == 0).all()
    sel[sel] = ref.val[rows[sel], 0] > 0
    t._report(path + " step v", ref64.check_particles(world[1][sel, 1:4], vg[rows[sel]], bv[rows[sel]], path + " v"))
    bound = np.zeros_like(world[1])
    bound[sel] = np.concatenate([ref.bound()[rows[sel], :1], bv[rows[sel]], ref.bound()[rows[sel], 4:]], 1)
    return before, dict(after, x=x_after), world, bound


@pytest.mark.gpu
@pytest.mark.parametrize("write_all", [True, False])
def test_flush_covers_every_face_edge_and_corner_of_the_shell(pol, oracle, write_all):
    """One step of the shell cloud (write_all on; off = the product instantiation): movers leave bins through all 6 faces, across edges
    and corners, into bins of the same block and into neighbouring blocks (counted from the stored positions), and all 7 channels of the
    grid are within the node-local float64 bounds, untouched nodes exactly 0."""
    mt = _slotted(pol, shell_cloud())
    om = OracleMpm(oracle, 0, DX, DT, 8, VOL)
    before, after, _, _ = _checked_step("flush[shell wa%d]" % write_all, mt, om, write_all)
    cr = crossings(before["x"], after["x"])
    print("FLUSH crossings", cr)
    assert _covered(cr), cr


@pytest.mark.gpu
def test_zero_on_flush_carries_across_bins_and_steps(pol, oracle):
    """Three steps of the shell cloud: the arena is cleared once per workgroup, so every later bin (8 per block) and every later step rely
    on the flush having left it zero.  Per step: the grid as above, and the sum of the mass channel equals the sum of the particle
    masses.  Tolerance of the sum (MASS_SUM_RTOL): the spread the float32 CPU oracle's P2G shows on this input -- over the three steps'
    particle states and 64 particle orders each (the given one and 63 random permutations), the mass channel of its grid (~1290 non-zero
    nodes) sums to within 1.37e-8 sum(m) of sum(m), measured; taken as 1.4e-8."""
    mt = _slotted(pol, shell_cloud())
    om = OracleMpm(oracle, 0, DX, DT, 8, VOL)
    moved = 0
    for step in range(3):
        before, after, world, _ = _checked_step("flush[3 steps] step %d" % step, mt, om, step == 1)
        moved += crossings(before["x"], after["x"])["cell"]
        total, want = world[1][:, 0].sum(), after["m"].astype(np.float64).sum()
        print("FLUSH mass sum step %d: rel. difference %.3g" % (step, abs(total - want) / want))
        assert abs(total - want) <= MASS_SUM_RTOL * want, (step, total, want)
    assert moved > 150, moved


def at_rest_result(pol):
    """(stored particle state by mass, world nodes) after one zs_rocm_mpm_step_slotted(write_all) of the cloud at rest"""
    t = _helpers()
    mt = _slotted(pol, shell_cloud(at_rest=True))
    mt.step_slotted(G, write_all=True)
    pol.syncCtx()
    mt.check_slots()
    return t._by_mass(t._fields(t._read_all(mt), mt)), ref64.to_world_nodes(mt)


@pytest.mark.gpu
def test_at_rest_no_face_is_flushed_and_the_result_is_the_parents(pol, oracle):
    """The same positions at rest (v = 0): no particle changes its cell, the lists are empty, the face mask is 0 and only the cores are
    flushed.  The grid is within the node-local bounds, and every node, on all 7 channels (the velocities after the grid update
    included), is within that same bound of the grid the parent of this change computed; the stored particle state is bit-identical to
    the parent's -- the first step's G2P half reads a grid the unfused kernels built, so it does not depend on the order of any atomic sum.

    The parent's result is tests/golden/slot_block_flush_at_rest.npz: at_rest_result() run on an MI355X with the library built from the
    commit before this change (da15d84; `ZS_ROCM_LIB=<that libzsrocm.so> python tests/test_slot_block_flush_gpu.py OUT.npz`), stored as
    m, x, v, C, F, PF (particles ordered by their tagged mass) and coords (int32) / grid (float32, 7 channels) of every partition node."""
    om = OracleMpm(oracle, 0, DX, DT, 8, VOL)
    mt = _slotted(pol, shell_cloud(at_rest=True))
    before, after, world, bound = _checked_step("flush[at rest]", mt, om, True)
    assert crossings(before["x"], after["x"])["cell"] == 0
    assert int(mt.mover_count[:mt.nbins].sum().item()) == 0
    t = _helpers()
    gold = np.load(GOLDEN)
    state = t._by_mass(t._fields(t._read_all(mt), mt))
    for k in ("m", "x", "v", "C", "F", "PF"):
        assert np.array_equal(state[k].view(np.uint32), gold[k].view(np.uint32)), k
    assert np.array_equal(world[0], gold["coords"])
    err = np.abs(world[1] - gold["grid"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    print("FLUSH at rest vs the parent's grid, worst |difference| / bound per channel:", " ".join("%.3f" % x for x in ratio.max(0)))
    assert (err <= bound).all(), ratio.max(0)


@pytest.mark.gpu
def test_core_node_of_a_missing_block_still_latches_status_2(pol):
    """Status report: a partition without margin (the blocks of the first upload and their +1 neighbours), then eight particles put
    into the apron block at +x, 0.01 cell below the face between its cells 5 and 6 and moving +x.  They are in-bin movers (no outbox, no
    list: the producers report nothing); from cell 6 their stencil reaches node 8 = the block at +2, which is not in the partition: the
    flush of the bin's core finds mass for a missing block and latches status[2]."""
    from zpc_amd.mpm import MpmTransfer
    g = rng(5)
    n = 8
    p0 = ORG + 1.0 + 5.0 * g.random((n, 3))                           # first upload: inside the block at ORG, defines the partition
    p1 = np.stack([np.full(n, ORG + 8 + 5.99), ORG + 1.5 + 2.0 * g.random(n), ORG + 1.5 + 2.0 * g.random(n)], 1)
    mass = tag_masses(np.full(n, 1000.0 * VOL, np.float32))
    vel = np.tile(np.array([0.12 * DX / DT, 0.0, 0.0], np.float32), (n, 1))
    Cm = np.zeros((n, 9), np.float32)
    F = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))
    mt = MpmTransfer(pol, n, DX, DT, model=0, side=8, volume=VOL, cache_stress=True)
    mt.upload(mass, ((p0 + 0.5) * DX).astype(np.float32), vel, Cm, F, None)
    mt.build_partition(n, margin=0)
    keys = {tuple(k) for k in (mt.active_keys().astype(np.int64) * (8 // mt.kstride) // 8).tolist()}
    assert (ORG // 8 + 1, ORG // 8, ORG // 8) in keys and (ORG // 8 + 2, ORG // 8, ORG // 8) not in keys
    x1 = ((p1 + 0.5) * DX).astype(np.float32)
    mt.upload(mass, x1, vel, Cm, F, None)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, 0.0, 0.0))
    mt.slot(K=16, outbox_cap=64)
    mt.g2p2g(write_all=True)
    pol.syncCtx()
    assert int(mt.mover_count[:mt.nbins].sum().item()) == 0
    st = mt.check_slots(strict=False)
    assert st[2] == 1, st
    assert st[0] == 0 and st[1] == 0 and st[4] == 0 and st[5] == st[6], st
    d = mt.download()
    c1 = ref64.arena32(d["x"], DX)[0]
    assert (c1[:, 0] == ORG + 8 + 6).all() and (ref64.arena32(x1, DX)[0][:, 0] == ORG + 8 + 5).all()


@pytest.mark.gpu
def test_shell_node_of_a_missing_block_still_latches_status_2(pol):
    """Status report, the face pass: a partition without margin built from particles in the blocks (4, 4, 4) and (3, 3, 4) holds the
    blocks (3, 4, 4) and (4, 5, 4) but not (3, 5, 4).  Eight particles are then put into block (4, 4, 4) just inside its -x face, y
    cell 6, moving -x.  They are movers into block (3, 4, 4), which exists: the producers report nothing and write one outbox record
    each.  Their terms reach the bin's arena through the list, at arena coordinate 0 of x; the nodes (x = -1, y = 8) of that face belong
    to block (3, 5, 4): the flush of the flagged face finds mass for a missing block and latches status[2].  Every core node of the bin
    (x = 0 .. 5, y up to 9: blocks (4, 4, 4) and (4, 5, 4)) exists, so the core pass cannot be what latches it."""
    from zpc_amd.mpm import MpmTransfer
    g = rng(6)
    n = 8
    p0 = ORG + 1.0 + 5.0 * g.random((n, 3))                           # first upload: defines the partition
    p0[n // 2:, :2] -= 8.0                                            # half of it in block (3, 3, 4)
    p1 = np.stack([ORG + 0.004 + 0.016 * g.random(n), ORG + 6.2 + 0.6 * g.random(n), ORG + 1.5 + 2.0 * g.random(n)], 1)
    mass = tag_masses(np.full(n, 1000.0 * VOL, np.float32))
    vel = np.tile(np.array([-0.12 * DX / DT, 0.0, 0.0], np.float32), (n, 1))
    Cm = np.zeros((n, 9), np.float32)
    F = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))
    mt = MpmTransfer(pol, n, DX, DT, model=0, side=8, volume=VOL, cache_stress=True)
    mt.upload(mass, ((p0 + 0.5) * DX).astype(np.float32), vel, Cm, F, None)
    mt.build_partition(n, margin=0)
    keys = {tuple(k) for k in (mt.active_keys().astype(np.int64) * (8 // mt.kstride) // 8).tolist()}
    b = ORG // 8
    assert {(b, b, b), (b - 1, b, b), (b, b + 1, b), (b - 1, b, b + 1), (b, b + 1, b + 1)} <= keys
    assert (b - 1, b + 1, b) not in keys and (b - 1, b + 1, b + 1) not in keys
    x1 = ((p1 + 0.5) * DX).astype(np.float32)
    mt.upload(mass, x1, vel, Cm, F, None)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, 0.0, 0.0))
    mt.slot(K=16, outbox_cap=64)
    mt.g2p2g(write_all=True)
    pol.syncCtx()
    assert int(mt.mover_count[:mt.nbins].sum().item()) == n        # every one a mover into another block
    st = mt.check_slots(strict=False)
    assert st[2] == 1, st
    assert st[0] == 0 and st[1] == 0 and st[4] == 0 and st[5] == st[6] == n, st
    c0, c1 = ref64.arena32(x1, DX)[0], ref64.arena32(mt.download()["x"], DX)[0]
    assert (c0[:, 0] == ORG).all() and (c1[:, 0] == ORG - 1).all() and (c1[:, 1] == ORG + 6).all()


if __name__ == "__main__":   # the golden file of the at-rest case, from the library ZS_ROCM_LIB names (see that test's docstring)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import zpc_amd
    st, world = at_rest_result(zpc_amd.rocm_exec())
    np.savez_compressed(sys.argv[1], coords=world[0].astype(np.int32), grid=world[1].astype(np.float32),
                        **{k: st[k] for k in ("m", "x", "v", "C", "F", "PF")})
