"""The chunk lists of the 8^3 block kernel of the slotted step (blk_xlist_lds / blk_consumer, zpc_amd/csrc/mpm_slotblk.hip): ONE consumer
wave scatters a chunk's list -- movers into neighbour bins, arrival-queue overflow, stayers whose local position rounds to 1.5 -- into all
seven channels of the bin's 8^3 arena; the other three consumers add their register planes and flush only after that wave has finished
the list of the bin's last chunk, and the faces of the shell to flush reach them through LDS.

Every cloud is one 8^3 block with its margin, dx = 1/64, built from per-cell stayer counts (which fix the rounds of a bin: round r holds
the cells with more than r particles) and from movers placed within 0.02 cell of a cell or bin face, in the velocity field of
tests/test_slot_block_flush_gpu.py (0.12 cell per step, sign set by the next axis' coordinate).  The grid of every step is checked node
by node, all seven channels, against the float64 reference exactly as that module does (_checked_step: node-local bounds, untouched
nodes exactly 0); the stored particle state after the FIRST step -- which does not depend on the consumers, and reads a grid the unfused
kernels built -- is bit-identical in m, x and F to what the parent of this change stored (tests/golden/slot_block_list_parent.npz; v, C and
the stress of a write_all step are held by the float64 bounds: see _same_as_parent for why and for the figures).

T is the number of live lanes at or below which an iteration of the lane = cell loop would be handed to the list wave (`sparse rounds`,
profiles/block_list.md: measured as an experiment, not in the kernel); the threshold, tall-cell and straddle clouds are built around it, so
they are the right inputs for that step too."""
import os

import numpy as np
import pytest

import ref64
from util import rng, tag_masses, OracleMpm

DX = 1.0 / 64
DT = 1e-3
VOL = DX ** 3 / 8
ORG = 32
A_VEL = 0.12      # cells per step at the field's maximum
T = 12
SL_XQ = 64        # list entries per chunk (mpm_slot.hpp)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slot_block_list_parent.npz")


def _fl():
    import test_slot_block_flush_gpu as fl   # _slotted, _checked_step, crossings, shell_cloud: the checked step of that module
    return fl


# ---------------------------------------------------------------------------------------------------------------- cloud pieces
def _field(p):
    return np.cos(0.25 * np.pi * p)


def stayers(g, counts):
    """counts [8, 8, 8] particles per cell of the block -> block-local coordinates, 0.25 .. 0.75 inside their cells (0.12 cell of
    travel keeps them there)"""
    cells = np.argwhere(counts > 0)
    rep = np.repeat(cells, counts[counts > 0], axis=0)
    return rep + 0.25 + 0.5 * g.random(rep.shape)


def mover(g, d, s, plane, steer_cell, free_cell):
    """a particle within 0.004 .. 0.02 cell of the plane p_d = `plane`, on the side it leaves through it in direction s: the field's sign on
    axis d is set by the coordinate on axis e = d + 1 (cells 0, 7: +, cells 3, 4: -), which sits in `steer_cell`; axis d + 2 in free_cell"""
    assert (steer_cell in (0, 7)) == (s > 0) and (steer_cell in (3, 4)) == (s < 0)
    e, f = (d + 1) % 3, (d + 2) % 3
    eps = 0.004 + 0.016 * g.random()
    p = np.zeros(3)
    p[d] = plane - eps if s > 0 else plane + eps
    p[e] = steer_cell + 0.25 + 0.5 * g.random()
    p[f] = free_cell + 0.25 + 0.5 * g.random()
    return p


def finish(g, P, org=(ORG, ORG, ORG), still=None):
    """(mass, pos, vel, C, F) of block-local coordinates P (base node = floor(P)); still: mask of particles with v = 0 and C = 0"""
    P = np.asarray(P, np.float64)
    n = P.shape[0]
    pos = ((P + 0.5 + np.asarray(org, np.float64)) * DX).astype(np.float32)
    vel = np.ascontiguousarray(A_VEL * DX / DT * _field(P[:, [1, 2, 0]]), np.float32)
    Cm = (0.01 * g.standard_normal((n, 9))).astype(np.float32)
    if still is not None:
        vel[still] = 0
        Cm[still] = 0
    F = (np.eye(3).reshape(1, 9) + 1e-3 * g.standard_normal((n, 9))).astype(np.float32)
    mass = tag_masses(np.full(n, 1000.0 * VOL, np.float32))
    return mass, pos, vel, Cm, F


def rounds_counts(g, sizes, lo=(0, 0, 0)):
    """per-cell counts [8, 8, 8] that give the bin at cells lo .. lo + 3 the rounds `sizes` (non-increasing occupied-cell counts): a random
    nested choice of cells per round"""
    assert all(a >= b for a, b in zip(sizes, sizes[1:])) and sizes[0] <= 64
    order = g.permutation(64)
    cnt = np.zeros(64, np.int64)
    for s in sizes:
        cnt[order[:s]] += 1
    out = np.zeros((8, 8, 8), np.int64)
    out[lo[0]:lo[0] + 4, lo[1]:lo[1] + 4, lo[2]:lo[2] + 4] = cnt.reshape(4, 4, 4)
    return out


def bin_rounds(pos, org=(ORG, ORG, ORG)):
    """{bin of the block: occupied cells per round} of a cloud, from its base cells"""
    c = ref64.arena32(pos, DX)[0] - np.asarray(org)
    assert ((c >= 0) & (c < 8)).all()
    b = ((c[:, 0] >> 2) * 2 + (c[:, 1] >> 2)) * 2 + (c[:, 2] >> 2)
    lane = ((c[:, 0] & 3) * 4 + (c[:, 1] & 3)) * 4 + (c[:, 2] & 3)
    out = {}
    for k in np.unique(b):
        cnt = np.bincount(lane[b == k], minlength=64)
        out[int(k)] = [int((cnt > r).sum()) for r in range(cnt.max())]
    return out


# ---------------------------------------------------------------------------------------------------------------------- clouds
def threshold_cloud():
    """bin 0: rounds of 64, 64, 64, T + 1, T and 1 occupied cells -- both sides of the threshold in one chunk and one step; a few particles
    in the bin diagonally opposite.  Stayers only."""
    g = rng(31)
    cnt = rounds_counts(g, [64, 64, 64, T + 1, T, 1]) + rounds_counts(g, [9, 3], lo=(4, 4, 4))
    return finish(g, stayers(g, cnt))


def tall_cloud():
    """bin 0: one cell with 24 particles among cells of 1 - 2 (rounds 64, 40, then 22 rounds of one cell)"""
    g = rng(32)
    return finish(g, stayers(g, rounds_counts(g, [64, 40] + [1] * 22)))


def straddle_cloud(first_sparse):
    """bin 0 holds more than 256 entries and a sparse round (<= T cells) straddles entry 256, i.e. begins in the bin's first chunk and ends in
    its second.  first_sparse: the straddling round is the bin's first sparse one (entries 248 .. 259); else two sparse rounds precede it
    (232 .. 243, 244 .. 253, then 254 .. 261)."""
    g = rng(33 + first_sparse)
    sizes = [64, 64, 64, 56, 12, 5] if first_sparse else [64, 64, 64, 40, 12, 10, 8, 3]
    return finish(g, stayers(g, rounds_counts(g, sizes)))


MIXED_ORG = (-8, ORG, ORG)   # the block left of world x = 0: its cell 7 is world cell -1, where a local position can round to 1.5


def mixed_cloud():
    """One chunk (bin 4 of the block: cells 4 .. 7 on x, 0 .. 3 on y and z; 150 - 190 entries) whose list carries all four kinds:
      * stayers of sparse rounds (rounds 64, 64, 7, 2);
      * in-bin arrivals: movers across cell faces inside the bin, six of them into ONE cell (the queue of a cell takes four per chunk, the
        others take the list);
      * movers into a neighbour bin through each of the bin's 6 faces, 4 per face (into bins of the same block, and into the blocks at +x
        and -y);
      * a stayer at world X = 0.5 - 2^-25 on x (base cell -1 = cell 7 of the block; X - floor(X - 0.5) rounds to 1.5).  It must not move on
        x at all, so every particle whose stencil shares a node with it (cells 5 .. 7 x 1 .. 3 x 1 .. 3) is at rest with C = 0; gravity
        then moves them on y alone.
    Returns the cloud and the index of that stayer."""
    g = rng(35)
    P = [stayers(g, rounds_counts(g, [64, 64, 7, 2], lo=(4, 0, 0)))]
    mv = []
    for _ in range(4):
        mv += [mover(g, 0, -1, 4, 3, 0), mover(g, 0, +1, 8, 0, 0),      # x faces: into bin 0 / into the block at +x
               mover(g, 1, -1, 0, 3, 4), mover(g, 1, +1, 4, 0, 4),      # y faces: into the block at -y / into bin 6
               mover(g, 2, -1, 0, 4, 0), mover(g, 2, +1, 4, 7, 0)]      # z faces: into the block at -z / into bin 5
    for _ in range(6):
        mv.append(mover(g, 0, +1, 6, 0, 0))                             # in-bin: cell (5, 0, 0) -> (6, 0, 0), six into one cell
    mv += [mover(g, 1, +1, 2, 0, 4), mover(g, 1, +1, 3, 0, 4), mover(g, 2, +1, 2, 7, 0), mover(g, 0, -1, 6, 3, 0)]   # in-bin, other cells
    P.append(np.asarray(mv))
    P.append(np.array([[8.0 - 2.0 ** -25, 3.5, 3.5]]))
    P = np.concatenate(P)
    c = np.floor(P).astype(int)
    still = (c[:, 0] >= 5) & (c[:, 1] >= 1) & (c[:, 1] <= 3) & (c[:, 2] >= 1) & (c[:, 2] <= 3)
    cloud = finish(g, P, MIXED_ORG, still)
    assert cloud[1][-1, 0] == np.float32((0.5 - 2.0 ** -25) * DX)
    return cloud, P.shape[0] - 1


def overflow_cloud():
    """bin 0: rounds 64, 64, 9, 4 of stayers and 80 movers through its +x face into bin 4 of the block -- more than SL_XQ producer entries
    for the list of ONE chunk (the bin has 221 entries): the movers beyond the list's capacity leave a flagged outbox record, scattered
    after the chunk loop"""
    g = rng(36)
    P = [stayers(g, rounds_counts(g, [64, 64, 9, 4]))]
    P.append(np.asarray([mover(g, 0, +1, 4, 0, k % 4) for k in range(80)]))
    return finish(g, np.concatenate(P))


def two_bin_cloud():
    """bins 0 and 1 of the block (the two halves on z), one chunk each, back to back in the chunk sequence: the last chunk of the first
    and the first chunk of the second both carry lists (movers out of each bin through x, y and z faces, among them the face between the
    two), and sparse rounds"""
    g = rng(37)
    P = [stayers(g, rounds_counts(g, [64, 30, 6, 2]) + rounds_counts(g, [64, 41, 11, 3], lo=(0, 0, 4)))]
    mv = []
    for _ in range(6):
        mv += [mover(g, 0, +1, 4, 0, 1), mover(g, 0, +1, 4, 0, 6), mover(g, 0, -1, 0, 3, 2), mover(g, 0, -1, 0, 3, 5),
               mover(g, 1, +1, 4, 0, 1), mover(g, 1, -1, 0, 3, 2), mover(g, 1, -1, 0, 4, 1),
               mover(g, 2, +1, 4, 0, 1), mover(g, 2, -1, 4, 3, 2), mover(g, 2, +1, 8, 0, 2), mover(g, 2, -1, 0, 3, 1)]
    P.append(np.asarray(mv))
    return finish(g, np.concatenate(P))


CASES = {
    "threshold": (threshold_cloud, (ORG, ORG, ORG)),
    "tall": (tall_cloud, (ORG, ORG, ORG)),
    "straddle": (lambda: straddle_cloud(False), (ORG, ORG, ORG)),
    "straddle_first": (lambda: straddle_cloud(True), (ORG, ORG, ORG)),
    "mixed": (lambda: mixed_cloud()[0], MIXED_ORG),
    "overflow": (overflow_cloud, (ORG, ORG, ORG)),
    "two_bins": (two_bin_cloud, (ORG, ORG, ORG)),
}


def list_kinds(x0, x1):
    """what a step's particles ask of the lists, from the stored positions before and after it: movers into another bin, movers inside
    their bin (arrivals), the largest number of in-bin movers into one cell, stayers whose local position left [0.5, 1.5)"""
    c0, c1 = ref64.arena32(x0, DX)[0], ref64.arena32(x1, DX)[0]
    lpn = ref64.arena32(x1, DX)[1]
    moved = (c0 != c1).any(1)
    other_bin = ((c0 >> 2) != (c1 >> 2)).any(1)
    in_bin = moved & ~other_bin
    per_cell = np.unique(c1[in_bin], axis=0, return_counts=True)[1] if in_bin.any() else np.zeros(1, int)
    edge = ~moved & ~((lpn >= 0.5) & (lpn < 1.5)).all(1)
    return dict(other_bin=int(other_bin.sum()), in_bin=int(in_bin.sum()), most_into_one_cell=int(per_cell.max()), edge_stayers=int(edge.sum()),
                other_block=int(((c0 >> 3) != (c1 >> 3)).any(1).sum()))


# -------------------------------------------------------------------------------------------------------------------- no GPU
def test_the_clouds_have_the_rounds_and_the_lists_they_are_named_for(oracle):
    """No GPU.  The rounds of every cloud's bins, from its base cells, are the ones its docstring states -- the threshold, the tall cell,
    the straddled entry 256 -- and one step of the float32 CPU oracle moves the mixed, overflow and two-bin clouds as intended: every
    face of the mixed bin crossed, more than four arrivals into one cell, the stayer's local position on 1.5, more than SL_XQ list
    entries in the overflow chunk, movers out of both bins of the two-bin cloud."""
    r = bin_rounds(threshold_cloud()[1])
    assert r[0] == [64, 64, 64, T + 1, T, 1] and sorted(r) == [0, 7]
    r = bin_rounds(tall_cloud()[1])
    assert r[0] == [64, 40] + [1] * 22 and len(r[0]) == 24
    for first, sizes in ((False, [64, 64, 64, 40, 12, 10, 8, 3]), (True, [64, 64, 64, 56, 12, 5])):
        r = bin_rounds(straddle_cloud(first)[1])[0]
        assert r == sizes and sum(r) > 256
        start = np.concatenate([[0], np.cumsum(r)])
        strad = [k for k in range(len(r)) if start[k] < 256 < start[k + 1]]
        assert len(strad) == 1 and r[strad[0]] <= T
        assert (min(k for k in range(len(r)) if r[k] <= T) == strad[0]) == first

    def oracle_step(cloud, org):
        mass, pos, vel, Cm, F = cloud
        om = OracleMpm(oracle, 0, DX, DT, 8, VOL)
        k0 = np.asarray(org) // 8
        keys = np.stack(np.meshgrid(*[np.arange(k - 1, k + 2) for k in k0], indexing="ij"), -1).reshape(-1, 3)
        om.adopt_partition(keys)
        om.p2g(mass, pos, vel, Cm, F)
        om.grid_update(_fl().G)
        po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
        om.g2p(po, vo, Co, Fo)
        return po

    (cloud, stayer) = mixed_cloud()
    assert bin_rounds(cloud[1], MIXED_ORG).keys() == {4}
    po = oracle_step(cloud, MIXED_ORG)
    k = list_kinds(cloud[1], po)
    cr = _fl().crossings(cloud[1], po)
    assert all(cr["face%d" % f] >= 3 for f in range(6)), cr
    assert k["most_into_one_cell"] > 4 and k["in_bin"] >= 8 and k["edge_stayers"] >= 1 and k["other_block"] >= 6, k
    assert po[stayer, 0] == cloud[1][stayer, 0] and ref64.arena32(po[stayer:stayer + 1], DX)[1][0, 0] == 1.5
    assert k["other_bin"] + k["most_into_one_cell"] - 4 + k["edge_stayers"] > 2     # longer than one pass of two entries
    cloud = overflow_cloud()
    assert sum(bin_rounds(cloud[1])[0]) <= 256
    assert list_kinds(cloud[1], oracle_step(cloud, (ORG,) * 3))["other_bin"] > SL_XQ
    cloud = two_bin_cloud()
    assert bin_rounds(cloud[1]).keys() == {0, 1}
    po = oracle_step(cloud, (ORG,) * 3)
    c0 = ref64.arena32(cloud[1], DX)[0] - ORG
    left = ((c0 >> 2) != ((ref64.arena32(po, DX)[0] - ORG) >> 2)).any(1)
    assert left[c0[:, 2] < 4].sum() >= 10 and left[c0[:, 2] >= 4].sum() >= 10


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _state(mt):
    t = _fl()._helpers()
    return t._by_mass(t._fields(t._read_all(mt), mt))


STATE_KEYS = ("m", "x", "F")


def _same_as_parent(name, state):
    """The particle state the step stores (m, x, F) after the first step is the parent's, bit for bit.

    Not v, C and the stress of a write_all step, although the fixture holds them: the step's G2P half reads a grid that the unfused P2G built
    with float atomics from several workgroups, and the order of those sums changes from run to run.  Measured with the PARENT library on
    the at-rest cloud of tests/test_slot_block_flush_gpu.py, whose 8 bins share nodes: in 2 of 4 fresh processes the stored v differed
    from the recorded one in its last bits, with the library of this change in 1 of 4 (x and F never did, in more than 20 runs of either
    library: a last bit of v times dt is far below an ulp of x).  v and C are
    held per particle by the float64 G2P bounds of _checked_step instead, the stress by its P2G check."""
    gold = np.load(GOLDEN)
    for k in STATE_KEYS:
        assert np.array_equal(state[k].view(np.uint32), gold[name + "_" + k].view(np.uint32)), (name, k)


def _run(pol, oracle, name, write_all, steps=1):
    fl = _fl()
    cloud = CASES[name][0]()
    mt = fl._slotted(pol, cloud)
    om = OracleMpm(oracle, 0, DX, DT, 8, VOL)
    out = []
    for step in range(steps):
        wa = write_all if steps == 1 else step == 1
        before, after, world, _ = fl._checked_step("list[%s wa%d] step %d" % (name, wa, step), mt, om, wa)
        if step == 0:
            _same_as_parent(name, _state(mt))
        out.append((before, after, world))
    return mt, out


@pytest.mark.gpu
@pytest.mark.parametrize("write_all", [True, False])
@pytest.mark.parametrize("name", ["threshold", "tall", "straddle", "straddle_first"])
def test_sparse_rounds_on_both_sides_of_the_threshold_a_tall_cell_and_the_straddled_chunk_boundary(pol, oracle, name, write_all):
    """Stayers only: the rounds of T + 1, T and 1 cells in one chunk; the cell of 24 among cells of 1 - 2; the sparse round that straddles
    entry 256 of its bin (as the first sparse round, and behind two others).  All 7 channels within the node-local bounds, untouched nodes
    exactly 0, nobody moves, particle state as the parent stored it."""
    mt, out = _run(pol, oracle, name, write_all)
    before, after, _ = out[0]
    assert _fl().crossings(before["x"], after["x"])["cell"] == 0
    assert int(mt.mover_count[:mt.nbins].sum().item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("write_all", [True, False])
def test_one_list_with_sparse_stayers_arrivals_neighbour_bin_movers_and_a_stayer_on_1_5(pol, oracle, write_all):
    """The mixed cloud: the list of its one chunk holds movers through all 6 faces of the bin (the shell is reached on every face), the
    arrivals beyond a cell's queue and the stayer whose local position is 1.5, beside sparse rounds and queued arrivals -- counted
    from the stored positions; the grid is within the bounds on all 7 channels."""
    mt, out = _run(pol, oracle, "mixed", write_all)
    before, after, _ = out[0]
    k = list_kinds(before["x"], after["x"])
    cr = _fl().crossings(before["x"], after["x"])
    print("LIST mixed", k, cr)
    assert all(cr["face%d" % f] >= 3 for f in range(6)), cr
    assert k["most_into_one_cell"] > 4 and k["in_bin"] >= 8 and k["edge_stayers"] >= 1 and k["other_block"] >= 6, k
    assert k["other_bin"] + k["most_into_one_cell"] - 4 + k["edge_stayers"] <= SL_XQ


@pytest.mark.gpu
@pytest.mark.parametrize("write_all", [True, False])
def test_more_producer_entries_than_the_list_holds_fall_back_to_records(pol, oracle, write_all):
    """More than SL_XQ movers into a neighbour bin in one chunk, with sparse rounds: the list takes SL_XQ, the others leave flagged outbox
    records although their new bin is in the same block (so there are more records than movers into other blocks), every term still
    reaches the grid (the bounds), and the status words are as ever: no flag, sent == re-homed (_checked_step)."""
    mt, out = _run(pol, oracle, "overflow", write_all)
    before, after, _ = out[0]
    k = list_kinds(before["x"], after["x"])
    records = int(mt.mover_count[:mt.nbins].sum().item())
    print("LIST overflow", k, "records", records)
    assert k["other_bin"] > SL_XQ and k["other_block"] == 0
    assert records == k["other_bin"] - SL_XQ


@pytest.mark.gpu
def test_lists_in_two_bins_back_to_back_over_three_steps(pol, oracle):
    """Bins 0 and 1 of the block, one chunk each, lists in both: the first bin's flush must wait for the list wave, and the second bin's
    list must find the arena zero.  Three steps: the grid within the bounds with exact zeros at untouched nodes every step (a shell node
    flushed before its list term arrived would surface in the NEXT bin or step as a stray value), the particle count unchanged, the mass
    sum within MASS_SUM_RTOL of tests/test_slot_block_flush_gpu.py."""
    fl = _fl()
    mt, out = _run(pol, oracle, "two_bins", True, steps=3)
    n = out[0][0]["m"].shape[0]
    left = 0
    for step, (before, after, world) in enumerate(out):
        assert after["m"].shape[0] == n
        c0 = ref64.arena32(before["x"], DX)[0]
        left += int(((c0 >> 2) != (ref64.arena32(after["x"], DX)[0] >> 2)).any(1).sum())
        total, want = world[1][:, 0].sum(), after["m"].astype(np.float64).sum()
        print("LIST two bins, mass sum step %d: rel. difference %.3g" % (step, abs(total - want) / want))
        assert abs(total - want) <= fl.MASS_SUM_RTOL * want, (step, total, want)
    assert left >= 40, left


@pytest.mark.gpu
def test_at_rest_nothing_goes_through_the_list_and_the_result_is_the_stored_one(pol, oracle):
    """The shell cloud of tests/test_slot_block_flush_gpu.py at rest: no mover, empty lists, no face flushed; all 7 channels within the
    node-local bound of the grid stored in tests/golden/slot_block_flush_at_rest.npz, the stored particle state (m, x, F) bit-identical to it."""
    fl = _fl()
    om = OracleMpm(oracle, 0, DX, DT, 8, VOL)
    mt = fl._slotted(pol, fl.shell_cloud(at_rest=True))
    before, after, world, bound = fl._checked_step("list[at rest]", mt, om, True)
    assert fl.crossings(before["x"], after["x"])["cell"] == 0
    assert int(mt.mover_count[:mt.nbins].sum().item()) == 0
    gold = np.load(fl.GOLDEN)
    state = _state(mt)
    for k in STATE_KEYS:   # (v, C and the stress: see _same_as_parent)
        assert np.array_equal(state[k].view(np.uint32), gold[k].view(np.uint32)), k
    assert np.array_equal(world[0], gold["coords"])
    assert (np.abs(world[1] - gold["grid"]) <= bound).all()


if __name__ == "__main__":   # the parent's particle states (GOLDEN), from the library ZS_ROCM_LIB names: python tests/<this file> OUT.npz
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import zpc_amd
    pol_ = zpc_amd.rocm_exec()
    rec = {}
    for name_ in CASES:
        mt_ = _fl()._slotted(pol_, CASES[name_][0]())
        mt_.step_slotted(_fl().G, write_all=True)
        pol_.syncCtx()
        mt_.check_slots()
        st_ = _state(mt_)
        rec.update({name_ + "_" + k: st_[k] for k in ("m", "x", "v", "C", "F", "PF")})
    np.savez_compressed(sys.argv[1], **rec)
