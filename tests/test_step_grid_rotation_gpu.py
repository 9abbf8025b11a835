"""Three-grid rotation of the fused slotted step with 8^3 blocks (zs_rocm_mpm_step.gridClear / gridBIsClear, blk_clear_block in
zpc_amd/csrc/mpm_slotblk.hip): while a step gathers from grid A and scatters into grid B, every workgroup of the block kernel writes zero
over its own block of a third grid C, which is the next step's target -- no memset between the steps.

The scene (rotation_scene): the shell cloud of tests/test_slot_block_flush_gpu.py -- 446 particles in the one 8^3 block at cells 32..39,
movers through every face, edge and corner of its bins -- plus a single particle in the block diagonally behind it (cells 40..47), in the
partition build_partition(margin=1) makes of the two: 2 populated blocks, the rest empty apron blocks that leave the block kernel at its
early exit.

What bounds the grids of two runs that differ in the clear alone: they add the same float32 terms in another order.  A node's sum of N
terms of magnitude sum T is within (N - 1) u T of the exact sum in any order; the tests hold the two runs' difference to ref64's
node-local (N + c) u T of tests/ref64.py (c = 12 / 19 / 23 roundings inside a term), taken from the stored particle state WITHOUT the
propagated input errors the flush tests add to it (narrower than theirs), and carried through the grid update for the velocity channels
as grid_update64 does."""
import ctypes as C

import numpy as np
import pytest

import ref64
from util import tag_masses
from test_slot_block_flush_gpu import shell_cloud, DX, DT, G, VOL, ORG, MASS_SUM_RTOL

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BLK = 7 * 512    # floats of one 8^3 block


def _t():
    import test_mpm_ref64_gpu as t
    return t


def rotation_scene(model=0):
    """(mass, pos, vel, C, F, logJp): shell_cloud() and one more particle at rest in the block at cells 40..47 of every axis"""
    t = _t()
    mass, pos, vel, Cm, F, _ = shell_cloud()
    assert pos.shape[0] == 446
    one = ((np.array([[4.3, 3.6, 2.4]]) + 0.5 + ORG + 8) * DX).astype(np.float32)
    pos = np.concatenate([pos, one])
    vel = np.concatenate([vel, np.zeros((1, 3), np.float32)])
    Cm = np.concatenate([Cm, np.zeros((1, 9), np.float32)])
    F = np.concatenate([F, np.eye(3, dtype=np.float32).reshape(1, 9)])
    n = pos.shape[0]
    mass = tag_masses(np.full(n, 1000.0 * VOL, np.float32))
    F, lj = t._state(model, F, n)
    return mass, pos, vel, Cm, F, lj


def _slotted(pol, model=0, side=8, rotate=True, first=None):
    """the scene on slotted storage, ready for step_slotted; first(keys) -> bool mask: those blocks are numbered first (n_boundary)"""
    from zpc_amd.mpm import MpmTransfer
    t = _t()
    mass, pos, vel, Cm, F, lj = rotation_scene(model)
    n = pos.shape[0]
    mt = MpmTransfer(pol, n, DX, DT, model=model, side=side, volume=VOL, cache_stress=True, **t._kw(model))
    mt.rotate_grids = rotate
    mt.upload(mass, pos, vel, Cm, F, lj if model in (1, 3) else None)
    mt.build_partition(n, margin=1)
    mt.n_first = mt.reorder_partition(first(mt.active_keys() // mt.kstride)) if first is not None else 0
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update(G)
    mt.slot(K=32, outbox_cap=512)
    return mt


def _state_of(mt):
    t = _t()
    return t._by_mass(t._fields(t._read_all(mt), mt))


def _stress(mt, F, lj):
    """the GPU's own zs_rocm_mpm_stress of copies of (F, logJp): the magnitude of the force terms"""
    from zpc_amd import lib
    n = len(F)
    Fd = torch.from_numpy(np.ascontiguousarray(F, np.float32)).cuda()
    ljd = torch.from_numpy(np.ascontiguousarray(lj if lj is not None else np.zeros(n), np.float32)).cuda()
    PF = torch.empty(n, 9, device="cuda")
    lib().zs_rocm_mpm_stress(mt.pol.handle, C.byref(mt.params), Fd.data_ptr(), ljd.data_ptr(), n, PF.data_ptr())
    mt.pol.syncCtx()
    return PF.cpu().numpy()


def _order_bound(mt, grid_before, before, after, world):
    """[nodes of `world`, 7]: the node-local bound of the step that took `before` (and the node velocities grid_before) to `after` --
    mass and force: (N + c) u T of p2g64 on the stored particles; velocities: that bound through grid_update64.  0 at untouched nodes."""
    r = ref64.g2p64((grid_before[0], grid_before[1][:, 1:4]), before["x"], DX, DT, F=before["F"])
    PF = _stress(mt, after["F"], before.get("logJp"))
    ref = ref64.p2g64(after["m"], after["x"], r["v"], r["C"], DX, DT, PF=PF)
    b = ref.bound()
    _, bv = ref64.grid_update64(ref.val[:, 0], ref.val[:, 1:4], DT, G, b[:, 0], b[:, 1:4])
    rows = ref.lookup(world[0])
    sel = rows >= 0
    out = np.zeros_like(world[1])
    out[sel] = np.concatenate([b[rows[sel], :1], bv[rows[sel]], b[rows[sel], 4:]], 1)
    return out


def _dirty(t, value=-3.25):
    t.fill_(value)
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int32)


def test_clear_is_complete_and_stays_inside_the_partition(pol):
    """One step with a clear grid full of a non-zero pattern and one guard block behind it: afterwards every float of every block of
    [0, nblocks) is +0.0 bit for bit -- the two populated blocks through the kernel's tail, the apron blocks through its early exit --
    and the guard block still holds the pattern."""
    mt = _slotted(pol)
    nb = mt.nblocks
    populated = int((mt.cell_mask.view(nb, 512) != 0).any(1).sum().item())
    assert populated == 2 and nb > 8, (populated, nb)
    big = torch.empty((nb + 1) * BLK, dtype=torch.float32, device="cuda")
    _dirty(big)
    mt.grid3 = big[:nb * BLK]
    mt.step_slotted(G)
    mt.pol.syncCtx()
    mt.check_slots()
    assert mt.grid2 is not None and mt.grid2.data_ptr() == big.data_ptr()      # the cleared grid is the next target
    per_block = (_bits(big[:nb * BLK]).view(nb, BLK) != 0).sum(1)
    assert int(per_block.sum().item()) == 0, per_block.nonzero().flatten().tolist()[:8]
    assert bool((big[nb * BLK:] == -3.25).all().item())


def _hand_over(src, dst):
    """dst starts its next step from src's state, bit for bit: slot buffer, occupancy words, the grid to gather from, mover and status words"""
    for name in ("buf", "cell_mask", "grid", "slot_status", "mover_count", "mover_dest"):
        getattr(dst, name).copy_(getattr(src, name))
    torch.cuda.synchronize()


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_three_rotated_steps_equal_three_steps_with_the_memset(pol, model):
    """Three consecutive steps (write_all off, on, off) with the rotation -- one object, no memset after its first step -- against three
    steps of the memset path (gridClear = NULL): x, F and logJp of every particle bit-identical after every step, all 7 grid channels
    within the node-local bound of the module docstring (0 at untouched nodes: exact zeros in both), and the mass channel of either run
    sums to sum(m) within the flush tests' MASS_SUM_RTOL.

    The particles of a step depend on the gathered velocities alone, so they are bit-identical exactly when the two paths gather the same
    bits.  Two objects stepped side by side do not: the float atomics that sum a grid do not run in the same order twice, and already two
    runs of the MEMSET path differ from each other -- measured on the MI355X with this scene, memset against memset: 251 differing grid
    words after the first step and 434 differing words of F after the second (fixed-corotated), 601 grid words and 174 words of F after
    the first (Drucker-Prager; there the unfused P2G that primes the grid differs as well).  So before every step the memset object takes
    over the rotated object's state bit for bit (_hand_over); the rotated object runs its three steps on its own."""
    a, b = _slotted(pol, model, rotate=True), _slotted(pol, model, rotate=False)
    targets = []
    for step in range(3):
        grid_before = ref64.to_world_nodes(a)
        before = _state_of(a)
        _hand_over(a, b)
        for mt in (a, b):
            targets.append((mt.rotate_grids, mt.grid2.data_ptr() if mt.grid2 is not None else 0,
                            mt._clean_grid is not None and mt._clean_grid[0] is mt.grid2))
            mt.step_slotted(G, write_all=step == 1)
            mt.pol.syncCtx()
            st = mt.check_slots()
            assert st[5] == st[6], st
        sa, sb = _state_of(a), _state_of(b)
        for k in ("m", "x", "F") + (("logJp",) if model in (1, 3) else ()):
            diff = int((sa[k].view(np.uint32) != sb[k].view(np.uint32)).sum())
            print("ROTATION model %d step %d: %s differs in %d words" % (model, step, k, diff))
            assert diff == 0, (step, k, diff)
        wa, wb = ref64.to_world_nodes(a), ref64.to_world_nodes(b)
        assert np.array_equal(wa[0], wb[0])
        bound = _order_bound(a, grid_before, before, sa, wa)
        err = np.abs(wa[1] - wb[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)
        print("ROTATION model %d step %d: worst |rotated - memset| / bound per channel: %s" % (model, step, " ".join("%.3f" % x for x in ratio.max(0))))
        assert (err <= bound).all(), (step, ratio.max(0))
        ma, mb, want = wa[1][:, 0].sum(), wb[1][:, 0].sum(), sa["m"].astype(np.float64).sum()
        print("ROTATION model %d step %d: mass sums off sum(m) by %.3g (rotated) %.3g (memset)" % (model, step, abs(ma - want) / want, abs(mb - want) / want))
        assert abs(ma - want) <= MASS_SUM_RTOL * want and abs(mb - want) <= MASS_SUM_RTOL * want
    # the rotated run took its targets without a memset from the second step on; the other one never had a clean target
    rot = [t for t in targets if t[0]]
    assert [t[2] for t in rot] == [False, True, True] and len({t[1] for t in rot}) == 3
    assert not any(t[2] for t in targets if not t[0])


def single_range(pol, like):
    """(grid as world nodes, node-local bound, particle state) after one plain single-range step that starts from the bits `like` starts
    from (_hand_over: two objects set up alike still differ in the last bits of the grid their unfused P2G primes, see
    test_three_rotated_steps_equal_three_steps_with_the_memset, and the force terms mu (F - R) amplify a last bit of F far beyond a
    bound that is taken from their magnitude)"""
    mt = _slotted(pol, first=_near)
    _hand_over(like, mt)
    grid_before = ref64.to_world_nodes(mt)
    before = _state_of(mt)
    mt.step_slotted(G)
    mt.pol.syncCtx()
    mt.check_slots()
    after = _state_of(mt)
    world = ref64.to_world_nodes(mt)
    return world, _order_bound(mt, grid_before, before, after, world), after


def _near(kb):
    """the blocks numbered first: the upper layers of the partition on y -- the lone particle's block and apron blocks around it, while
    the shell cloud's block stays in the interior range and sends movers into them"""
    return kb[:, 1] >= ORG // 8 + 1


@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_every_range_schedule_clears_every_block_once(pol, schedule):
    """IN_TURN, SIDE_BY_SIDE and ONE_LAUNCH of the overlapped step on one GPU (world-size-1 communicator, the exchange of a few boundary
    blocks with this rank itself into a scratch grid, as bench.py --rank-proxy does): the clear grid is all zero after the step, the
    guard block behind it untouched, the grid within the single-range step's bound and the particles bit-identical to it."""
    import zpc_amd
    from zpc_amd.dist import NativeComm, NativeHaloPlan
    mt = _slotted(pol, first=_near)
    world0, bound, after0 = single_range(pol, mt)
    nb, nbd = mt.nblocks, mt.n_first
    assert 0 < nbd < nb
    populated = (mt.cell_mask.view(nb, 512) != 0).any(1).cpu().numpy()
    assert populated[:nbd].sum() == 1 and populated[nbd:].sum() == 1      # one populated block in either range
    comm = NativeComm(0, 1, 0, None)
    shared = np.arange(0, nbd, 2, dtype=np.int32)
    plan = NativeHaloPlan.from_lists(comm, 8, [(0, 0, shared.shape[0])], shared)
    scratch = torch.zeros_like(mt.grid)
    stream = torch.cuda.Stream(priority=-1)
    pol_comm = zpc_amd.rocm_exec().sync(False).external_stream(stream.cuda_stream)
    big = torch.empty((nb + 1) * BLK, dtype=torch.float32, device="cuda")
    _dirty(big)
    mt.grid3 = big[:nb * BLK]
    mt.step_slotted(G, n_boundary=nbd, comm=comm, plan=plan, comm_pol=pol_comm, halo_grid=scratch, halo_channels=4, range_schedule=schedule)
    mt.pol.syncCtx()
    torch.cuda.synchronize()
    mt.check_slots()
    assert int((_bits(big[:nb * BLK]) != 0).sum().item()) == 0
    assert bool((big[nb * BLK:] == -3.25).all().item())
    world = ref64.to_world_nodes(mt)
    assert np.array_equal(world[0], world0[0])
    err = np.abs(world[1] - world0[1])
    assert (err <= bound).all(), (schedule, (err / np.where(bound > 0, bound, 1)).max(0))
    after = _state_of(mt)
    for k in ("m", "x", "F"):
        assert np.array_equal(after[k].view(np.uint32), after0[k].view(np.uint32)), k


def test_a_dirty_target_without_the_flag_is_cleared_as_before(pol):
    """gridBIsClear = 0 (the first step of an object): a target full of garbage gives the single-range result -- the call's memset ran"""
    mt = _slotted(pol, first=_near)
    world0, bound, after0 = single_range(pol, mt)
    mt.grid2 = torch.empty_like(mt.grid)
    _dirty(mt.grid2, 7.5)
    assert mt._clean_grid is None
    mt.step_slotted(G)
    mt.pol.syncCtx()
    mt.check_slots()
    world = ref64.to_world_nodes(mt)
    assert (np.abs(world[1] - world0[1]) <= bound).all()
    assert np.array_equal(_state_of(mt)["x"].view(np.uint32), after0["x"].view(np.uint32))


def test_the_flag_is_what_skips_the_memset(pol):
    """the other direction, through the C call: with gridClear set and gridBIsClear = 1 a pattern in untouched nodes of the target
    survives the step (nothing cleared it: the caller vouched for the target), with gridBIsClear = 0 it is gone"""
    for flag in (1, 0):
        mt = _slotted(pol)
        nb = mt.nblocks
        populated = (mt.cell_mask.view(nb, 512) != 0).any(1)
        far = int((~populated).nonzero().flatten()[-1].item())    # an apron block; is it out of every stencil's reach?
        mt.grid2 = torch.zeros_like(mt.grid)
        mt.grid2.view(nb, BLK)[far, 5] = 11.0
        torch.cuda.synchronize()
        mt._clean_grid = (mt.grid2, mt.table) if flag else None
        mt.step_slotted(G)
        mt.pol.syncCtx()
        mt.check_slots()
        got = float(mt.grid.view(nb, BLK)[far, 5].item())
        assert got == (11.0 if flag else 0.0), (flag, got)


def test_first_step_after_a_repartition_clears_with_a_memset(pol):
    """repartition_slotted() drops the flag: a pattern written into the would-be target afterwards is cleared by the next step (grid
    nodes no particle reaches are 0), and the step after that rotates again"""
    mt = _slotted(pol)
    for _ in range(2):
        mt.step_slotted(G)
    mt.pol.syncCtx()
    assert mt._clean_grid is not None and mt._clean_grid[0] is mt.grid2
    mt.repartition_slotted()
    assert mt._clean_grid is None
    _dirty(mt.grid2, 9.0)
    _dirty(mt.grid3, 9.0)
    mt.step_slotted(G)
    mt.pol.syncCtx()
    mt.check_slots()
    g = mt.grid.view(mt.nblocks, 7, 512)
    assert int((g == 9.0).sum().item()) == 0
    assert mt._clean_grid is not None and mt._clean_grid[0] is mt.grid2
    assert int((_bits(mt.grid2) != 0).sum().item()) == 0                   # ... which the step has cleared in the kernel
    mt.step_slotted(G)
    mt.pol.syncCtx()
    mt.check_slots()
    assert int((mt.grid.view(mt.nblocks, 7, 512) == 9.0).sum().item()) == 0


def test_side_4_ignores_grid_clear(pol):
    """4^3 blocks: the per-bin kernel does not clear.  The C call with gridClear set and gridBIsClear = 1 on a target full of garbage:
    the clear grid keeps its pattern, and the target was cleared by the memset all the same -- no garbage left, exact zeros exactly
    where a plain step of the same scene has them."""
    from zpc_amd import lib
    from zpc_amd._lib import MpmStep
    b = _slotted(pol, side=4)
    b.step_slotted(G)
    b.pol.syncCtx()
    c = _slotted(pol, side=4)
    assert c.grid3 is None and c.nblocks == b.nblocks
    third, target = torch.empty_like(c.grid), torch.empty_like(c.grid)
    _dirty(third, 4.0)
    _dirty(target, 6.0)
    args = MpmStep()
    args.params, args.particles, args.table = C.addressof(c.params), c.particles(), c.table.handle
    args.gridA, args.gridB, args.nblocks, args.storage = c.grid.data_ptr(), target.data_ptr(), c.nblocks, C.addressof(c.slot_storage)
    args.extf = (C.c_float * 3)(*G)
    args.gridClear, args.gridBIsClear = third.data_ptr(), 1
    assert lib().zs_rocm_mpm_step_slotted(c.pol.handle, C.byref(args)) == 0
    c.pol.syncCtx()
    torch.cuda.synchronize()
    c.check_slots()
    assert bool((third == 4.0).all().item())
    gb, gc = b.grid.cpu().numpy(), target.cpu().numpy()
    assert (gb == 0).sum() > gb.size // 2 and ((gb == 0) == (gc == 0)).all()
