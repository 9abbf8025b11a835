"""The 8^3 block kernel of the slotted step re-slots a mover whose new cell lies in another bin of the SAME block itself (ticket of that
bin's LDS counter, state stored straight into the free round): only movers into another block leave an outbox record for
slot_rehome_kernel (zpc_amd/csrc/mpm_slot.hpp, slot_produce_entry; mpm_slotblk.hip)."""
import numpy as np
import pytest

from util import rng, make_drifting_cloud, make_full_cell_cloud, OracleMpm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _id_order(m, x):
    return np.lexsort((x[:, 2], x[:, 1], x[:, 0], m))


def _by_mass(d):
    o = _id_order(d["m"], d["x"])
    return {k: v[o] for k, v in d.items()}


def _base_cell(x, dx):
    """base node of a position as the kernels derive it (float32: X = x / dx, floor(X - 0.5))"""
    return np.floor(x.astype(np.float32) * np.float32(1.0 / dx) - np.float32(0.5)).astype(np.int64)


def _stored_cells(mt, dx):
    """(base cell of every stored particle, cell of the slot it is stored in), both in world cells"""
    lib = __import__("zpc_amd").lib()
    slots = torch.empty(mt.n_slots, dtype=torch.int32, device="cuda")
    cnt = int(lib.zs_rocm_mpm_slot_list(mt.pol.handle, mt.cell_mask.data_ptr(), mt.nbins, mt.K, slots.data_ptr()))
    mt.pol.syncCtx()
    i = slots[:cnt].cpu().numpy().astype(np.int64)
    buf = mt.buf.cpu().numpy()
    x = np.stack([buf[(i // 64) * 64 * mt.nchn + (mt.off["x"] + d) * 64 + i % 64] for d in range(3)], 1)
    bins = i // (mt.K * 64)
    lane = i % 64
    sub = bins % 8
    org = mt.active_keys().astype(np.int64)[bins // 8] * (mt.side // mt.kstride)
    loc = np.stack([4 * ((sub >> 2) & 1) + (lane >> 4), 4 * ((sub >> 1) & 1) + ((lane >> 2) & 3), 4 * (sub & 1) + (lane & 3)], 1)
    return _base_cell(x, dx), org + loc


def test_slotted_block_movers_across_bin_and_block_faces_vs_oracle(pol, oracle):
    """A cloud drifting ~0.1 cell per step on all three axes through 8^3 blocks: its particles cross bin faces inside blocks (cells 20 and
    28 of every axis) and block faces (cell 24).  Every step: the step against the oracle's g2p -> p2g sequence node for node, sent ==
    re-homed with status words 0, 1, 2, 4 clear, every particle stored under its own cell, the occupancy bits equal to the particle
    count, and the outbox records of the step (sum of moverCount) equal to the movers whose new cell lies in ANOTHER BLOCK, counted
    here from the positions before and after the step.  After the last step every particle agrees with the oracle."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt, side, model = 1.0 / 64, 1e-3, 8, 1
    mass, pos, vel, Cm, F = make_drifting_cloud()                      # identity-tagged, ~0.1 cell per step
    n = pos.shape[0]
    vol = dx ** 3 / 8
    lj = (0.01 * rng(7).standard_normal(n)).astype(np.float32)
    om = OracleMpm(oracle, model, dx, dt, side, vol)
    mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, lj)
    mt.build_partition(n, margin=1)
    om.adopt_partition(mt.active_keys())
    ljo = lj.copy()
    om.p2g(mass, pos, vel, Cm, F, ljo)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    om.grid_update((0.0, -9.8, 0.0))
    mt.grid_update((0.0, -9.8, 0.0))
    mt.slot(K=24, outbox_cap=512)
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    in_block = cross_block = 0
    prev = _by_mass(mt.download())
    for step in range(8):
        om.g2p(po, vo, Co, Fo)
        om.grid[:] = 0
        om.p2g(mass, po, vo, Co, Fo, ljo)
        mt.g2p2g(write_all=(step == 7))
        pol.syncCtx()
        mt.check_slots(strict=True)
        ga = mt.grid.cpu().numpy().reshape(om.grid.shape)
        scale = np.abs(om.grid).max(axis=(0, 2)) + 1e-30
        assert (np.abs(ga - om.grid).max(axis=(0, 2)) <= 3e-4 * scale).all(), (step, np.abs(ga - om.grid).max(axis=(0, 2)) / scale)
        om.grid_update((0.0, -9.8, 0.0))
        mt.grid_update((0.0, -9.8, 0.0))
        # storage after the commit: every particle once, under the cell of its base node
        cur = _by_mass(mt.download())
        assert np.array_equal(cur["m"], prev["m"]), step
        want, have = _stored_cells(mt, dx)
        assert want.shape[0] == n and np.array_equal(want, have), (step, int((want != have).any(axis=1).sum()))
        # outbox records of the step = movers into another block
        c0, c1 = _base_cell(prev["x"], dx), _base_cell(cur["x"], dx)
        moved = (c0 != c1).any(axis=1)
        other_block = moved & ((c0 >> 3) != (c1 >> 3)).any(axis=1)
        other_bin = moved & ((c0 >> 2) != (c1 >> 2)).any(axis=1)
        records = int(mt.mover_count[:mt.nbins].sum().item())
        assert records == int(other_block.sum()), (step, records, int(other_block.sum()), int(other_bin.sum()))
        in_block += int((other_bin & ~other_block).sum())
        cross_block += int(other_block.sum())
        prev = cur
    assert in_block > 100 and cross_block > 100, (in_block, cross_block)   # both kinds of mover were on the path, on every axis
    d = _by_mass(mt.download())
    o = _id_order(mass, po)
    assert np.array_equal(d["m"], mass[o])
    assert np.abs(d["x"] - po[o]).max() <= 2e-6
    assert np.abs(d["v"] - vo[o]).max() <= 2e-4 * np.abs(vo).max()
    assert np.abs(d["F"] - Fo[o]).max() <= 5e-5


def test_slotted_full_destination_cell_in_another_bin_of_the_block_keeps_the_mover(pol):
    """The same-block twin of test_slotted_full_destination_cell_in_another_bin_returns_the_mover: four particles just below the +x face
    of cell 35 (bin 0 of the block at cell 32) move into cell 36 (bin 4 of the same block), which holds K particles at rest.  The cell
    has no free round: the movers keep their old slots with their new state, status word [1] latches, no outbox record is written,
    sent == re-homed, and every particle is still stored."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt, side, K = 1.0 / 64, 1e-3, 8, 8
    mass, pos, vel, Cm, F = make_full_cell_cloud(dx, K)
    n = pos.shape[0]
    mt = MpmTransfer(pol, n, dx, dt, model=0, side=side, volume=dx ** 3 / 8, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, None)
    mt.build_partition(n, margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    mt.slot(K=K, outbox_cap=64)
    keys = mt.active_keys().astype(np.int64) * (side // mt.kstride)
    assert any((k == 32).all() for k in keys)   # the block at cell 32 holds both cells
    mt.g2p2g(write_all=True)
    pol.syncCtx()
    records = int(mt.mover_count[:mt.nbins].sum().item())
    st = mt.check_slots(strict=False)
    assert st[1], "the destination cell was not full: the test does not test"
    assert st[0] == 0 and st[2] == 0 and st[4] == 0, st
    assert st[5] == st[6], st
    assert records == 0, records
    d = _by_mass(mt.download())
    o = _id_order(mass, pos)
    assert np.array_equal(d["m"], mass[o])
    moved = _base_cell(d["x"], dx)[:, 0] == 36
    assert moved.sum() == n, _base_cell(d["x"], dx)   # the four movers did reach cell 36 (and are stored under cell 35)
    want, have = _stored_cells(mt, dx)
    assert int((want != have).any(axis=1).sum()) == 4
