"""The step call's three-grid rotation, the parts that need no GPU: where zs_rocm_mpm_step keeps gridClear / gridBIsClear (header against
the ctypes mirror), and MpmTransfer's bookkeeping of which grid buffer is known to be clear, with the library's entry points replaced by a
recorder."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_clear_fields_of_the_step_struct_match_the_header(tmp_path):
    """gridClear (a pointer) and gridBIsClear (an int) sit at the offsets the host compiler gives them in include/zs_rocm.h, in that order,
    directly in front of `levelset`, which stays the struct's last member (tests/test_levelset_cpu.py pins that); every field in front of
    them keeps the offset it had."""
    from zpc_amd import _lib
    names = [m for m, _ in _lib.MpmStep._fields_]
    assert names[-3:] == ["gridClear", "gridBIsClear", "levelset"] and names[-4] == "handoverSnapshot"
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "zs_rocm.h"', 'int main(void) {',
           '  printf("size|%zu|0\\n", sizeof(zs_rocm_mpm_step));']
    for m in names:
        src.append('  printf("%s|%%zu|%%zu\\n", offsetof(zs_rocm_mpm_step, %s), sizeof(((zs_rocm_mpm_step *)0)->%s));' % (m, m, m))
    src += ['  return 0;', '}']
    c = tmp_path / "step.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "step"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        m, a, b = line.split("|")
        got[m] = [int(a), int(b)]
    assert C.sizeof(_lib.MpmStep) == got["size"][0]
    for m in names:
        f = getattr(_lib.MpmStep, m)
        assert [f.offset, f.size] == got[m], (m, [f.offset, f.size], got[m])
    S = _lib.MpmStep
    assert S.gridClear.size == C.sizeof(C.c_void_p) and S.gridBIsClear.size == C.sizeof(C.c_int)
    assert S.handoverSnapshot.offset + S.handoverSnapshot.size == S.gridClear.offset
    assert S.gridClear.offset + S.gridClear.size == S.gridBIsClear.offset < S.levelset.offset
    # a zero-initialised struct asks for the old behaviour
    z = S()
    assert not z.gridClear and z.gridBIsClear == 0


class _Recorder:
    """stands in for the loaded library: every entry point returns 0 and is recorded; the step call keeps a copy of its grid arguments"""

    def __init__(self):
        self.calls, self.steps = [], []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append(name)
            if name == "zs_rocm_mpm_step_slotted":
                a = args[1]._obj
                self.steps.append((a.gridA, a.gridB, a.gridClear, a.gridBIsClear))
            return 0
        return f


class _Table:
    handle = None


@pytest.fixture
def host_transfer(monkeypatch):
    """an MpmTransfer on host memory in the state slot() leaves it in (8^3 blocks), and the recorder its calls go to"""
    torch = pytest.importorskip("torch")
    from zpc_amd import mpm, _lib

    def make(side=8, nblocks=3):
        rec = _Recorder()
        monkeypatch.setattr(mpm, "lib", lambda: rec)
        mt = mpm.MpmTransfer.__new__(mpm.MpmTransfer)
        mt.__dict__.update(pol=type("P", (), {"handle": None})(), n=64, L=64, side=side, device=torch.device("cpu"), model=0, fluid=False, nF=9,
                           nchn=25, off={"m": 0, "x": 1, "v": 4, "C": 7, "F": 16, "logJp": 25}, cache_stress=False, aos=False,
                           params=_lib.MpmParams(), table=_Table(), nblocks=nblocks, slotted=True, n_slots=64, K=1,
                           buf=torch.zeros(64 * 25), slot_storage=_lib.SlotStorage(), grid=torch.zeros(nblocks * 7 * side ** 3),
                           grid2=None, grid3=None, _clean_grid=None, rotate_grids=True)
        mt.grid3 = torch.empty_like(mt.grid) if side == 8 else None      # (slot() allocates it)
        return mt, rec
    return make


def test_step_slotted_rotates_three_buffers_and_vouches_only_for_what_the_last_step_cleared(host_transfer):
    mt, rec = host_transfer()
    for _ in range(5):
        mt.step_slotted()
    A, B, Cl, flag = zip(*rec.steps)
    assert list(flag) == [0, 1, 1, 1, 1]                                   # the first target was never cleared by a step
    for k in range(5):
        assert len({A[k], B[k], Cl[k]}) == 3 and Cl[k] % 16 == 0
        if k:
            assert A[k] == B[k - 1] and B[k] == Cl[k - 1] and Cl[k] == A[k - 1]   # gather what was written, scatter into what was cleared
    assert (A[3], B[3], Cl[3]) == (A[0], B[0], Cl[0])
    assert mt.grid.data_ptr() == B[4] and mt.grid2.data_ptr() == Cl[4] and mt.grid3.data_ptr() == A[4]   # mt.grid: what the last step wrote
    assert "zs_rocm_memset" not in rec.calls                               # (the step's memset lives inside the C call)


@pytest.mark.parametrize("touch", ["clear_grid", "grid_update", "p2g", "_grids_written", "new_table", "swap_target", "no_rotation"])
def test_anything_that_touches_a_grid_or_the_partition_withdraws_the_flag_for_one_step(host_transfer, touch):
    mt, rec = host_transfer()
    mt.step_slotted()
    mt.step_slotted()
    assert rec.steps[-1][3] == 1
    if touch in ("clear_grid", "grid_update", "_grids_written"):
        getattr(mt, touch)()
    elif touch == "p2g":
        mt.binned, mt.nbr = False, None
        mt.p2g()
    elif touch == "new_table":            # the buffer was cleared under another partition
        mt.table = _Table()
    elif touch == "swap_target":          # somebody else's buffer as the target
        import torch
        mt.grid2 = torch.empty_like(mt.grid)
    else:
        mt.rotate_grids = False
    mt.step_slotted()
    assert rec.steps[-1][3] == 0
    if touch == "no_rotation":
        assert rec.steps[-1][2] is None
        return
    mt.step_slotted()
    assert rec.steps[-1][3] == 1 and rec.steps[-1][2] is not None


def test_side_4_passes_no_clear_grid(host_transfer):
    mt, rec = host_transfer(side=4)
    for _ in range(3):
        mt.step_slotted()
    assert [(s[2], s[3]) for s in rec.steps] == [(None, 0)] * 3
    assert rec.steps[1][0] == rec.steps[0][1] and rec.steps[1][1] == rec.steps[0][0]   # two grids, swapped


def test_a_failed_step_leaves_no_flag_behind(host_transfer):
    mt, rec = host_transfer()
    mt.step_slotted()
    assert mt._clean_grid is not None
    rec.__dict__["zs_rocm_mpm_step_slotted"] = lambda *a: -1
    with pytest.raises(RuntimeError):
        mt.step_slotted()
    assert mt._clean_grid is None


def test_partition_and_storage_changes_withdraw_the_flag_in_their_own_code():
    """build_partition, adopt_partition (reorder_partition goes through it), slot, repartition_slotted and the two-grid g2p2g need a GPU to
    run: that each of them calls _grids_written() is read from its source"""
    from zpc_amd.mpm import MpmTransfer
    for name in ("build_partition", "adopt_partition", "slot", "repartition_slotted", "g2p2g", "apply_boundary", "p2c2g"):
        assert "self._grids_written()" in inspect.getsource(getattr(MpmTransfer, name)), name
    assert "self.adopt_partition(" in inspect.getsource(MpmTransfer.reorder_partition)
