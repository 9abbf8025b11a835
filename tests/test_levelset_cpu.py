"""Sparse level-set colliders, the parts that need no GPU: the ctypes mirror of zs_rocm_levelset (and of the step struct's new member)
against the header, the float64 restatement (tests/ref64_levelset.py) on a sampled plane, and the block selection of from_dense."""
import ctypes as C
import os
import subprocess

import numpy as np

import ref64_levelset as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_mirror_of_the_levelset_struct_matches_the_header(tmp_path):
    """every field of _lib.LevelSet at the offset and of the size the host compiler gives zs_rocm_levelset's member of the same name,
    same total size (the method of test_ctypes_mirrors_of_the_mpm_structs_match_the_header); the step struct ends with `levelset`"""
    from zpc_amd import _lib
    pairs = {"zs_rocm_levelset": _lib.LevelSet, "zs_rocm_bht_view_lite": _lib.BhtViewLite, "zs_rocm_mpm_step": _lib.MpmStep}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "zs_rocm.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append('  printf("%s|size|%%zu|0\\n", sizeof(%s));' % (cname, cname))
        for m, _ in cls._fields_:
            src.append('  printf("%s|%s|%%zu|%%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, m, cname, m, cname, m))
    src += ['  return 0;', '}']
    c = tmp_path / "mirror.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "mirror"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        sname, m, a, b = line.split("|")
        got.setdefault(sname, {})[m] = [int(a), int(b)]
    for cname, cls in pairs.items():
        assert C.sizeof(cls) == got[cname]["size"][0], (cname, C.sizeof(cls), got[cname]["size"][0])
        for m, _ in cls._fields_:
            f = getattr(cls, m)
            assert [f.offset, f.size] == got[cname][m], (cname, m, [f.offset, f.size], got[cname][m])
    assert _lib.MpmStep._fields_[-1][0] == "levelset"
    assert _lib.MpmStep.levelset.offset + _lib.MpmStep.levelset.size == C.sizeof(_lib.MpmStep)


def _plane_levelset(h, nrm, org, n=24, band=1e9):
    from zpc_amd.levelset import select_blocks
    idx = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).astype(np.float64)
    sdf = ((idx * h - org) * nrm).sum(-1)
    keys, cells = select_blocks(sdf.astype(np.float32), band, band)
    return rl.LevelSet64(keys, cells, (0.0, 0.0, 0.0), h, band), sdf


def test_ref64_on_a_sampled_plane_reproduces_the_analytic_plane():
    """a trilinear interpolant reproduces a linear function: distance and normal of the restatement equal the plane's up to the
    float32 rounding of the stored samples (u |value| per cell, 13 u T for the restatement's own bound) -- the check of the checker"""
    h = 1.0 / 16
    nrm = np.array([0.36, 0.8, -0.48])
    org = np.array([0.5, 0.6, 0.55])
    ls, _ = _plane_levelset(h, nrm, org)
    g = np.random.default_rng(3)
    x = (0.2 + g.random((4000, 3)) * 0.9).astype(np.float32)
    sd, b = ls.sdf(x)
    want = ((x.astype(np.float64) - org) * nrm).sum(1)
    # stored samples carry u |value| each; the reproduced float32 index position X carries 2 u |X| per axis, i.e. 2 u |X| h |n_d| of distance
    X = x.astype(np.float64) / h
    slack = rl.U * (np.abs(want) + 3 * h) + (2 * rl.U * np.abs(X) * h * np.abs(nrm)).sum(1)
    assert (np.abs(sd - want) <= b + slack).all(), (np.abs(sd - want) / (b + slack)).max()
    n, bn, l = ls.normal(x)
    assert (np.abs(l - 1) < 1e-4).all()
    # the difference quotient divides the samples' roundings by 2 eps = h / 2
    assert (np.abs(n - nrm) <= bn + 8 * (slack / (h / 2))[:, None]).all(), np.abs(n - nrm).max()
    assert np.abs(n - nrm).max() < 2e-5
    v, bv = ls.velocity(x)
    assert (v == 0).all() and (bv == 0).all()


def test_ref64_blends_the_background_and_returns_it_outside():
    from zpc_amd.levelset import select_blocks
    sdf = np.full((16, 8, 8), 1.0, np.float32)
    sdf[:8] = -0.25                      # block (0,0,0) stored, block (8,0,0) not (no cell under the band)
    keys, cells = select_blocks(sdf, 0.5, 0.5)
    assert keys.tolist() == [[0, 0, 0]]
    ls = rl.LevelSet64(keys, cells, (0.0, 0.0, 0.0), 1.0, 0.5)
    x = np.array([[7.25, 3.0, 3.0], [30.0, 3.0, 3.0], [3.0, 3.0, 3.0]], np.float32)
    sd, b = ls.sdf(x)
    assert sd[0] == 0.75 * -0.25 + 0.25 * 0.5 and sd[1] == 0.5 and sd[2] == -0.25


def test_from_dense_block_selection():
    """select_blocks (the host half of SparseLevelSet.from_dense): a block is stored exactly when one of its cells has |sdf| < band; keys are
    block origins in lexicographic order; the cell order inside a block is (x * 8 + y) * 8 + z; the array is padded with the background;
    the velocity rides along as channels 1..3"""
    from zpc_amd.levelset import select_blocks
    sdf = np.full((20, 9, 8), 1.0, np.float32)
    sdf[17, 8, 3] = 0.01
    sdf[1, 2, 3] = -0.4
    sdf[9, 1, 1] = 0.5          # not under the band: |sdf| < band is strict
    vel = np.zeros(sdf.shape + (3,), np.float32)
    vel[17, 8, 3] = (1, 2, 3)
    keys, cells = select_blocks(sdf, 0.5, 0.75, vel)
    assert keys.dtype == np.int32 and keys.tolist() == [[0, 0, 0], [16, 8, 0]]
    assert cells.shape == (2 * 512, 4) and cells.dtype == np.float32
    assert cells[(1 * 8 + 2) * 8 + 3].tolist() == [np.float32(-0.4), 0, 0, 0]
    assert cells[512 + (1 * 8 + 0) * 8 + 3].tolist() == [np.float32(0.01), 1, 2, 3]
    pad = cells[512 + (5 * 8 + 0) * 8 + 3]     # index (21, 8, 3): beyond the array
    assert pad.tolist() == [0.75] * 4
    k1, c1 = select_blocks(sdf, 0.5, 0.75)
    assert np.array_equal(k1, keys) and np.array_equal(c1[:, 0], cells[:, 0]) and c1.shape[1] == 1
