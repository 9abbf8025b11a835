"""Shared helpers for the parity tests: seeded inputs (xorshift64*) and oracle wrappers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

SEED0 = 0x9E3779B97F4A7C15


def rng(config_id=0):
    return np.random.Generator(np.random.PCG64(SEED0 ^ config_id))


def xorshift64star(n, seed):
    """The synthetic-input generator named by SURVEY.md 8(d); returns n uint64."""
    out = np.empty(n, dtype=np.uint64)
    x = np.uint64(seed if seed else 1)
    m = np.uint64(0x2545F4914F6CDD1D)
    with np.errstate(over="ignore"):
        for i in range(n):
            x ^= x >> np.uint64(12)
            x ^= x << np.uint64(25)
            x ^= x >> np.uint64(27)
            out[i] = x * m
    return out


def ptr(a, ct=None):
    return a.ctypes.data_as(C.c_void_p)


def orc_call(oracle, name, *args):
    f = getattr(oracle, name)
    f.restype = None
    conv = []
    for a in args:
        if isinstance(a, np.ndarray):
            conv.append(a.ctypes.data_as(C.c_void_p))
        elif isinstance(a, (int, np.integer)):
            conv.append(C.c_size_t(int(a)) if int(a) >= 0 else C.c_int(int(a)))
        else:
            conv.append(a)
    return f(*conv)


# ---------------------------------------------------------------------------------------- oracle MPM helpers (oracle/orc.py)
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "oracle"))
from orc import OrcMpmParams, YIELD_SURFACE, OracleMpm  # noqa: E402,F401


def make_cloud(n_side, dx, ppc_side=2, origin=(0.30, 0.31, 0.29), seed=3, noise=0.01, vel_scale=0.5):
    """Jittered lattice of particles: ppc_side^3 particles per cell in an n_side^3-cell cube."""
    g = rng(seed)
    k = n_side * ppc_side
    idx = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3)
    h = dx / ppc_side
    pos = (np.asarray(origin) + (idx + 0.5) * h + (g.random(idx.shape) - 0.5) * h * 0.8).astype(np.float32)
    n = pos.shape[0]
    vel = (vel_scale * g.standard_normal((n, 3))).astype(np.float32)
    F = (np.eye(3).reshape(1, 9) + noise * g.standard_normal((n, 9))).astype(np.float32)
    Cm = (0.1 * g.standard_normal((n, 9))).astype(np.float32)
    mass = np.full(n, 1000.0 * dx ** 3 / ppc_side ** 3, np.float32)
    return mass, pos, vel, Cm, F


def tag_masses(mass):
    """pairwise different masses (identity tag: particles are matched by mass after the slotted / re-ordering steps)"""
    n = len(mass)
    out = (mass * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    assert len(np.unique(out)) == n
    return out


def make_drifting_cloud(seed=4242, drift=(1.6, -1.5, 1.4), vel_scale=0.1):
    """identity-tagged 8^3-cell cloud drifting ~0.1 cell per step (dt = 1e-3) on all three axes: its particles cross bin and block faces"""
    dx = 1.0 / 64
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=seed, vel_scale=vel_scale)
    vel += np.array(drift, np.float32)
    return tag_masses(mass), pos, vel, Cm, F


def make_uneven_cloud(seed, ncell=10, cap=22):
    """ncell^3-cell box whose per-cell particle count is heavy-tailed (up to `cap` in a cell beside cells with one), drifting ~0.2 cell
    per step (dt = 1e-3); identity-tagged masses"""
    dx = 1.0 / 64
    g = rng(seed)
    cells = np.stack(np.meshgrid(np.arange(ncell), np.arange(ncell), np.arange(ncell), indexing="ij"), -1).reshape(-1, 3)
    cnt = np.minimum(1 + (g.pareto(1.2, cells.shape[0]) * 2).astype(int), cap)
    org = np.array([0.30, 0.31, 0.29])
    pos = np.concatenate([org + (c + 0.5 + g.random((k, 3))) * dx for c, k in zip(cells, cnt)]).astype(np.float32)  # base node = c
    n = pos.shape[0]
    mass = (1000.0 * dx ** 3 / 8 * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    vel = (0.3 * g.standard_normal((n, 3)) + np.array([3.0, -4.0, 2.0])).astype(np.float32)
    Cm = (0.1 * g.standard_normal((n, 9))).astype(np.float32)
    F = (np.eye(3).reshape(1, 9) + 0.01 * g.standard_normal((n, 9))).astype(np.float32)
    return mass, pos, vel, Cm, F, cnt


def make_mixed_cloud(n_side, dx, origin=(0.30, 0.31, 0.29), seed=5, vel_scale=0.5):
    """make_cloud with three abutting slabs along x of per-particle mass m, 1e-3 m and 1e-6 m, and neighbouring particles moving in
    opposite directions (the lattice parity flips the sign of v and C), so that momentum cancels at the nodes; free surface on every side"""
    ppc = 2
    mass, pos, vel, Cm, F = make_cloud(n_side, dx, ppc, origin=origin, seed=seed, vel_scale=vel_scale)
    k = n_side * ppc
    idx = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3)
    slab = np.minimum(3 * idx[:, 0] // k, 2)
    mass = (mass * np.array([1.0, 1e-3, 1e-6], np.float32)[slab]).astype(np.float32)
    sign = np.where(idx.sum(1) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None]
    base = np.array([0.8, -0.6, 0.7], np.float32)
    vel = (sign * base + 0.05 * vel).astype(np.float32)
    Cm = (sign * np.abs(Cm)).astype(np.float32)
    return mass, pos, vel, Cm, F


def make_edge_cloud(dx=1.0 / 64, seed=17, vel_scale=0.2, drift=(0.0, 0.0, 0.0)):
    """8^3-cell cloud straddling world coordinate 0 whose particles sit on the arena's edges, one axis each: X - 0.5 integral (one
    weight is 0), X = 0.5 - 2^-25 and 0.5 - 2^-24 (lpn rounds up to 1.5), X = -0.5 - 2^-24 (X - 0.5 rounds to an integer: lpn just below
    0.5), and the first / last 1e-3 cell of base cells on bin faces (cell = 0, 3 mod 4) and block faces (0, 7 mod 8), at negative
    coordinates too.  dx must be a power of two (the edge positions are then exact)."""
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, origin=(-4 * dx, -4 * dx, -4 * dx), seed=seed, vel_scale=vel_scale)
    n = pos.shape[0]
    vel += np.array(drift, np.float32)
    X = [np.float32(c + 0.5) for c in range(-4, 4)]
    X += [np.float32(0.5) - np.float32(2.0 ** -25), np.float32(0.5) - np.float32(2.0 ** -24), np.float32(-0.5) - np.float32(2.0 ** -24)] * 3
    X += [np.float32(c + 0.5 + e) for c in (-5, -4, -1, 0, 3) for e in (1e-3, 1 - 1e-3)]
    g = rng(seed + 1)
    picked = g.choice(n, 3 * len(X), replace=False)
    for j, i in enumerate(picked):
        pos[i, j % 3] = X[j % len(X)] * np.float32(dx)
    return mass, pos, vel, Cm, F


def make_full_cell_cloud(dx, K, seed=99):
    """four particles just below the +x face of cell 35 moving (v_x = 2) into cell 36, which holds K particles at rest (the full
    destination cell of the slotted step); identity-tagged masses, C = 0, F = I"""
    g = rng(seed)
    yz = 35.0 + 0.3 * (g.random((K + 4, 2)) - 0.5)
    xa = np.full(4, 36.49)                     # cell 35 (X in [35.5, 36.5)), about to cross into cell 36
    xb = 37.0 + 0.2 * (g.random(K) - 0.5)      # cell 36, centred
    pos = (np.concatenate([np.stack([xa, yz[:4, 0], yz[:4, 1]], 1), np.stack([xb, yz[4:, 0], yz[4:, 1]], 1)]) * dx).astype(np.float32)
    n = pos.shape[0]
    mass = (1000.0 * dx ** 3 / 8 * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    vel = np.zeros((n, 3), np.float32)
    vel[:4, 0] = 2.0
    Cm = np.zeros((n, 9), np.float32)
    F = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))
    return mass, pos, vel, Cm, F


def move_after_binning(mt, pos, seed=59, frac=0.17, reach=2.4):
    """move a fraction of the inner particles of a binned MpmTransfer (two cells from the cloud's faces: they stay inside the
    partition) by up to reach / 2 cells on every axis AFTER binning: in-bin movers and out-of-bin movers for the P2G kernels.
    Every other channel of the particle buffer is kept.  Returns (new positions in the original numbering, moved mask)."""
    import torch
    from zpc_amd import lib
    dx = mt.params.dx
    n = pos.shape[0]
    r = rng(seed)
    lo, hi = pos.min(0) + 2 * dx, pos.max(0) - 2 * dx
    moved = (r.random(n) < frac) & ((pos >= lo) & (pos <= hi)).all(1)
    pos2 = pos.copy()
    pos2[moved] += (r.random((moved.sum(), 3)).astype(np.float32) - 0.5) * reach * dx
    order = mt.order.cpu().numpy()
    aos = torch.empty(n, mt.nchn, dtype=torch.float32, device=mt.buf.device)
    lib().zs_rocm_tv_to_aos_f32(mt.pol.handle, mt.buf.data_ptr(), n, mt.nchn, mt.L, aos.data_ptr())
    mt.pol.syncCtx()
    aos[:, 1:4] = torch.from_numpy(pos2[order]).to(aos.device)
    lib().zs_rocm_tv_from_aos_f32(mt.pol.handle, aos.data_ptr(), n, mt.nchn, mt.L, mt.buf.data_ptr())
    mt.pol.syncCtx()
    return pos2, moved


def oracle_stress(oracle, om, Cm, F, logJp=None):
    """[n, 9] P F^T vol of every particle as orc_mpm_p2g's model_contrib computes it (before the -dt D_inv scale), from copies of the
    inputs; the fluid's (model 4, J in F[:, 0]) restated in numpy float32 in the same operation order (the oracle builds without
    FP contraction)."""
    p = om.p
    n = F.shape[0]
    out = np.zeros((n, 9), np.float32)
    cf = C.c_float
    if p.model == 4:
        f = np.float32
        J = F[:, 0].astype(np.float32)
        vol = f(p.volume) * J
        J2 = J * J
        J4 = J2 * J2
        pressure = f(p.bulk) * (f(1) / (J * J2 * J4) - f(1))
        Cf = Cm.astype(np.float32)
        vis = f(p.viscosity)
        for r in range(3):
            for c in range(3):
                d = r + 3 * c
                s = (Cf[:, d] + Cf[:, c + 3 * r]) * vis
                out[:, d] = ((s - pressure) if r == c else s) * vol
        return out
    mu, lam = cf(), cf()
    oracle.orc_lame(cf(p.E), cf(p.nu), C.byref(mu), C.byref(lam))
    oracle.orc_nacc_bulk.restype = cf
    lj = np.zeros(n, np.float32) if logJp is None else logJp.astype(np.float32).copy()
    for i in range(n):
        Fi = np.ascontiguousarray(F[i], np.float32).copy()
        if p.model == 0:
            oracle.orc_stress_fixedcorotated(cf(p.volume), mu, lam, ptr(Fi), ptr(out[i]))
        elif p.model == 2:
            oracle.orc_stress_vonmises(cf(p.volume), mu, lam, cf(p.yieldStress), p.hostVariant, ptr(Fi), ptr(out[i]))
        elif p.model == 1:
            l = cf(lj[i])
            oracle.orc_stress_sand(cf(p.volume), mu, lam, cf(p.cohesion), cf(p.beta), cf(p.yieldSurface), p.volCorrection, C.byref(l),
                                   ptr(Fi), ptr(out[i]))
        else:
            l = cf(lj[i])
            oracle.orc_stress_nacc(cf(p.volume), mu, lam, cf(oracle.orc_nacc_bulk(cf(p.E), cf(p.nu))), cf(p.xi), cf(p.beta), cf(p.Msqr),
                                   p.hardeningOn, p.hostVariant, C.byref(l), ptr(Fi), ptr(out[i]))
    return out


def stress_tol(om, PF, F):
    """e_in of a stress computed by another instantiation than the one under test (the oracle's, the test entry's) used in place of
    the kernel's own: 1e-4 of the row scale (test_svd_and_stress_blocks)"""
    mu, lam = C.c_float(), C.c_float()
    om.o.orc_lame(C.c_float(om.p.E), C.c_float(om.p.nu), C.byref(mu), C.byref(lam))
    scale = (2 * mu.value + lam.value) * om.p.volume
    rowmag = np.maximum(np.abs(PF).max(1, keepdims=True), scale * np.maximum(1.0, np.abs(F - np.eye(3).reshape(1, 9)).max(1, keepdims=True)))
    return np.broadcast_to(1e-4 * rowmag, PF.shape)


# ---------------------------------------------------------------------------------------- scenes of the gather-style (C2) ref64 tests
C2_SCENES = ["lattice", "mixed", "edge", "edge_origin", "far", "faces", "counts", "lone"]
_C2_CACHE = {}


def _c2_fill(pos, seed, vel_scale=0.3):
    g = rng(seed)
    n = pos.shape[0]
    vel = (vel_scale * g.standard_normal((n, 3))).astype(np.float32)
    Cm = (0.1 * g.standard_normal((n, 9))).astype(np.float32)
    F = (np.eye(3).reshape(1, 9) + 0.01 * g.standard_normal((n, 9))).astype(np.float32)
    return vel, Cm, F


def c2_scene(name, dx=1.0 / 64):
    """Scenes of tests/test_c2_ref64_cpu.py and tests/test_c2_ref64_gpu.py: dict of mass, pos, vel, B (= C dx^2 / 4, the scale of
    test_c2_gpu._setup), F, J (the fluid's state), logJp, key_is_origin and, for `lone`, block (the single block of its partition, in
    block coordinates: the partition is adopted, not built).  dx must be a power of two.
      lattice      make_cloud(7, dx, 2)
      mixed        make_mixed_cloud(6, dx): three mass slabs m, 1e-3 m, 1e-6 m, momentum cancelling at the nodes
      edge         make_edge_cloud(dx): straddles 0 on all axes (edge_origin: the same with block-origin keys)
      far          lattice translated by (16, -16, 8): |x| / dx is 50 times larger
      faces        cells 3 and 4 per axis (two blocks at side 4); per axis the in-cell fractions 0, 0+, 0.25, 0.5-, 0.5, 0.5+, 0.75, 1-
                   (+ / -: the neighbouring float32), the third of the 512 combinations with (i + 2 j + 3 k) % 3 == 0: 176 per cell
      counts       5^3 cells of 8 particles; five of them hold instead 21, 22, 255 (all in octant 0), 255 (all in octant 7) and 256
      lone         one particle in the corner cell (side - 1, 0, 2) of a block that is the whole partition"""
    if (name, dx) in _C2_CACHE:
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _C2_CACHE[(name, dx)].items()}
    f = np.float32
    block = None
    if name in ("lattice", "far"):
        mass, pos, vel, Cm, F = make_cloud(7, dx, 2, seed=71, vel_scale=0.3)
        if name == "far":
            pos = (pos + np.array([16.0, -16.0, 8.0], f)).astype(f)
    elif name == "mixed":
        mass, pos, vel, Cm, F = make_mixed_cloud(6, dx)
    elif name in ("edge", "edge_origin"):
        mass, pos, vel, Cm, F = make_edge_cloud(dx)
    elif name == "faces":
        fr = lambda c: [f(c), np.nextafter(f(c), f(99)), f(c + 0.25), np.nextafter(f(c + 0.5), f(-99)), f(c + 0.5),
                        np.nextafter(f(c + 0.5), f(99)), f(c + 0.75), np.nextafter(f(c + 1), f(-99))]
        ax = np.array(fr(3) + fr(4), f)                                   # [16] X = x / dx along one axis
        i = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
        i = i[((i % 8) @ np.array([1, 2, 3])) % 3 == 0]
        pos = (ax[i] * f(dx)).astype(f)
        vel, Cm, F = _c2_fill(pos, 72)
        mass = np.full(len(pos), 1000.0 * dx ** 3 / 8, f)
    elif name == "counts":
        g = rng(73)
        org = np.array([20, 20, 16])
        mass, pos, _, _, _ = make_cloud(5, dx, 2, origin=tuple(org * dx), seed=74)
        special = {(1, 1, 1): (21, 0.0, 1.0), (3, 1, 1): (22, 0.0, 1.0), (1, 3, 1): (255, 0.0, 0.5), (3, 3, 1): (255, 0.5, 0.5),
                   (2, 2, 3): (256, 0.0, 1.0)}
        cell = np.floor(pos.astype(np.float64) / dx).astype(int) - org
        keep = np.ones(len(pos), bool)
        extra = []
        for c, (k, lo, width) in special.items():
            keep &= ~(cell == np.array(c)).all(1)
            extra.append(((org + np.array(c) + lo + width * (0.001 + 0.998 * g.random((k, 3)))) * dx).astype(f))
        pos = np.concatenate([pos[keep]] + extra).astype(f)
        vel, Cm, F = _c2_fill(pos, 75)
        mass = np.full(len(pos), mass[0], f)
    elif name == "lone":
        block = (5, 5, 4)
        pos = None   # depends on the block side: see c2_lone_pos
        mass = np.full(1, 1000.0 * dx ** 3 / 8, f)
        vel, Cm, F = _c2_fill(np.zeros((1, 3), f), 76)
    else:
        raise ValueError(name)
    n = len(mass)
    out = dict(mass=mass, pos=pos, vel=vel, B=(Cm * dx * dx * 0.25).astype(f), F=F,
               J=(1.0 + 0.01 * rng(77).standard_normal((n, 1))).astype(f), logJp=(0.01 * rng(78).standard_normal(n)).astype(f),
               key_is_origin=name == "edge_origin", block=block)
    _C2_CACHE[(name, dx)] = out
    return c2_scene(name, dx)


def c2_lone_pos(block, side, dx=1.0 / 64):
    """the lone particle: cell (side - 1, 0, 2) of the block, at fractions (0.7, 0.2, 0.4): of the 8 cells within dx, those one further
    along x and one back along y are outside the partition"""
    return ((np.array(block) * side + np.array([side - 1 + 0.7, 0.2, 2.4])) * dx).astype(np.float32).reshape(1, 3)


def lbvh_boxes(n, seed, dup=False):
    """n AABBs [n][6] = {min xyz, max xyz}: jittered centres in the unit cube, extents 0.5-3 % (dup: centres snapped to a
    coarse lattice so that many morton codes coincide)."""
    g = rng(seed)
    c = g.uniform(0, 1, (n, 3)).astype(np.float32)
    if dup:
        c = (np.round(c * 6) / 6).astype(np.float32)
    e = g.uniform(0.005, 0.03, (n, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([c - e, c + e], axis=1).astype(np.float32))


def oracle_lbvh(oracle, bv, refit=1):
    import ctypes as C
    n = bv.shape[0]
    oracle.orc_lbvh_create.restype = C.c_void_p
    oracle.orc_lbvh_num_nodes.restype = C.c_size_t
    for f in ("parents", "levels", "leaf_inds", "aux_indices"):
        getattr(oracle, "orc_lbvh_" + f).restype = C.POINTER(C.c_int32)
    oracle.orc_lbvh_bvs.restype = C.POINTER(C.c_float)
    b = C.c_void_p(oracle.orc_lbvh_create())
    oracle.orc_lbvh_build(b, bv.ctypes.data_as(C.c_void_p), C.c_size_t(n), refit)
    nn = oracle.orc_lbvh_num_nodes(b)
    A = lambda p, shape: np.ctypeslib.as_array(p, shape=shape).copy()
    arrs = {"numNodes": nn, "parents": A(oracle.orc_lbvh_parents(b), (nn,)), "levels": A(oracle.orc_lbvh_levels(b), (nn,)),
            "auxIndices": A(oracle.orc_lbvh_aux_indices(b), (nn,)), "leafInds": A(oracle.orc_lbvh_leaf_inds(b), (n,)),
            "bvs": A(oracle.orc_lbvh_bvs(b), (nn, 6))}
    return b, arrs


def collider_struct(cs):
    """row of tests/golden/collider.npz `cases` ([geometry, type, param x8, s, dsdt, R x9, omega x3, b x3, dbdt x3]) ->
    ctypes struct with the layout shared by zs_rocm_collider and orc_collider"""
    import ctypes as C

    class Col(C.Structure):
        _fields_ = [("geometry", C.c_int), ("type", C.c_int), ("param", C.c_float * 8), ("s", C.c_float), ("dsdt", C.c_float),
                    ("R", C.c_float * 9), ("omega", C.c_float * 3), ("b", C.c_float * 3), ("dbdt", C.c_float * 3)]
    return Col(int(cs[0]), int(cs[1]), (C.c_float * 8)(*cs[2:10]), float(cs[10]), float(cs[11]), (C.c_float * 9)(*cs[12:21]),
               (C.c_float * 3)(*cs[21:24]), (C.c_float * 3)(*cs[24:27]), (C.c_float * 3)(*cs[27:30]))


# ---------------------------------------------------------------------------------------- whole-function golden fixtures
GOLDEN_MODELS = {"fixedcorotated": 0, "sand": 1, "vonmises": 2, "nacc": 3, "eos": 4}
GOLDEN_CASES = [("fixedcorotated", 4), ("fixedcorotated", 8), ("sand", 4), ("sand", 8), ("vonmises", 8), ("nacc", 8), ("eos", 8)]


def golden_p2g_g2p(name, side):
    """One case of tests/golden/p2g_g2p.npz (made by tools/gen_golden.py from the reference's own LocalArena / compute_stress_* /
    matrixMatrixMultiplication3d, oracle/ref_shim.cpp): dict with the inputs, the reference's P2G grid, the grid handed to G2P, the
    G2P outputs and the next step's P2G grid, plus the model number / parameters in this repo's convention."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p2g_g2p.npz"))
    tag = "%s_s%d" % (name, side)
    prm = z["prm_" + name]
    F = z["F"].copy()
    if name == "eos":
        F[:, 0] = z["J"]
    # oracle / zs_rocm model numbering: 0 FixedCorotated, 1 DruckerPrager, 2 VonMises, 3 NACC, 4 EquationOfState
    kw = dict(E=float(prm[1]) if name != "eos" else 5e4, nu=float(prm[2]) if name != "eos" else 0.4)
    if name == "sand":
        kw.update(cohesion=float(prm[3]), beta=float(prm[4]))
    if name == "vonmises":
        kw.update(yield_stress=float(prm[7]))
    if name == "nacc":
        kw.update(beta=float(prm[4]), xi=float(prm[8]), friction_angle=float(prm[9]), hardening=bool(prm[10]))
    if name == "eos":
        kw.update(bulk=float(prm[11]), viscosity=float(prm[12]))
    return dict(model=GOLDEN_MODELS[name], side=side, dx=float(z["dx"]), dt=float(z["dt"]), volume=float(prm[0]), kw=kw,
                gravity=tuple(float(v) for v in z["gravity"]), keys=z["keys_s%d" % side], mass=z["mass"], pos=z["pos"], vel=z["vel"],
                C=z["C"], F=F, logJp=z["logJp"], grid=z["grid_" + tag], logJp1=z["logJp1_" + tag], gridv=z["gridv_" + tag],
                pos1=z["pos_" + tag], vel1=z["vel_" + tag], C1=z["C_" + tag], F1=z["F_" + tag], grid2=z["grid2_" + tag],
                logJp2=z["logJp2_" + tag],
                # physical scale of a nodal force entry for this cloud: the elastic (FixedCorotated) response to the same F set.
                # The NACC case projects every particle onto the tip of the yield surface, where P F^T is the difference of
                # nearly equal numbers (1e-4 of the elastic stress), so "relative to its own maximum" would measure noise.
                rhs_scale=float(np.abs(z["grid_fixedcorotated_s8"][:, 4:]).max()))


def golden_c2(name, side):
    """One case of tests/golden/c2.npz (P2C2GTransfer / G2C2PTransfer bodies over the reference's own pieces, oracle/ref_shim.cpp via
    tools/gen_golden.py): inputs, the reference's P2C2G grid (channels 0..3), a velocity grid and the reference's G2C2P v / B."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2.npz"))
    prm = z["prm_" + name]
    F = z["F"].copy()
    if name == "eos":
        F[:, 0] = z["J"]
    kw = dict(E=float(prm[1]) if name != "eos" else 5e4, nu=float(prm[2]) if name != "eos" else 0.4)
    if name == "vonmises":
        kw.update(yield_stress=float(prm[7]))
    if name == "eos":
        kw.update(bulk=float(prm[11]), viscosity=float(prm[12]))
    return dict(model=GOLDEN_MODELS[name], side=side, dx=float(z["dx"]), dt=float(z["dt"]), volume=float(prm[0]), kw=kw, keys=z["keys_s%d" % side],
                mass=z["mass"], pos=z["pos"], vel=z["vel"], B=z["B"], F=F, grid=z["grid_%s_s%d" % (name, side)], gridv=z["gridv_s%d" % side],
                vel1=z["g2c2p_vel_s%d" % side], B1=z["g2c2p_B_s%d" % side])


LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def code_object_kernels(obj, workdir, co_name="p.co"):
    """The gfx950 kernels of a built object file or program: (kernel name, metadata dict, symbol size) per kernel, and the path of the
    unbundled code object (for a disassembly).  objcopy takes the fat binary out of `obj`, clang-offload-bundler the gfx950 code object
    out of that, llvm-readelf its notes and symbols; the metadata values stay strings (".vgpr_count" -> "128").  None if `obj` or the
    llvm tools are missing."""
    bundler = os.path.join(LLVM_BIN, "clang-offload-bundler")
    if not (os.path.exists(obj) and os.path.exists(bundler)):
        return None
    fat, co = os.path.join(str(workdir), co_name + ".fat"), os.path.join(str(workdir), co_name)
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([bundler, "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co, "--unbundle"])
    readelf = os.path.join(LLVM_BIN, "llvm-readelf")
    notes = subprocess.run([readelf, "--notes", co], stdout=subprocess.PIPE, check=True).stdout.decode()
    syms = subprocess.run([readelf, "-sW", co], stdout=subprocess.PIPE, check=True).stdout.decode()
    size = {f[7]: int(f[2]) for f in (l.split() for l in syms.splitlines()) if len(f) == 8 and f[3] == "FUNC"}
    kernels = []
    for blk in notes.split("- .agpr_count:")[1:]:
        meta = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)\s*$", "    .agpr_count:" + blk, re.M))
        if ".name" in meta:
            kernels.append((meta[".name"], meta, size[meta[".name"]]))
    return kernels, co


# ---------------------------------------------------------------------------------------- per-sample oracle SVD / stress (ref64_stress)
_ORC_STRESS_CACHE = {}


def _proto(oracle, name, argtypes):
    """a private prototype of an oracle function: the argument types of the shared CDLL's own attribute stay as other tests set them"""
    return C.CFUNCTYPE(None, *argtypes)((name, oracle))


def oracle_svd_all(oracle, F):
    """orc_svd3 of every row of F [n, 9] float32 -> U [n, 9], S [n, 3], V [n, 9]"""
    F = np.ascontiguousarray(F, np.float32)
    n = len(F)
    Uo, So, Vo = np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 9), np.float32)
    f = _proto(oracle, "orc_svd3", [C.c_void_p] * 4)
    pF, pU, pS, pV = F.ctypes.data, Uo.ctypes.data, So.ctypes.data, Vo.ctypes.data
    for i in range(n):
        f(pF + 36 * i, pU + 36 * i, pS + 12 * i, pV + 36 * i)
    return Uo, So, Vo


def oracle_stress_all(oracle, m, F, lj, key=None):
    """the oracle's constitutive update of every sample: m is a ref64_stress.Material (models 0-3; CUDA-header variants of von Mises
    and NACC).  Returns P F^T vol [n, 9], the projected F [n, 9] and the new logJp [n] (copies; cached under `key`, which names the
    inputs, together with the material's values)."""
    if key is not None:
        key = (key, tuple(sorted(vars(m).items())))
    if key is not None and key in _ORC_STRESS_CACHE:
        return tuple(a.copy() for a in _ORC_STRESS_CACHE[key])
    Fo = np.ascontiguousarray(F, np.float32).copy()
    ljo = np.ascontiguousarray(lj, np.float32).copy()
    n = len(Fo)
    PF = np.zeros((n, 9), np.float32)
    cf, vp = C.c_float, C.c_void_p
    pF, pL, pP = Fo.ctypes.data, ljo.ctypes.data, PF.ctypes.data
    if m.model == 0:
        f = _proto(oracle, "orc_stress_fixedcorotated", [cf, cf, cf, vp, vp])
        for i in range(n):
            f(m.volume, m.mu, m.lam, pF + 36 * i, pP + 36 * i)
    elif m.model == 1:
        f = _proto(oracle, "orc_stress_sand", [cf, cf, cf, cf, cf, cf, C.c_int, vp, vp, vp])
        for i in range(n):
            f(m.volume, m.mu, m.lam, m.cohesion, m.beta, m.yield_surface, int(m.vol_correction), pL + 4 * i, pF + 36 * i, pP + 36 * i)
    elif m.model == 2:
        f = _proto(oracle, "orc_stress_vonmises", [cf, cf, cf, cf, C.c_int, vp, vp])
        for i in range(n):
            f(m.volume, m.mu, m.lam, m.yield_stress, 0, pF + 36 * i, pP + 36 * i)
    else:
        f = _proto(oracle, "orc_stress_nacc", [cf, cf, cf, cf, cf, cf, cf, C.c_int, C.c_int, vp, vp, vp])
        for i in range(n):
            f(m.volume, m.mu, m.lam, m.bm, m.xi, m.beta, m.Msqr, int(m.hardening), 0, pL + 4 * i, pF + 36 * i, pP + 36 * i)
    if key is not None:
        _ORC_STRESS_CACHE[key] = (PF.copy(), Fo.copy(), ljo.copy())
    return PF, Fo, ljo


def eos_f32(J, bulk, volume):
    """stress_eos without viscosity in numpy float32, in the header's operation order -> P F^T vol [n, 9]"""
    f = np.float32
    J = np.asarray(J, f)
    with np.errstate(all="ignore"):
        J2 = J * J
        J4 = J2 * J2
        p = f(bulk) * (f(1) / (J * J2 * J4) - f(1))
        d = (f(0) - p) * (f(volume) * J)
    out = np.zeros((len(J), 9), f)
    out[:, 0] = out[:, 4] = out[:, 8] = d
    return out
