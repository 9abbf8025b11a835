"""Float64 reference of the implicit-MPM force operator (G2P2GTransfer, zs_rocm_mpm_implicit_force), built from tests/ref64.py.

The gather half is ref64.g2p64 unchanged (C_trial, F_trial / J_trial and their bounds b_C, b_F / b_J from the dof velocities).  The
scatter half is the force channels of ref64.p2g64 with the scale +D_inv instead of -dt D_inv:

    f_i = sum_p W_ip D_inv (P F^T vol)_p (x_i - x_p)

with the same per-term constant C_F = 23 (the scale costs at most the 6 roundings counted there: D_inv 3, its product with P F^T vol,
and the product with dx of a kernel that keeps alpha / b_k per channel), so the bound of a node is (N + C_F) u T + e_in, T the sum of
D_inv W |P F^T vol| (k dx + lp).  The result is a ref64.Grid64 whose channels 4-6 hold the force, so ref64.check_grid checks it.

Also here: the inputs of the implicit tests (clouds, states, the trial velocity field), shared by the CPU test that proves the oracle's
stress finite on them and the GPU tests that use them.
"""
import numpy as np

import ref64
from util import rng, make_cloud, make_mixed_cloud, make_edge_cloud, tag_masses

DX = 1.0 / 64
DT = 1e-3
CLOUDS = ("lattice", "mixed", "edge")
TRIAL_SCALE = {"lattice": 1.0, "mixed": 1.0, "edge": 0.1}


def force64(PF, pos, dx, ePF=None):
    """Grid64 with channels 4-6 = +D_inv W (P F^T vol) xixp summed per node (channels 0-3 stay 0); ePF: absolute bound of PF (e_in)"""
    n = len(pos)
    nodes, W, xixp, X = ref64.stencil(pos, dx)
    dxd = float(np.float32(dx))
    s = 4.0 / (dxd * dxd)
    P = ref64._mat(PF)
    val = s * W[..., None] * np.einsum("ndj,nkj->nkd", P, xixp)
    T = s * W[..., None] * np.einsum("ndj,nkj->nkd", np.abs(P), X)
    ein = np.zeros((n, 27, 3)) if ePF is None else s * W[..., None] * np.einsum("ndj,nkj->nkd", ref64._mat(ePF), X)
    coords, out, N = ref64._accumulate(nodes, (val, T, ein))
    val, T, ein = (np.pad(a, ((0, 0), (4, 0))) for a in out)
    return ref64.Grid64(coords, val, T, N, ein, ref64.C_GRID.copy())


def dof_world(mt, dof):
    """an MpmTransfer's dof vector [nblocks side^3, 3] as ref64 world nodes: (coords, values [., 7] with the dof in channels 4-6)"""
    keys = np.asarray(mt.active_keys(), np.int64)
    side, kscale = mt.side, mt.side // mt.kstride
    l = np.arange(side ** 3)
    loc = np.stack([l // (side * side), (l // side) % side, l % side], 1)
    coords = (keys[:, None, :] * kscale + loc[None]).reshape(-1, 3)
    v = np.zeros((coords.shape[0], 7))
    v[:, 4:7] = np.asarray(dof, np.float64).reshape(-1, 3)
    return coords, v


def trial_velocity(coords, x0, dx=DX, scale=1.0):
    """float32 trial node velocities [M, 3]: a linear field G (x - x0) with |G| <= 12 / s (dt |C| ~ 1 % at DT; x0: the cloud's centre,
    which keeps |v| below 2) plus +-0.01 of exact integer-hash noise per node and component (its gradient adds ~1 / s to C).
    A particle whose arena rounded (d0 != lpn, the edge cloud) gathers D_inv dx (d0 - lpn) v on top of the gradient, i.e. up to
    4 / dx |v|, which would put dt |C| at ~0.5 there (the oracle's von Mises stress is not finite for some of them): the edge cloud
    takes scale = 0.1 (TRIAL_SCALE), |v| < 0.2, so that dt |C| stays below 5 % for every particle."""
    c = np.asarray(coords, np.int64)
    G = np.array([[5.0, -12.0, 3.0], [9.0, -4.0, -6.0], [-2.0, 11.0, -6.0]])
    x = c.astype(np.float64) * dx - np.asarray(x0, np.float64)
    h = (c[:, 0] * 73856093) ^ (c[:, 1] * 19349663) ^ (c[:, 2] * 83492791)
    noise = np.stack([((h >> (5 * d)) & 0xFFFF) / 65536.0 - 0.5 for d in range(3)], 1)
    return (scale * (x @ G.T + 0.02 * noise)).astype(np.float32)


def cloud_centre(pos):
    """x0 of trial_velocity: the middle of the cloud's bounding box, on the grid"""
    p = np.asarray(pos, np.float64)
    return np.round((p.min(0) + p.max(0)) / 2 / DX) * DX


def model_kw(model):
    return dict(yield_stress=200.0) if model == 2 else dict(beta=0.5) if model == 3 else {}


def implicit_case(cloud, model):
    """(mass, pos, vel, C, state, logJp): the clouds of the ref64 GPU tests (F = I + 1 % noise), the fluid's J = 1 + 1 % noise in
    state[:, 0], logJp = 1 % noise"""
    if cloud == "lattice":
        m, x, v, Cm, F = make_cloud(6, DX, 2, seed=3)
    elif cloud == "mixed":
        m, x, v, Cm, F = make_mixed_cloud(6, DX)
    else:
        m, x, v, Cm, F = make_edge_cloud(DX)
    n = x.shape[0]
    lj = (0.01 * rng(33).standard_normal(n)).astype(np.float32)
    if model == 4:
        F = (1.0 + 0.01 * rng(11).standard_normal(n)).astype(np.float32)[:, None]
    return tag_masses(m), x, v, Cm, F, lj


def trial64(grid_v, pos, state, model, dx=DX, dt=DT):
    """ref64.g2p64 on the trial velocities: C, b_C and F, b_F (solids) or J, b_J (fluid)"""
    return ref64.g2p64(grid_v, pos, dx, dt, F=state if model != 4 else None, J=state[:, 0] if model == 4 else None)


def stencil_nodes(pos, dx=DX):
    """the distinct nodes the particles' stencils touch, [M, 3]"""
    nodes = ref64.stencil(pos, dx)[0].reshape(-1, 3)
    k, i = np.unique(ref64.node_key(nodes), return_index=True)
    return nodes[i]
