"""Float64 reference of the gather-style transfers P2C2G / G2C2P (oracle/mpm.c orc_mpm_p2c2g, orc_mpm_g2c2p, orc_mpm_post_g2c2p;
zpc_amd/csrc/mpm_c2.hip) with a node-local and particle-local error bound, in the style of tests/ref64.py.

Semantics.  Cells are the partition's cells only.  A particle contributes to every partition cell whose centre is within dx per axis,
with the weight W = prod_axis (1 - |d| / dx), d = x_c - x_p.  Per particle Q = C m - dt Dinv PF (kind 0), C m (kind 1), - dt Dinv PF
(kind 2), with C[r + 3 j] = B[r + 3 j] Dinv_j, Dinv_j = 2 / (dx^2 - 2 r_j^2), r_j = x_j - floor(x_j / dx + 0.5) dx.  A cell holds
m_c = sum m W, mv_c = sum m v W, Q_c = sum Q W, (Q x_p)_c = sum (Q x_p) W; a node receives 1/8 of each of its 8 cells that exist,
m_c and mv_c + (Q_c x_i - (Q x_p)_c); nodes outside the partition receive nothing.  G2C2P: per cell v_c = sum v_i / 8 and
vx_c = sum v_i (x) x_i / 8 over the cell's present nodes, per particle v += sum W v_c, B += sum W (vx_c - v_c (x) x_p) over the present
cells within dx; Post: C = B Dinv, F <- (I + dt C) F or J <- (1 + dt tr C) J, x += dt v.

Bound of every value, as in ref64:

    |got - ref| <= (N + c) u T + e_in + (N + c) 2^-126

    N     terms summed into the value: a node's N = sum of the particle counts of its cells + 8 (the 8 cells); a particle's N = its
          cells + 1 (the value accumulated into).  (N - 1) u T bounds float32 summation in any order, so cell-major (the oracle) and
          octant-ordered, 2x2x2-cells-per-lane (the kernels) sums are both covered.
    T     the sum over the terms of the products of the MAGNITUDES of their factors.  The two cancellations of this family enter with
          both halves: the node's (Q_c x_i - (Q x_p)_c) as sum |Q| (|x_i| + |x_p|) W, the particle's W (vx_c - v_c x_p) as
          W (|vx_c| + |v_c| |x_p|), with |v_c| = sum |v_i| / 8 and |vx_c| = sum |v_i| |x_i| / 8.  Their rounding error therefore grows with
          |x| / dx, and so does the bound.
    e_in  the weight's ABSOLUTE error (below), and the propagated bound ePF of a stress that is not the kernel's own.

The linear weight.  dx is a power of two (asserted), so x_c = (c + 0.5) dx and d / dx are exact; d = x_c - x_p rounds only where x_p has
finer ulps than dx / 2^24 (next to the origin), by <= u |d| <= u dx, and 1 - |d| / dx rounds by <= u: every axis weight has an absolute
error <= EW = 2 u -- not a relative one, the weight itself may be 0.  It is carried as e_W = EW (w_y w_z + w_x w_z + w_x w_y) (each
w + EW) times the magnitude of the term; the two products of W are relative (2 u, in c).  The same term covers the one discrete decision
of the family: a particle within rounding of |d| = dx is taken by one implementation (with a weight <= EW) and skipped by another (the
range check of the reference functor; the kernel's 8 cells floor(x / dx - 0.5) + {0, 1}^3 where the functor walks 27).  The reference
here takes every cell within dx (1 + 4 u), with the weight clamped at 0, so no float32 decision is replayed.

Dinv.  k = floor(x / dx + 0.5) is taken in float32 as the implementations take it (x / dx exact, one addition: a fused x * (1 / dx) + 0.5
gives the same bits), then r = x - k dx is exact, r r rounds once (u 2 r^2 <= u dx^2 / 2 <= u of the result dx^2 - 2 r^2 >= dx^2 / 2), the
subtraction once more, the division is correctly rounded (the kernels build without fast-math): Dinv <= 3 u, counted as 4.

Per-term constants c (first order, each factor's relative error counted once):

    C      B Dinv: 4 + 1                                                                = 5 u
    Q      C m: 6 u of |C| m;  PF (Dinv * -dt): 4 + 1 + 1 = 6 u of |PF| Dinv dt;  their sum one more: 7 u of |Q| = |C| m + |PF| Dinv dt
    W      two products                                                                 = 2 u
    mass   m W: 2 + 1, the add into the grid (the transfer ADDS: one rounding against a pre-filled node) 1:  C2_M  = 4
    mv     three kinds of term end in the node's momentum:
             m v W                 two products, W, the add to lin:               2 + 2 + 1      = 5
             (Q x_p) W             Q 7, three products and two adds 3, W 2, the product 1, the subtraction 1, the add to mv_c 1 = 15
             Q W x_i               Q 7, W 2, the product 1, then x_i: product and two adds 3, the subtraction 1, the add 1      = 15
           with the add into the grid                                                    C2_MV = 16
    v_p    v_c W: v_c is a sum of 8 exact products (8 u), W 2, the product 1:            C2_GV = 11
    B_p    W (vx_c - v_c x_p): vx_c 8 + 1 (the product with x_i), v_c x_p 8 + 1, the subtraction 1, W 2, the product 1: C2_GB = 14
    C      B Dinv after the transfer: 5 u of |C| plus Dinv * bound(B)
    x, F, J  as in ref64.g2p64: x + dt v 2 u; (I + dt C) F 5 u; (1 + dt tr C) J 4 u

Matrices are 9-vectors in column-major order (M[r + 3 j]).  numpy only."""
import numpy as np

from ref64 import U, FLT_MIN, node_key, Grid64, _mat, _vec9

EW = 2 * U
C2_M, C2_MV = 4, 16
C2_GRID = np.array([C2_M, C2_MV, C2_MV, C2_MV, 0, 0, 0], np.float64)
C2_GV, C2_GB = 11, 14
_COL = np.repeat(np.arange(3), 3)    # column j of component d = r + 3 j
_ROW = np.tile(np.arange(3), 3)      # row r
_K4 = np.stack(np.meshgrid(np.arange(-1, 3), np.arange(-1, 3), np.arange(-1, 3), indexing="ij"), -1).reshape(64, 3)
_O8 = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(8, 3)


def _dx64(dx):
    dx32 = np.float32(dx)
    assert np.frexp(dx32)[0] == 0.5, "ref64_c2 needs a power-of-two dx (see the module docstring)"
    return float(dx32)


def partition_cells(keys, side, key_is_origin=False):
    """[nb side^3, 3] cell (= node) coordinates of a partition, sorted by node_key"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    l = np.arange(side ** 3)
    loc = np.stack([l // (side * side), (l // side) % side, l % side], 1)
    c = (keys[:, None, :] * (1 if key_is_origin else side) + loc[None]).reshape(-1, 3)
    return c[np.argsort(node_key(c))]


def _lookup(sorted_coords, coords):
    """row of coords [..., 3] in sorted_coords (-1: absent)"""
    if len(sorted_coords) == 0:
        return np.full(np.shape(coords)[:-1], -1, np.int64)
    sk = node_key(sorted_coords)
    k = node_key(coords)
    i = np.minimum(np.searchsorted(sk, k), len(sk) - 1)
    return np.where(sk[i] == k, i, -1)


def dinv64(x, dx):
    """[n, 3] Dinv per axis (P2C2G.hpp:88-89); the nearest node k in float32, as every implementation takes it"""
    dxd = _dx64(dx)
    x32 = np.asarray(x, np.float32)
    k = np.floor(x32 * (np.float32(1.0) / np.float32(dx)) + np.float32(0.5)).astype(np.float64)
    r = x32.astype(np.float64) - k * dxd
    return 2.0 / (dxd * dxd - 2.0 * r * r)


def pairs(x, cells, dx, only_cells=None):
    """every (particle, partition cell) with the cell centre within dx (1 + 4 u) per axis: p [P], c [P] (row of `cells`), W [P] and its
    absolute error e_W [P].  only_cells [k, 3]: keep the pairs of these cells only (the negative controls)."""
    dxd = _dx64(dx)
    X = np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3) / dxd
    c0 = np.floor(X - 0.5).astype(np.int64)
    cc = c0[:, None, :] + _K4[None]                        # [n, 64, 3]
    a = np.abs(cc + 0.5 - X[:, None, :])
    w = np.clip(1.0 - a, 0.0, None)
    row = _lookup(cells, cc)
    keep = (a <= 1.0 + 4 * U).all(-1) & (row >= 0)
    if only_cells is not None:
        keep &= _lookup(partition_sorted(only_cells), cc) >= 0
    p, s = np.nonzero(keep)
    w = w[p, s]
    wa = w + EW
    return p, row[p, s], w.prod(-1), EW * (wa[:, 1] * wa[:, 2] + wa[:, 0] * wa[:, 2] + wa[:, 0] * wa[:, 1])


def partition_sorted(coords):
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    return c[np.argsort(node_key(c))]


def _sum(idx, cols, size):
    return np.stack([np.bincount(idx, weights=cols[:, j], minlength=size) for j in range(cols.shape[1])], 1)


def p2c2g64(kind, keys, side, mass, x, v, B, dx, dt, PF=None, ePF=None, key_is_origin=False, only_cells=None):
    """P2C2GTransfer (kind 0), ...Momentum (1), ...Force (2) in float64: Grid64 of channels 0-3 over the touched partition nodes (4-6 stay
    0: the transfers do not write them).  PF [n, 9] = P F^T vol (kinds 0, 2), ePF its absolute error bound.  only_cells [k, 3]: the
    moments of these cells only (one term of the sum, for the negative controls)."""
    dxd, dtd = _dx64(dx), float(np.float32(dt))
    cells = partition_cells(keys, side, key_is_origin)
    m = np.asarray(mass, np.float32).astype(np.float64)
    xp = np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3)
    vp = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(m)
    Dcol = dinv64(x, dx)[:, _COL]
    Q, Qm, eQ = np.zeros((n, 9)), np.zeros((n, 9)), np.zeros((n, 9))
    if kind != 1:
        P = np.asarray(PF, np.float64).reshape(n, 9)
        Q -= dtd * Dcol * P
        Qm += dtd * Dcol * np.abs(P)
        if ePF is not None:
            eQ += dtd * Dcol * np.asarray(ePF, np.float64).reshape(n, 9)
    mk = m if kind != 2 else np.zeros(n)
    if kind != 2:
        Cq = np.asarray(B, np.float32).astype(np.float64).reshape(n, 9) * Dcol
        Q += Cq * m[:, None]
        Qm += np.abs(Cq) * m[:, None]
    qx = lambda q, xx: np.stack([(q[:, r::3] * xx).sum(1) for r in range(3)], 1)       # (Q x)[r] = sum_j Q[r + 3 j] x[j]
    A = np.concatenate([mk[:, None], mk[:, None] * vp, Q, qx(Q, xp)], 1)                # the 16 moments of a cell, per unit weight
    Am = np.concatenate([mk[:, None], mk[:, None] * np.abs(vp), Qm, qx(Qm, np.abs(xp))], 1)
    E = np.concatenate([np.zeros((n, 4)), eQ, qx(eQ, np.abs(xp))], 1)
    p, c, W, eW = pairs(x, cells, dx, only_cells)
    nc = len(cells)
    val = _sum(c, A[p] * W[:, None], nc)
    T = _sum(c, Am[p] * W[:, None], nc)
    epf = _sum(c, E[p] * W[:, None], nc)
    ein = _sum(c, Am[p] * eW[:, None], nc) + epf
    Nc = np.bincount(c, minlength=nc).astype(np.float64)
    # cell -> its 8 nodes that exist
    src = np.nonzero(Nc > 0)[0]
    nodes = cells[src][:, None, :] + _O8[None]                                           # [k, 8, 3]
    row = _lookup(cells, nodes)
    ok = row >= 0
    xi = np.abs(nodes[ok] * dxd)                                                         # |x_i| [P, 3]
    xs = nodes[ok] * dxd
    s = np.broadcast_to(src[:, None], row.shape)[ok]
    t = row[ok]

    def node_terms(M, pos, sign):
        out = np.zeros((len(s), 4))
        out[:, 0] = M[s, 0]
        for r in range(3):
            out[:, 1 + r] = M[s, 1 + r] + (M[s, 4 + r::3][:, :3] * pos).sum(1) + sign * M[s, 13 + r]
        return out / 8.0

    gv = _sum(t, node_terms(val, xs, -1.0), nc)
    gT = _sum(t, node_terms(T, xi, 1.0), nc)
    ge = _sum(t, node_terms(ein, xi, 1.0), nc)
    gp = _sum(t, node_terms(epf, xi, 1.0), nc)
    gN = np.bincount(t, weights=Nc[s], minlength=nc)
    touched = gN > 0
    pad = lambda a: np.pad(a[touched], ((0, 0), (0, 3)))
    g = Grid64(cells[touched], pad(gv), pad(gT), gN[touched] + 8, pad(ge), C2_GRID.copy())
    g.e_pf = pad(gp)   # the part of ein that ePF brings: the unit in which the GPU tests report the force gap
    return g


def g2c2p64(keys, side, nodes, x, dx, dt, v0=None, B0=None, F=None, J=None, key_is_origin=False, only_cells=None):
    """G2C2PTransfer (+ PostG2C2PTransfer) in float64.  nodes = (coords [M, 3], v [M, 3]): the present nodes and their velocities (a node
    that is not listed is skipped in v_c / vx_c); cells are the partition's; v0 [n, 3], B0 [n, 9]: the values accumulated into (default 0,
    PreG2C2PTransfer).  Returns a dict of v, B, C = B Dinv, x (and F [n, 9] or J [n]) with bounds b_v, b_B, b_C, b_x (b_F / b_J)."""
    dxd, dtd = _dx64(dx), float(np.float32(dt))
    cells = partition_cells(keys, side, key_is_origin)
    gc = np.asarray(nodes[0], np.int64).reshape(-1, 3)
    gv = np.asarray(nodes[1], np.float64).reshape(-1, 3)
    o = np.argsort(node_key(gc))
    gc, gv = gc[o], gv[o]
    xp = np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(xp)
    nd = cells[:, None, :] + _O8[None]                                                   # [nc, 8, 3]
    row = _lookup(gc, nd)
    has = (row >= 0)[..., None]
    vi = np.where(has, gv[np.maximum(row, 0)], 0.0)                                      # [nc, 8, 3]
    xi = nd * dxd
    vc = vi.sum(1) / 8.0                                                                 # [nc, 3]
    Tvc = np.abs(vi).sum(1) / 8.0
    vx = np.einsum("kor,koj->kjr", vi, xi).reshape(-1, 9) / 8.0                          # [nc, 9], d = r + 3 j
    Tvx = np.einsum("kor,koj->kjr", np.abs(vi), np.abs(xi)).reshape(-1, 9) / 8.0
    p, c, W, eW = pairs(x, cells, dx, only_cells)
    v0 = np.zeros((n, 3)) if v0 is None else np.asarray(v0, np.float64).reshape(n, 3)
    B0 = np.zeros((n, 9)) if B0 is None else np.asarray(B0, np.float64).reshape(n, 9)
    N = np.bincount(p, minlength=n).astype(np.float64)[:, None] + 1
    v = v0 + _sum(p, vc[c] * W[:, None], n)
    Tv = np.abs(v0) + _sum(p, Tvc[c] * W[:, None], n)
    bv = (N + C2_GV) * U * Tv + _sum(p, Tvc[c] * eW[:, None], n) + (N + C2_GV) * FLT_MIN
    tB = vx[c] - vc[c][:, _ROW] * xp[p][:, _COL]
    mB = Tvx[c] + Tvc[c][:, _ROW] * np.abs(xp[p])[:, _COL]
    Bm = B0 + _sum(p, tB * W[:, None], n)
    TB = np.abs(B0) + _sum(p, mB * W[:, None], n)
    bB = (N + C2_GB) * U * TB + _sum(p, mB * eW[:, None], n) + (N + C2_GB) * FLT_MIN
    Dcol = dinv64(x, dx)[:, _COL]
    Cv = Bm * Dcol
    bC = Dcol * bB + 5 * U * np.abs(Cv) + 5 * FLT_MIN
    out = dict(v=v, b_v=bv, B=Bm, b_B=bB, C=Cv, b_C=bC, x=xp + dtd * v, b_x=2 * U * (np.abs(xp) + dtd * np.abs(v)) + dtd * bv + 2 * FLT_MIN)
    Cm, bCm = _mat(Cv), _mat(bC)
    if F is not None:
        Fm = _mat(F)
        out["F"] = _vec9((np.eye(3)[None] + dtd * Cm) @ Fm)
        out["b_F"] = _vec9((5 * U * (np.eye(3)[None] + dtd * np.abs(Cm)) + dtd * bCm) @ np.abs(Fm) + 5 * FLT_MIN)
    if J is not None:
        J = np.asarray(J, np.float64).reshape(n)
        out["J"] = (1 + dtd * np.trace(Cm, axis1=1, axis2=2)) * J
        out["b_J"] = (4 * U * (1 + dtd * np.abs(np.diagonal(Cm, axis1=1, axis2=2)).sum(1)) + dtd * np.trace(bCm, axis1=1, axis2=2)) * np.abs(J) \
            + 4 * FLT_MIN
    return out
