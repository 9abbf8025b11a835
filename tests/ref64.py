"""Float64 reference of the particle <-> grid transfers with a node-local (and particle-local) error bound.

The transfers have an exact answer: given the float32 inputs and the kernel's own float32 discrete decisions (the base node and the
d0 of the quadratic B-spline, `make_arena` in zpc_amd/csrc/mpm_particles.hpp), weights, scatter, gather, grid update and the F update
involve no approximation.  So every node and every particle is checked against its own bound

    |got - ref| <= (N + c) * u * T + e_in + (N + c) * 2^-126

    u    = 2^-24, the unit roundoff of float32
    N    = number of terms summed into the value (contributors of a node, 27 stencil nodes of a particle)
    T    = sum over the terms of the product of the MAGNITUDES of their factors (cancellation inside or between terms does not
           shrink it); |k dx - lp| is taken as k dx + lp, the magnitude of the float32 subtraction that forms it
    c    = roundings inside one term (derived below, per channel)
    e_in = propagated bound of an input that is itself a kernel result (v, C of the G2P half of a fused step; m, mv of a grid update
           that is checked without the pre-update sums)
    2^-126 per operation: hardware float atomics (-munsafe-fp-atomics) may flush a denormal result to zero.

(N - 1) u T bounds float32 summation in any order or tree (atomics, LDS arenas, register partial sums), so the bound does not depend
on the schedule.  The per-term constants c (first order, each factor's relative error counted once):

    w_k    one axis weight, from the exact float32 d0: 0.5 (1.5 - d0)^2 and 0.5 (d0 - 0.5)^2 round at most 3 times; 0.75 - (d0 - 1)^2
           rounds twice, the square by <= 0.25 u absolute against w >= 0.5: <= 1.5 u.  Each w_k <= 3 u.
    W      w_x w_y w_z: 3 * 3 u + 2 products                                           = 11 u
    xixp   k dx - fl(lpn dx): <= u lp + u |xixp| <= 2 u (k dx + lp)                   =  2 u of X = k dx + lp
    scale  -dt D_inv: D_inv = 4 / dx^2 (<= 3 roundings), the product with dt and with PF F^T vol, and once more for a kernel that
           folds dx into it (fscaleDx)                                                 =  6 u
    mass   m W                                                   C_M  = 11 + 1         = 12
    mv     W m (v + C xixp): products 2 + 1 each, three adds 3, then W (11) and two products: C_MV = 6 + 11 + 2 = 19
    force  W (s PF) xixp: scale 6, products 2 + 1, two adds 2, W 11 and one product:   C_F  = 6 + 5 + 12 = 23
    G2P v  W v_i:                                                C_GV = 11 + 1         = 12
    G2P C  D_inv W v_i xixp: D_inv 3, xixp 2, W 11, three products: C_GC               = 19
    x      x + dt v: two roundings of |x| + dt |v|, plus dt * bound(v)
    F      (I + dt C) F: tmp = I + dt C rounds twice, the 3-term dot three times: 5 u of sum_k (I + dt |C|)_rk |F_kc|, plus
           dt * bound(C) |F|; J <- (1 + dt tr C) J: 4 u of (1 + dt sum |C_dd|) |J|, plus dt sum bound(C_dd) |J|
    grid   v = mv / m + g dt: 3 u of |mv| / m + |g dt|, plus (e_mv + |v| e_m) / m

The arena is reproduced in float32 exactly.  It is restricted to a power-of-two dx: then pos * (1/dx) is exact, the product equals the
oracle's pos / dx and a contracted fma(pos, 1/dx, -0.5) or fma(pos, 1/dx, -fl) returns the same bits as the separate operations, so the
stencil does not depend on FP contraction in the kernels' translation units.  The subtraction X - fl can still round (next to the
origin X has finer ulps than lpn): lpn may round up to 1.5 or X - 0.5 to an integer, and d0 = lpn - floor(lpn - 0.5) then weights the
particle as if one cell away on the unchanged corner, as the reference does (InterpolationKernel.hpp:108 on Utils.hpp:59-60).

Matrices are 9-vectors in column-major order (M[r + 3 c]), as the reference stores F and C.  numpy only.
"""
import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
C_M, C_MV, C_F = 12, 19, 23
C_GRID = np.array([C_M, C_MV, C_MV, C_MV, C_F, C_F, C_F], np.float64)
C_GV, C_GC = 12, 19
_OFF = 1 << 20


def _mat(a):
    """[n, 9] column-major -> [n, 3, 3] indexed [row][col]"""
    return np.asarray(a, np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)


def _vec9(m):
    """[n, 3, 3] [row][col] -> [n, 9] column-major"""
    return m.transpose(0, 2, 1).reshape(-1, 9)


def node_key(coords):
    c = np.asarray(coords, np.int64) + _OFF
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


def arena32(pos, dx):
    """make_arena in float32: (corner [n, 3] int64, lpn [n, 3] f32, d0 [n, 3] f32)"""
    dx32 = np.float32(dx)
    assert np.frexp(dx32)[0] == 0.5, "ref64 needs a power-of-two dx (see the module docstring)"
    dxinv = np.float32(1.0) / dx32
    X = np.asarray(pos, np.float32) * dxinv
    fl = np.floor(X - np.float32(0.5))
    lpn = X - fl
    d0 = lpn - np.floor(lpn - np.float32(0.5))
    return fl.astype(np.int64), lpn, d0


def weights64(d0):
    """[..., 3 axes] d0 -> [..., 3 axes, 3 nodes] quadratic B-spline weights in float64"""
    d = np.asarray(d0, np.float64)
    return np.stack([0.5 * (1.5 - d) ** 2, 0.75 - (d - 1.0) ** 2, 0.5 * (d - 0.5) ** 2], -1)


_K = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(27, 3)  # (a, b, c) loop order


def stencil(pos, dx):
    """nodes [n, 27, 3], W [n, 27], xixp [n, 27, 3] = k dx - lpn dx, X [n, 27, 3] = k dx + lpn dx (its magnitude)"""
    corner, lpn, d0 = arena32(pos, dx)
    w = weights64(d0)
    W = w[:, 0, _K[:, 0]] * w[:, 1, _K[:, 1]] * w[:, 2, _K[:, 2]]
    dxd = float(np.float32(dx))
    kdx = _K[None, :, :] * dxd
    lp = lpn.astype(np.float64)[:, None, :] * dxd
    return corner[:, None, :] + _K[None], W, kdx - lp, kdx + lp


class Grid64:
    """Reference values of the touched nodes: coords [M, 3], val / T / ein [M, 7], N [M], c [7]."""

    def __init__(self, coords, val, T, N, ein, c):
        self.coords, self.val, self.T, self.N, self.ein, self.c = coords, val, T, N, ein, c
        self.keys = node_key(coords)

    def bound(self):
        k = self.N[:, None] + self.c[None, :]
        return k * U * self.T + self.ein + k * FLT_MIN

    def subset(self, rows):
        """the reference restricted to some of its nodes (rows: index or mask)"""
        return Grid64(self.coords[rows], self.val[rows], self.T[rows], self.N[rows], self.ein[rows], self.c)

    def lookup(self, coords):
        """row of every node of coords [..., 3] (-1: not touched)"""
        k = node_key(coords)
        i = np.searchsorted(self.keys, k)
        i = np.minimum(i, len(self.keys) - 1)
        return np.where(self.keys[i] == k, i, -1)


def _accumulate(nodes, cols):
    keys = node_key(nodes).ravel()
    uk, inv = np.unique(keys, return_inverse=True)
    inv = inv.ravel()
    out = [np.stack([np.bincount(inv, weights=c[..., j].ravel(), minlength=len(uk)) for j in range(c.shape[-1])], 1) for c in cols]
    N = np.bincount(inv, minlength=len(uk)).astype(np.float64)
    c = uk.copy()
    coords = np.stack([(c >> 42) - _OFF, ((c >> 21) & ((1 << 21) - 1)) - _OFF, (c & ((1 << 21) - 1)) - _OFF], 1)
    return coords, out, N


def p2g64(mass, pos, vel, C, dx, dt, PF=None, ev=None, eC=None, ePF=None):
    """P2G (oracle/mpm.c orc_mpm_p2g, P2G.hpp:51-125) in float64: Grid64 of channels m, mv (and, with PF = P F^T vol [n, 9], the force
    -dt D_inv PF xixp W).  ev [n, 3], eC [n, 9], ePF [n, 9]: absolute error bounds of those inputs (e_in)."""
    n = len(mass)
    nodes, W, xixp, X = stencil(pos, dx)
    m = np.asarray(mass, np.float64)[:, None]
    v = np.asarray(vel, np.float64)
    Cm = _mat(C)
    mW = m * W
    nch = 4 if PF is None else 7   # (channels 4-6 stay 0 without PF)
    val = np.zeros((n, 27, nch))
    T = np.zeros((n, 27, nch))
    ein = np.zeros((n, 27, nch))
    val[..., 0] = mW
    T[..., 0] = mW
    val[..., 1:4] = mW[..., None] * (v[:, None, :] + np.einsum("ndj,nkj->nkd", Cm, xixp))
    T[..., 1:4] = mW[..., None] * (np.abs(v)[:, None, :] + np.einsum("ndj,nkj->nkd", np.abs(Cm), X))
    if ev is not None:
        ein[..., 1:4] += mW[..., None] * np.asarray(ev, np.float64)[:, None, :]
    if eC is not None:
        ein[..., 1:4] += mW[..., None] * np.einsum("ndj,nkj->nkd", _mat(eC), X)
    dxd = float(np.float32(dx))
    s = float(np.float32(dt)) * 4.0 / (dxd * dxd)
    if PF is not None:
        P = _mat(PF)
        val[..., 4:7] = -s * W[..., None] * np.einsum("ndj,nkj->nkd", P, xixp)
        T[..., 4:7] = s * W[..., None] * np.einsum("ndj,nkj->nkd", np.abs(P), X)
        if ePF is not None:
            ein[..., 4:7] += s * W[..., None] * np.einsum("ndj,nkj->nkd", _mat(ePF), X)
    del W, xixp, X, mW
    coords, out, N = _accumulate(nodes, (val, T, ein))
    val, T, ein = (np.pad(a, ((0, 0), (0, 7 - nch))) for a in out)
    return Grid64(coords, val, T, N, ein, C_GRID.copy())


def eos_pf64(J, bulk, volume):
    """the fluid's P F^T vol without viscosity, -bulk (J^-7 - 1) volume J I, as [n, 9], and its float32 error bound (stress_eos,
    mpm_math.hpp): J^7 from J2, J4 and two products (6 u), the reciprocal (7 u of J^-7), then - 1, * bulk, volume * J and * vol one
    rounding each: <= 11 u of bulk volume |J| (J^-7 + 1) on the diagonal, 0 off it"""
    J = np.asarray(J, np.float64)
    b, vol = float(np.float32(bulk)), float(np.float32(volume))
    p = b * (J ** -7 - 1.0) * vol * J
    e = 11 * U * b * vol * np.abs(J) * (np.abs(J) ** -7 + 1.0) + 11 * FLT_MIN
    PF, ePF = np.zeros((len(J), 9)), np.zeros((len(J), 9))
    for d in (0, 4, 8):
        PF[:, d], ePF[:, d] = -p, e
    return PF, ePF


def grid_update64(m, mv, dt, extf, e_m=None, e_mv=None):
    """GridOp.hpp:71-108 on nodes with mass: v = mv / m + g dt and its bound [M, 3]"""
    m = np.asarray(m, np.float64)[:, None]
    mv = np.asarray(mv, np.float64)
    gdt = np.asarray(extf, np.float64)[None, :] * float(np.float32(dt))
    v = mv / m + gdt
    b = 3 * U * (np.abs(mv) / m + np.abs(gdt)) + 3 * FLT_MIN
    if e_m is not None:
        b = b + (np.asarray(e_mv, np.float64) + np.abs(mv / m) * np.asarray(e_m, np.float64)[:, None]) / m
    return v, b


def g2p64(grid_v, pos, dx, dt, F=None, J=None, ev_node=None):
    """G2P (orc_mpm_g2p, G2P.hpp:44-83) in float64.  grid_v: (coords [M, 3], v [M, 3]) of the node velocities the kernel reads;
    ev_node [M, 3]: their error bound.  Returns a dict of v, C, x (and F [n, 9] or J [n]) with bounds b_v, b_C, b_x (b_F / b_J)."""
    gc, gv = grid_v
    gk = node_key(gc)
    o = np.argsort(gk)
    gk, gv = gk[o], np.asarray(gv, np.float64)[o]
    nodes, W, xixp, X = stencil(pos, dx)
    k = node_key(nodes)
    i = np.minimum(np.searchsorted(gk, k), len(gk) - 1)
    miss = gk[i] != k
    assert not miss.any(), "G2P reads %d nodes outside the partition, e.g. %s" % (int(miss.sum()), nodes[miss][:3].tolist())
    vi = gv[i]                                           # [n, 27, 3]
    evi = np.asarray(ev_node, np.float64)[o][i] if ev_node is not None else np.zeros_like(vi)
    dxd = float(np.float32(dx))
    dtd = float(np.float32(dt))
    Dinv = 4.0 / (dxd * dxd)
    v = np.einsum("nk,nkd->nd", W, vi)
    bv = (27 + C_GV) * U * np.einsum("nk,nkd->nd", W, np.abs(vi)) + np.einsum("nk,nkd->nd", W, evi) + (27 + C_GV) * FLT_MIN
    Cm = Dinv * np.einsum("nk,nkr,nkc->nrc", W, vi, xixp)
    bC = ((27 + C_GC) * U * Dinv * np.einsum("nk,nkr,nkc->nrc", W, np.abs(vi), X) + Dinv * np.einsum("nk,nkr,nkc->nrc", W, evi, X)
          + (27 + C_GC) * FLT_MIN)
    x = np.asarray(pos, np.float64)
    out = dict(v=v, b_v=bv, C=_vec9(Cm), b_C=_vec9(bC), x=x + dtd * v, b_x=2 * U * (np.abs(x) + dtd * np.abs(v)) + dtd * bv + 2 * FLT_MIN)
    if F is not None:
        Fm = _mat(F)
        tmp = np.eye(3)[None] + dtd * Cm
        mag = np.eye(3)[None] + dtd * np.abs(Cm)
        out["F"] = _vec9(tmp @ Fm)
        out["b_F"] = _vec9((5 * U * mag + dtd * bC) @ np.abs(Fm) + 5 * FLT_MIN)
    if J is not None:
        J = np.asarray(J, np.float64)
        tr = np.trace(Cm, axis1=1, axis2=2)
        out["J"] = (1 + dtd * tr) * J
        out["b_J"] = (4 * U * (1 + dtd * np.abs(np.diagonal(Cm, axis1=1, axis2=2)).sum(1)) + dtd * np.trace(bC, axis1=1, axis2=2)) * np.abs(J) \
            + 4 * FLT_MIN
    return out


def world_nodes(keys, grid, side, kscale):
    """partition -> (coords [nb side^3, 3], values [nb side^3, 7]).  keys [nb, 3] in block-number order; grid [nb, 7, side^3] (or
    flat); kscale = cells per key unit (side for block coordinates, 1 when the keys are block origins)."""
    keys = np.asarray(keys, np.int64)
    nb = keys.shape[0]
    g = np.asarray(grid).reshape(nb, 7, side ** 3)
    l = np.arange(side ** 3)
    loc = np.stack([l // (side * side), (l // side) % side, l % side], 1)
    coords = (keys[:, None, :] * kscale + loc[None]).reshape(-1, 3)
    return coords, g.transpose(0, 2, 1).reshape(-1, 7).astype(np.float64)


def to_world_nodes(mt):
    """an MpmTransfer's partition and grid as world nodes, for both key conventions (key_is_origin: keys are block origins)"""
    return world_nodes(mt.active_keys(), mt.grid.cpu().numpy(), mt.side, mt.side // mt.kstride)


def _report(what, ratio, err, got, want, bnd, extra, k=5):
    worst = np.argsort(ratio.ravel())[::-1][:k]
    rows = []
    for f in worst:
        i, ch = np.unravel_index(f, ratio.shape)
        rows.append("%s ch %d: got %.9g want %.9g |err| %.3g bound %.3g (%.2fx)%s" % (extra(i), ch, got[i, ch], want[i, ch], err[i, ch], bnd[i, ch],
                                                                                 ratio[i, ch], ""))
    return "%s: %d values over their bound\n  " % (what, int((ratio > 1).sum())) + "\n  ".join(rows)


def check_grid(ref, world, channels=range(7), what="grid", bound=None):
    """Node-local check of a partition's grid (world = (coords, values) of every partition node) against a Grid64: every node the
    reference touches exists, is within its bound on every channel of `channels`, and every other node is exactly 0 on those channels
    (a missed clear, a stray write).  Returns the worst err / bound per channel (nan for the channels not checked)."""
    ch = np.asarray(list(channels))
    gc, gv = world
    gk = node_key(gc)
    o = np.argsort(gk)
    gks = gk[o]
    i = np.minimum(np.searchsorted(gks, ref.keys), len(gks) - 1)
    miss = gks[i] != ref.keys
    assert not miss.any(), "%s: %d touched nodes are not in the partition, e.g. %s" % (what, int(miss.sum()), ref.coords[miss][:3].tolist())
    rows = o[i]
    stray = np.ones(len(gk), bool)
    stray[rows] = False
    sv = gv[stray][:, ch]
    assert (sv == 0).all(), "%s: %d untouched nodes are not 0, e.g. %s = %s" % (
        what, int((sv != 0).any(1).sum()), gc[stray][(sv != 0).any(1)][:3].tolist(), sv[(sv != 0).any(1)][:3].tolist())
    got = gv[rows][:, ch]
    want = ref.val[:, ch]
    bnd = (ref.bound() if bound is None else bound)[:, ch]
    err = np.abs(got - want)
    ratio = err / bnd
    if not (ratio <= 1).all():
        raise AssertionError(_report(what, ratio, err, got, want, bnd,
                                     lambda r: "node %s N=%d T=%.3g" % (ref.coords[r].tolist(), ref.N[r], ref.T[r, ch].max())))
    out = np.full(7, np.nan)
    out[ch] = ratio.max(0) if len(ratio) else 0.0
    return out


def check_particles(got, want, bound, what="particles"):
    """per-particle, per-component check; returns the worst err / bound"""
    got = np.asarray(got, np.float64).reshape(len(want), -1)
    want = np.asarray(want, np.float64).reshape(len(got), -1)
    bnd = np.asarray(bound, np.float64).reshape(want.shape)
    err = np.abs(got - want)
    ratio = err / bnd
    if not (ratio <= 1).all():
        raise AssertionError(_report(what, ratio, err, got, want, bnd, lambda r: "particle %d" % r))
    return float(ratio.max())
