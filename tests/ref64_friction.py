"""Float64 restatement of lagged IPC friction on mesh proximity pairs (include/zensim_rocm/friction_device.hpp, the friction operations of
zpc_amd/csrc/mesh_barrier.hip), numpy plus torch float64 on the CPU, on top of ref64_barrier / ref64_proximity / ref64_mesh: the lag record
and the closed forms of energy, gradient and Hessian-vector product, the same energy on the reference's per-feature tangent bases (for
torch.autograd), a float32 replay of the device chain operation by operation, and the bounds on the float32 result.

Model.  Lag, at the positions the contact forces are frozen at:  r = P - Q, d = |r|, n = r / d, lambda = m (-b'(d2)) 2 d, w the weights
of the barrier gradient.  Evaluation at a displacement u with mu and eps (the threshold eps_v):
    ur = sum_k w_k u_k,  ut = ur - (n . ur) n,  y = |ut|
    energy    mu lambda f0(y),      f0 = y (y >= eps), else y^2 (eps - y / 3) / eps^2 + eps / 3
    gradient  mu lambda c1 w_k ut,  c1 = 1 / y (y >= eps), else (2 eps - y) / eps^2
    product   mu lambda w_k (c1 zt + c2 (ut . zt) ut),  zt the tangential part of sum_k w_k x_k,  c2 = -1 / y^3, else -1 / (eps^2 y)

The bounds, with u = 2^-24 (U).  Lag: everything starts, as in ref64_barrier.py, from the distance bound delta of ref64_proximity.py and
from the spread over the eligible candidates of tri_closest / ee_closest, which ref64_barrier._spread computes for the weights and for r
(Dw_k, Dr); b' and its deviation Db' over [d - delta, d + delta] come from ref64_barrier._scalar_bounds, the mollifier's Dm is restated
from ref64_barrier.ee_pairs64.
  lambda   lambda = m (-b') 2 d with d = sqrtf(d2) (one more rounding, u d, on top of delta):
           Dlambda = 2 ((m + Dm)(|b'| + Db')(d + delta + u d) - m |b'| d) + 4 u |lambda|   (the products m b', 2 d, their product: 3, stated 4)
  n        n = r / d:  |r32 / d32 - r / d| <= Dr / d32 + |r| |1 / d32 - 1 / d| <= (Dr + delta + u d) / (d - delta), the division 1 more
           rounding on a unit vector: Dn = (Dr + delta + u d) / (d - delta) + 2 u.  d - delta <= 0: infinite, the pair stays in.
  w        Dw_k of the spread, at most 1.
  parallel EE only.  The spread counts the parameters of the common perpendicular to first order, 16 u S / (|e| sin(angle)).  Between nearly
           parallel edges the float32 cross product n = u x v also turns by 3 u / sin, which moves s = (v x w) . n / |n|^2 by
           3 u |w| / (|u| sin^2): at sin = 2e-5 (above the threshold of ee_closest) the float32 interior candidate is any point pair,
           and it is returned when its distance ties with the boundary candidates'.  So Dr and Dw_k get one more term, the second-order
           parameter error 16 u S / (|e| sin^2) (times the edge lengths for r), and for r at most what ANY point pair within 2 delta of
           the minimum allows: the vectors r(s, t) form a convex set whose shortest element is r, so r . (r' - r) >= 0 and
           |r' - r|^2 <= |r'|^2 - |r|^2 <= (d + 2 delta)^2 - d^2: sqrt(4 d delta + 4 delta^2), plus the rounding of the points, 8 u (S + M).
Evaluation, counting the roundings of the chain W u -> projection -> norm -> f on top of what the record's deviation propagates to:
  W u      z = sum_k w_k u_k, four products and three additions per component, every term through at most 4 roundings:
           Dz = sum_k Dw_k |u_k| + 4 u A,  A = sum_k (|w_k| + Dw_k) |u_k|
  project  t = z - (n . z) n.  With the exact unit n the projector is a contraction; n32 n32^T - n n^T is at most Dn (2 + Dn); the dot
           product (3 products, 2 additions), its product with n and the subtraction: 6 roundings on |z| (1 + Dn)^2, stated 8:
           Dt = Dz + Dn (2 + Dn)(|z| + Dz) + 8 u (|z| + Dz)(1 + Dn)^2
  norm     y = sqrt(t . t): 3 squares, 2 additions, the root: relative 3 u:  Dy = Dt + 3 u (y + Dt)
  f0       f0' = c1 y lies in [0, 1], so f0 moves by at most Dy.  Below the threshold y2 (eps - y / 3) / eps^2 + eps / 3 has 7 roundings
           on positive terms (eps - y / 3 >= 2 eps / 3: no cancellation), above it none:  Df0 = Dy + 8 u f0.  The branch follows the
           float32 y; f0 is one C^2 function, so a branch that differs from the reference's changes nothing in this argument.
  energy   E = mu lambda f0:  DE = mu ((lambda + Dlambda)(f0 + Df0) - lambda f0) + 2 u |E|
  G        G(ut) = c1(|ut|) ut, the friction force per unit mu lambda.  Its Jacobian c1 I + c2 ut ut^T has the eigenvalues c1 (across ut)
           and c1 + c2 y^2 = f0'' (along), both in [0, c1], and c1 decreases in y: G is Lipschitz with constant c1(ylo), ylo =
           max(y - Dt, 0).  c1 itself: 2 eps - y >= eps (1 rounding, relative 2 u), eps^2 1, the division 1, and the 3 u of the float32 y
           moves c1 by at most 3 u c1 (|y c1' / c1| <= 1 on both branches): 8 u.
           DG = c1(ylo) Dt + 8 u (|G| + c1(ylo) Dt), and never more than |G| + 1 + 16 u: |G| = f0' <= 1 wherever ut is; likewise
           DH below never more than |M zt| + (2 / eps)(|zt| + Dzt)(1 + 40 u), from |M| <= c1 <= 2 / eps
  gradient g_k = mu lambda w_k G:  Dg_k = mu ((lambda + Dlambda)(|w_k| + Dw_k)(|G| + DG) - lambda |w_k| |G|) + 4 u |g_k|
  M zt     M(ut) = c1 I + c2 ut ut^T, |M| <= c1.  dM/dut in a direction e: c2 y (t . e) I + c2' y^2 (t . e) t t^T + c2 (e ut^T + ut e^T),
           t = ut / y: below the threshold (1 + 1 + 2) / eps^2, above it (1 + 3 + 2) / y^2; K(ylo) = 6 / max(ylo, eps)^2 covers both.
           Roundings: c1 8 u and the product c1 zt 1 on c1 |zt|; c2 (y3 = y2 y carries 3 x 3 u, the division 1, stated 12 u), ut . zt 3 u,
           their product 1, times ut 1, on |c2| y^2 |zt| <= c1 |zt|; the sum and the three products with mu lambda w_k: 4; 33, stated
           40 u c1 |zt|, RELATIVE TO c1 |zt| and not to |M zt|: above the threshold the component along ut cancels to f0'' = 0.
           DH = K(ylo) Dt (|zt| + Dzt) + c1(ylo) Dzt + 40 u c1(ylo)(|zt| + Dzt),  Dzt as Dt for the rows of x
  product  h_k = mu lambda w_k M zt:  Dh_k = mu ((lambda + Dlambda)(|w_k| + Dw_k)(|M zt| + DH) - lambda |w_k| |M zt|) + 4 u |h_k|
  vertex   the sum of the bounds of its incident (pair, corner) terms plus n_inc u sum |term| for the float32 accumulation.
A pair at zero distance has an all-zero record on both sides and an infinite lag bound (its interval reaches zero).
"""
import numpy as np

import ref64_barrier as rb
import ref64_mesh as rm
import ref64_proximity as rp
import ref64_terms as rt
from ref64_mesh import U, _dot, _cross

FLT_MAX, FLT_MIN = rb.FLT_MAX, rb.FLT_MIN
# the vacuity guard of tests/test_friction_gpu.py: the median over the contact vertices of scene `sheets` (dhat of the scene, kappa = 1,
# mollified, rest = the scene, u = displacement(nv, 1, EPS_V), mu = MU) of bound / |g|, measured by tests/test_friction_cpu.py with the
# float64 reference alone: 4.948e-03 (the barrier's own: 1.715e-03)
SHEETS_MEDIAN_BOUND_OVER_G = 4.948e-3
MU, EPS_V = 0.4, 1e-3
SCALES = (0.01, 1.0, 100.0)      # displacement scales in units of eps_v


def _norm(x):
    return np.sqrt(_dot(x, x))


def displacement(nv, seed, scale):
    """a seeded displacement [nv, 3] of typical size scale, rounded to float32 (the numbers the device gets)"""
    return (scale * np.random.default_rng(2000 + seed).standard_normal((nv, 3))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the scalar functions
def f0(y, eps):
    y = np.asarray(y, np.float64)
    return np.where(y >= eps, y, y * y * (eps - y / 3) / (eps * eps) + eps / 3)


def c1(y, eps):
    y = np.asarray(y, np.float64)
    return np.where(y >= eps, 1 / np.where(y >= eps, y, 1.0), (2 * eps - y) / (eps * eps))


def c2(y, eps):
    """0 at y = 0: the term it multiplies, (ut . zt) ut, vanishes there"""
    y = np.asarray(y, np.float64)
    y1 = np.where(y > 0, y, 1.0)
    return np.where(y > 0, np.where(y >= eps, -1 / y1 ** 3, -1 / (eps * eps * y1)), 0.0)


# ------------------------------------------------------------------------------------------------ the lag record in float64
def _spied(fn, *args):
    """fn(*args) (ref64_barrier.pt_pairs64 / ee_pairs64) and what its call of ref64_barrier._spread saw and returned: the reference's
    weights and r, their spreads Dw [n, 4] and Dr [n] over the eligible candidates, and the number of those candidates"""
    seen, orig = {}, rb._spread

    def spy(d, delta, dc, elig, wc, rc, dwc, drc, wref, rref):
        dw, dr = orig(d, delta, dc, elig, wc, rc, dwc, drc, wref, rref)
        seen.update(w=wref, r=rref, dw=dw, dr=dr, ncand=(elig & (dc <= (d + 2 * delta)[:, None])).sum(axis=1))
        return dw, dr
    rb._spread = spy
    try:
        return fn(*args), seen
    finally:
        rb._spread = orig


def _lag(q, s, m, dm, dhat2, kappa):
    """the record and its bounds from a pair dict of ref64_barrier (q), the spied spread (s) and the mollifier"""
    d, delta = q["d"], q["delta"]
    _, bp, _, dbp = rb._scalar_bounds(d, delta, dhat2, kappa)
    act = (d * d < dhat2) & (d > 0)
    d1 = np.where(act, d, 1.0)
    lam = np.where(act, m * -bp * 2 * d, 0.0)
    # n = r / |r|, not r / d: the same number, but d comes out of the distance chain and |r| out of the closest points, and at d = 1e-7
    # (pairs of `stack`) the two differ by 1e-9 in float64 -- a normal that is not a unit vector leaves that much of n . ur in ut
    lr = _norm(s["r"])
    n = np.where(act[:, None], s["r"] / np.where(act & (lr > 0), lr, d1)[:, None], 0.0)
    w = np.where(act[:, None], s["w"], 0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dlam = 2 * ((m + dm) * (np.abs(bp) + dbp) * (d + delta + U * d) - m * np.abs(bp) * d) + 4 * U * lam
        lo = d - delta
        dn = np.where(lo > 0, (s["dr"] + delta + U * d) / np.where(lo > 0, lo, 1.0) + 2 * U, np.inf)
    # within delta of dHat the float32 pair may be on the other side: one record is all zero, the other has a unit n and weights of order
    # one next to a lambda that vanishes there.  lambda is covered by its interval (b' is continuous and 0 beyond dHat); n and w are not
    # bounded, and neither is what is computed from them
    grey = np.abs(d - np.sqrt(dhat2)) <= delta
    open_ = grey | q["zero"]
    dlam = np.where(np.isfinite(dlam), dlam, np.inf)
    dn = np.where(open_, np.inf, dn)
    dw = np.where(open_[:, None], np.inf, np.where(act[:, None], s["dw"], 0.0))
    rec = np.concatenate([n, lam[:, None], w], axis=1)
    return dict(rec=rec, n=n, lam=lam, w=w, dn=dn, dlam=dlam, dw=dw, vert=q["vert"], zero=q["zero"], d=d, delta=delta, ncand=s["ncand"],
                act=act)


def lag_pt64(verts, tris, pairs, dhat2, kappa, M=None):
    """dict(rec [n, 8] = (n, lambda, w), n, lam, w, dn [n], dlam [n], dw [n, 4], vert [n, 4], zero, d, delta, ncand, act) of the (vertex,
    triangle) pairs"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    q, s = _spied(rb.pt_pairs64, verts, tris, pairs, dhat2, kappa, M)
    z = np.zeros(len(pairs))
    return _lag(q, s, z + 1, z, dhat2, kappa)


def lag_ee64(verts, edge_list, pairs, dhat2, kappa, rest2=None, M=None):
    """the same of the (edge, edge) pairs; rest2 [ne]: squared rest lengths (None: unmollified)"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    q, s = _spied(rb.ee_pairs64, verts, edge_list, pairs, dhat2, kappa, rest2, M)
    # Dm as ref64_barrier.ee_pairs64 states it (its docstring has the count)
    v, e = rp._v64(verts), np.asarray(edge_list, np.int64).reshape(-1, 2)
    a0, a1, b0, b1 = rb._ee_vertices(v, e, pairs)
    uu, vv = a1 - a0, b1 - b0
    lu, lv = _norm(uu), _norm(vv)
    nrm = _cross(uu, vv)
    c = _dot(nrm, nrm)
    n = len(pairs)
    eps = np.zeros(n) if rest2 is None else 1e-2 * np.asarray(rest2, np.float64)[pairs[:, 0]] * np.asarray(rest2, np.float64)[pairs[:, 1]]
    eps = np.where(eps >= FLT_MIN, eps, 0.0)
    dnn = 10 * U * lu * lv
    dcc = 2 * np.sqrt(c) * dnn + dnn * dnn + 3 * U * c
    e1 = np.where(eps > 0, eps, 1.0)
    dx = np.where(eps > 0, dcc / e1 + 17 * U * c / e1, 0.0)
    dm = np.where(eps > 0, np.minimum(2 * dx + 3 * U * q["m"], 1.0), 0.0)
    dm = np.where((eps > 0) & (c / e1 - dx >= 1), 0.0, dm)
    # nearly parallel edges (the docstring): the second-order error of the float32 interior candidate
    d, delta = q["d"], q["delta"]
    S = d + lu + lv
    M = rp.coord_max(verts) if M is None else M
    with np.errstate(divide="ignore", invalid="ignore"):
        sin = np.where(c > 0, np.sqrt(c) / np.where(lu * lv > 0, lu * lv, 1.0), 0.0)
        es2 = np.where(sin > 0, rb.K_TRIPLE * U * S / np.where(sin > 0, lu * sin * sin, 1.0), np.inf)
        et2 = np.where(sin > 0, rb.K_TRIPLE * U * S / np.where(sin > 0, lv * sin * sin, 1.0), np.inf)
    convex = np.sqrt(4 * d * delta + 4 * delta * delta) + rb.K_POINT * U * (S + M)
    s["dr"] = s["dr"] + np.minimum(np.where(np.isfinite(es2), es2 * lu + et2 * lv, np.inf), convex)
    s["dw"] = np.minimum(s["dw"] + np.minimum(np.stack([es2, es2, et2, et2], axis=1), 1.0), 1.0)
    return _lag(q, s, q["m"], dm, dhat2, kappa)


# ------------------------------------------------------------------------------------------------ the evaluation in float64
def _tangent(n, w, rows):
    z = (w[:, :, None] * rows).sum(axis=1)
    return z, z - _dot(n, z)[:, None] * n


def evaluate64(rec, urows, mu, eps, xrows=None):
    """dict(e [n], g [n, 4, 3], h [n, 4, 3] or None, y, ut, zt) of records rec [n, 8] at the corner rows urows [n, 4, 3] (and the direction's
    rows xrows)"""
    rec, urows = np.asarray(rec, np.float64), np.asarray(urows, np.float64)
    n, lam, w = rec[:, :3], rec[:, 3], rec[:, 4:]
    _, ut = _tangent(n, w, urows)
    y = _norm(ut)
    k1 = c1(y, eps)
    out = dict(y=y, ut=ut, e=mu * lam * f0(y, eps), g=(mu * lam * k1)[:, None, None] * w[:, :, None] * ut[:, None, :], h=None, zt=None)
    if xrows is not None:
        _, zt = _tangent(n, w, np.asarray(xrows, np.float64))
        m = k1[:, None] * zt + (c2(y, eps) * _dot(ut, zt))[:, None] * ut
        out.update(h=(mu * lam)[:, None, None] * w[:, :, None] * m[:, None, :], zt=zt, mzt=m)
    return out


def _tangent_bound(q, rows):
    """(|z|, Dt) of the docstring for the corner rows [n, 4, 3]"""
    rows = np.asarray(rows, np.float64)
    an = _norm(rows)
    dw = np.where(np.isfinite(q["dw"]), q["dw"], 1.0)
    z, _ = _tangent(q["n"], q["w"], rows)
    A = ((np.abs(q["w"]) + dw) * an).sum(axis=1)
    dz = (dw * an).sum(axis=1) + 4 * U * A
    dn = q["dn"]
    with np.errstate(invalid="ignore", over="ignore"):
        dt = dz + dn * (2 + dn) * (_norm(z) + dz) + 8 * U * (_norm(z) + dz) * (1 + dn) ** 2
    # an all-zero float64 record against a float32 record that is not (the grey zone at dHat): n32 is a unit vector
    dt = np.where(np.isfinite(dt), dt, np.inf)
    return _norm(z), dt


def evaluate_bounds(q, ev, urows, mu, eps, xrows=None):
    """(DE [n], Dg [n, 4], Dh [n, 4] or None) of the docstring for the lag dict q and its evaluation ev = evaluate64(q["rec"], ..)"""
    lam, dlam, aw = q["lam"], q["dlam"], np.abs(q["w"])
    dw = q["dw"]
    y = ev["y"]
    _, dt = _tangent_bound(q, urows)
    with np.errstate(invalid="ignore", over="ignore"):
        dy = dt + 3 * U * (y + dt)
        f = f0(y, eps)
        df0 = dy + 8 * U * f
        de = mu * ((lam + dlam) * (f + df0) - lam * f) + 2 * U * np.abs(ev["e"])
        ylo = np.maximum(y - np.where(np.isfinite(dt), dt, y), 0.0)
        k1 = c1(ylo, eps)
        G = c1(y, eps) * y
        dG = np.minimum(k1 * dt + 8 * U * (G + k1 * dt), G + 1 + 16 * U)      # |G| = f0' <= 1 wherever ut is
        dg = mu * ((lam + dlam)[:, None] * (aw + dw) * (G + dG)[:, None] - (lam * G)[:, None] * aw) + 4 * U * _norm(ev["g"])
        dh = None
        if xrows is not None:
            _, dzt = _tangent_bound(q, xrows)
            azt, am = _norm(ev["zt"]), _norm(ev["mzt"])
            K = 6 / np.maximum(ylo, eps) ** 2
            dH = K * dt * (azt + dzt) + k1 * dzt + 40 * U * k1 * (azt + dzt)
            dH = np.where(np.isnan(dH), np.inf, dH)
            dH = np.minimum(dH, am + (2 / eps) * (azt + dzt) * (1 + 40 * U))      # |M| <= c1 <= 2 / eps wherever ut is
            dh = mu * ((lam + dlam)[:, None] * (aw + dw) * (am + dH)[:, None] - (lam * am)[:, None] * aw) + 4 * U * _norm(ev["h"])
            dh = np.where(np.isnan(dh), np.inf, dh)
    # mu = 0, or a record that is zero on both sides for certain: exactly zero
    sure = (mu == 0) | ((lam == 0) & (dlam == 0))
    de = np.where(sure, 0.0, np.where(np.isnan(de), np.inf, de))
    dg = np.where(sure[:, None], 0.0, np.where(np.isnan(dg), np.inf, dg))
    if dh is not None:
        dh = np.where(sure[:, None], 0.0, dh)
    return de, dg, dh


# ------------------------------------------------------------------------------------------------ a scene
class Reference:
    """lag and evaluation of a constraint set, both in float64: the lag at positions verts, the evaluation at the displacement u [nv, 3]
    (and the direction x).  pt / ee: the lag dicts with ev (evaluate64) and be, bg, bh (evaluate_bounds); record [npt + nee, 8]; pt_e,
    ee_e, energy, grad [nv, 3], hx [nv, 3], pair_g / pair_h [npt + nee, 4, 3], vbound_g / vbound_h [nv], ninc [nv], zero = (pt, ee)"""

    def __init__(self, verts, tris, pt_pairs, ee_pairs, dhat, kappa, u, mu, eps, x=None, rest2=None, edge_list=None):
        nv = len(rp._v64(verts))
        self.dhat2 = rb.dhat2_f32(dhat)
        e = rp.edges(tris) if edge_list is None else edge_list
        M = rp.coord_max(verts)
        u = np.asarray(np.asarray(u, np.float32), np.float64)
        x = None if x is None else np.asarray(np.asarray(x, np.float32), np.float64)
        self.pt = lag_pt64(verts, tris, np.zeros((0, 2), int) if pt_pairs is None else pt_pairs, self.dhat2, kappa, M)
        self.ee = lag_ee64(verts, e, np.zeros((0, 2), int) if ee_pairs is None else ee_pairs, self.dhat2, kappa, rest2, M)
        self.zero = (int(self.pt["zero"].sum()), int(self.ee["zero"].sum()))
        self.grad, self.hx = np.zeros((nv, 3)), (None if x is None else np.zeros((nv, 3)))
        self.vbound_g, self.vbound_h, self.ninc = np.zeros(nv), np.zeros(nv), np.zeros(nv, np.int64)
        mg, mh = np.zeros(nv), np.zeros(nv)
        for q in (self.pt, self.ee):
            xr = None if x is None else x[q["vert"]]
            q["ev"] = evaluate64(q["rec"], u[q["vert"]], mu, eps, xr)
            q["be"], q["bg"], q["bh"] = evaluate_bounds(q, q["ev"], u[q["vert"]], mu, eps, xr)
            idx = q["vert"].ravel()
            np.add.at(self.ninc, idx, 1)
            for out, bound, mag, terms, b in ((self.grad, self.vbound_g, mg, q["ev"]["g"], q["bg"]), (self.hx, self.vbound_h, mh, q["ev"]["h"], q["bh"])):
                if terms is None:
                    continue
                np.add.at(out, idx, terms.reshape(-1, 3))
                np.add.at(bound, idx, b.ravel())
                np.add.at(mag, idx, (_norm(terms) + np.where(np.isfinite(b), b, 0.0)).ravel())
        self.record = np.concatenate([self.pt["rec"], self.ee["rec"]])
        self.pt_e, self.ee_e, self.pt_be, self.ee_be = self.pt["ev"]["e"], self.ee["ev"]["e"], self.pt["be"], self.ee["be"]
        self.energy = float(self.pt_e.sum() + self.ee_e.sum())
        self.energy_bound = float(self.pt_be.sum() + self.ee_be.sum())
        self.pair_g = np.concatenate([self.pt["ev"]["g"], self.ee["ev"]["g"]])
        self.pair_h = None if x is None else np.concatenate([self.pt["ev"]["h"], self.ee["ev"]["h"]])
        self.vbound_g = self.vbound_g + self.ninc * U * mg + 1e-37
        self.vbound_h = self.vbound_h + self.ninc * U * mh + 1e-37


# ------------------------------------------------------------------------------------------------ the reference's tangent bases
def _unit(x):
    return x / _norm(x)[..., None]


def basis_point_point(p0, p1):
    """point_point_tangent_basis: two unit vectors across p1 - p0, the first from the larger of its cross products with the x and y axes"""
    v = p1 - p0
    xc = np.stack([np.zeros(len(v)), -v[:, 2], v[:, 1]], axis=1)
    yc = np.stack([v[:, 2], np.zeros(len(v)), -v[:, 0]], axis=1)
    first = np.where((_dot(xc, xc) > _dot(yc, yc))[:, None], xc, yc)
    return np.stack([_unit(first), _unit(_cross(v, first))], axis=2)


def basis_point_edge(p, e0, e1):
    """point_edge_tangent_basis: along the edge, and across the plane of the edge and the point"""
    e = e1 - e0
    return np.stack([_unit(e), _unit(_cross(e, p - e0))], axis=2)


def basis_point_triangle(a, b, c):
    """point_triangle_tangent_basis: two unit vectors of the triangle's plane"""
    e = b - a
    return np.stack([_unit(e), _unit(_cross(_cross(e, c - a), e))], axis=2)


def basis_edge_edge(a0, a1, b0, b1):
    """edge_edge_tangent_basis: two unit vectors of the plane both edges are parallel to"""
    e = a1 - a0
    return np.stack([_unit(e), _unit(_cross(_cross(e, b1 - b0), e))], axis=2)


def bases_pt(verts, tris, pairs):
    """the reference's basis [n, 3, 2] of every (vertex, triangle) pair, chosen by the feature tri_closest reports"""
    v, t = rp._v64(verts), np.asarray(tris, np.int64).reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    p, a, b, c = v[pairs[:, 0]], v[t[pairs[:, 1], 0]], v[t[pairs[:, 1], 1]], v[t[pairs[:, 1], 2]]
    feat = rm.tri_closest(p, a, b, c)[3]
    T = np.zeros((len(pairs), 3, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, q in ((rm.VERT_A, a), (rm.VERT_B, b), (rm.VERT_C, c)):
            T = np.where((feat == k)[:, None, None], basis_point_point(p, q), T)
        for k, (e0, e1) in ((rm.EDGE_AB, (a, b)), (rm.EDGE_BC, (b, c)), (rm.EDGE_CA, (c, a))):
            T = np.where((feat == k)[:, None, None], basis_point_edge(p, e0, e1), T)
        T = np.where((feat == rm.FACE)[:, None, None], basis_point_triangle(a, b, c), T)
    return T


def bases_ee(verts, edge_list, pairs):
    """the same of the (edge, edge) pairs by the category ee_closest reports: both parameters interior: the edge-edge basis; one at an end:
    that end point against the other edge; both at an end: the two end points"""
    v, e = rp._v64(verts), np.asarray(edge_list, np.int64).reshape(-1, 2)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    a0, a1, b0, b1 = rb._ee_vertices(v, e, pairs)
    cat = rp.ee_closest(a0, a1, b0, b1)[3]
    cs, ct = cat // 3, cat % 3
    pa, pb = np.where((cs == rp.SECOND)[:, None], a1, a0), np.where((ct == rp.SECOND)[:, None], b1, b0)
    si, ti = cs == rp.INTERIOR, ct == rp.INTERIOR
    with np.errstate(invalid="ignore", divide="ignore"):
        T = basis_point_point(pa, pb)
        T = np.where((si & ~ti)[:, None, None], basis_point_edge(pb, a0, a1), T)
        T = np.where((~si & ti)[:, None, None], basis_point_edge(pa, b0, b1), T)
        T = np.where((si & ti)[:, None, None], basis_edge_edge(a0, a1, b0, b1), T)
    return T


def basis_energy_autograd(T, lam, w, vert, u, mu, eps, dirs=()):
    """(energy, gradient [nv, 3], [H x for x in dirs]) of sum mu lam f0(|T^T ur|) with torch.autograd in float64: backward for the gradient,
    double backward for the products"""
    import torch
    Tt, lt, wt = (torch.as_tensor(np.asarray(a, np.float64)) for a in (T, lam, w))
    idx = torch.as_tensor(np.asarray(vert, np.int64))
    x = torch.tensor(np.asarray(u, np.float64), requires_grad=True)
    ur = (wt[:, :, None] * x[idx]).sum(dim=1)
    tan = torch.einsum("ndk,nd->nk", Tt, ur)
    y = torch.sqrt((tan * tan).sum(dim=1))
    f = torch.where(y >= eps, y, y * y * (eps - y / 3) / (eps * eps) + eps / 3)
    energy = (mu * lt * f).sum()
    g, = torch.autograd.grad(energy, x, create_graph=True)
    hx = [torch.autograd.grad((g * torch.as_tensor(np.asarray(d, np.float64))).sum(), x, retain_graph=True)[0].numpy().copy() for d in dirs]
    return float(energy.detach()), g.detach().numpy().copy(), hx


# ------------------------------------------------------------------------------------------------ the float32 replay of the device chain
def _f32(x):
    return np.asarray(x, np.float32)


def _lag_finish32(r, d2, w, bp, m, st):
    """friction_lag_finish: (record [n, 8], status)"""
    f = np.float32
    with np.errstate(all="ignore"):
        act = st == 1
        d = np.sqrt(np.where(act, d2, f(1))).astype(f)
        lam = (m * -bp) * (f(2) * d)
        n = r / d[:, None]
        ok = (np.abs(lam) <= f(FLT_MAX)) & (np.abs(n) <= f(FLT_MAX)).all(axis=1)
    status = np.where(act & ~ok, 2, st).astype(np.int32)
    rec = np.concatenate([n, lam[:, None], w], axis=1).astype(f)
    return np.where((status == 1)[:, None], rec, f(0)).astype(f), status


def lag_pt32(p, a, b, c, dhat2, kappa, log=np.log):
    """friction_lag_pt: (record [n, 8], status, d2) in float32"""
    f = np.float32
    p, a, b, c = (_f32(x) for x in (p, a, b, c))
    d2, cp, bary, _ = rm.tri_closest(p, a, b, c, degenerate=rm.DEGENERATE32)
    _, bp, st = rb.barrier32(d2, dhat2, kappa, log)
    w = np.stack([np.ones_like(bp), -bary[:, 0], -bary[:, 1], -bary[:, 2]], axis=1).astype(f)
    rec, st = _lag_finish32(p - cp, d2, w, bp, np.ones_like(bp), st)
    return rec, st, d2


def lag_ee32(a0, a1, b0, b1, dhat2, kappa, eps, log=np.log):
    """friction_lag_ee: the same; eps [n] float32, 0 = unmollified"""
    f = np.float32
    a0, a1, b0, b1 = (_f32(x) for x in (a0, a1, b0, b1))
    eps = np.broadcast_to(_f32(eps), a0.shape[:1])
    d2, s, t, _, _ = rp.ee_closest(a0, a1, b0, b1, parallel=rp.PARALLEL32)
    s, t = s.astype(f), t.astype(f)
    _, bp, st = rb.barrier32(d2, dhat2, kappa, log)
    u, v = a1 - a0, b1 - b0
    n = _cross(u, v)
    c = _dot(n, n)
    with np.errstate(all="ignore"):
        on = (eps >= f(FLT_MIN)) & (c < eps)
        x = c / np.where(on, eps, f(1))
        m = np.where(on, (f(2) - x) * x, f(1)).astype(f)
        w = np.stack([f(1) - s, s, -(f(1) - t), -t], axis=1).astype(f)
        r = (a0 + s[:, None] * u) - (b0 + t[:, None] * v)
    rec, st = _lag_finish32(r, d2, w, bp, m, st)
    return rec, st, d2


def _tangent32(rec, rows):
    n, w = rec[:, :3], rec[:, 4:]
    with np.errstate(all="ignore"):
        z = w[:, 0, None] * rows[:, 0] + w[:, 1, None] * rows[:, 1] + w[:, 2, None] * rows[:, 2] + w[:, 3, None] * rows[:, 3]
        return z - _dot(n, z)[:, None] * n


def _finish32(t, st):
    """barrier_hvp_finish: terms beyond the float range make the pair ZERO"""
    with np.errstate(invalid="ignore"):
        ok = (np.abs(t) <= np.float32(FLT_MAX)).all(axis=(1, 2))
    st = np.where((st == 1) & ~ok, 2, st).astype(np.int32)
    return np.where((st == 1)[:, None, None], t, np.float32(0)).astype(np.float32), st


def evaluate32(rec, urows, mu, eps, xrows=None):
    """friction_energy / friction_gradient / friction_product in numpy float32 on records rec [n, 8] and rows [n, 4, 3]: dict(e, st_e of the
    energy call; eg, g, st_g of the gradient call; h, st_h of the product call), status 0 idle / 1 active / 2 overflow"""
    f = np.float32
    rec, urows, mu, eps = _f32(rec), _f32(urows), _f32(mu), _f32(eps)      # mu and eps: scalars or [n]
    lam, w = rec[:, 3], rec[:, 4:]
    with np.errstate(all="ignore"):
        scale = mu * lam
        idle = scale == 0
        ut = _tangent32(rec, urows)
        y2 = _dot(ut, ut)
        y = np.sqrt(y2).astype(f)
        fy = np.where(y >= eps, y, (y2 * (eps - y / f(3))) / (eps * eps) + eps / f(3)).astype(f)
        e = scale * fy
        ok = (y2 <= f(FLT_MAX)) & (np.abs(e) <= f(FLT_MAX))
        st_e = np.where(idle, 0, np.where(ok, 1, 2)).astype(np.int32)
        k1 = np.where(y >= eps, f(1) / y, (f(2) * eps - y) / (eps * eps)).astype(f)
        g = ((scale * k1)[:, None] * w)[:, :, None] * ut[:, None, :]
    g, st_g = _finish32(g.astype(f), st_e)
    out = dict(e=np.where(st_e == 1, e, f(0)).astype(f), st_e=st_e, g=g, st_g=st_g, eg=np.where(st_g == 1, e, f(0)).astype(f))
    if xrows is not None:
        with np.errstate(all="ignore"):
            y3 = y2 * y
            zt = _tangent32(rec, _f32(xrows))
            pos = y > 0
            k2 = np.where(pos, np.where(y >= eps, f(-1) / y3, f(-1) / ((eps * eps) * y)), f(0)).astype(f)
            q = np.where(pos, k2 * _dot(ut, zt), f(0)).astype(f)
            h = (scale[:, None] * w)[:, :, None] * (k1[:, None] * zt + q[:, None] * ut)[:, None, :]
            st = np.where(idle, 0, np.where(y3 <= f(FLT_MAX), 1, 2)).astype(np.int32)
        out["h"], out["st_h"] = _finish32(h.astype(f), st)
    return out


def gather32(terms, vert, nv):
    """per vertex the float32 sum of its (pair, corner) terms [n, 4, 3] front to back in list order (ref64_terms.gather); vert [n, 4], -1
    for a corner that is not in the mesh"""
    return rt.gather(nv, [rt.incidence(vert, nv) + (_f32(terms).reshape(-1, 3),)], np.float32)
