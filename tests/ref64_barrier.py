"""Float64 restatement of the mesh barrier potential (include/zensim_rocm/barrier_device.hpp, zpc_amd/csrc/mesh_barrier.hip), numpy plus
torch float64 on the CPU: energy and gradient of the IPC barrier over PT and EE pair lists, the gradient a second way through
torch.autograd and a min-over-candidates distance, a float32 replay of the device chain, and the bounds on the float32 result.

Reference.  d2, barycentrics / (s, t) come from ref64_mesh.tri_closest / ref64_proximity.ee_closest in float64 on the float32 coordinates
the device gets; dHat2 is the float32 product dHat * dHat the device forms (an input of the chain, like the coordinates).
    b(d2) = -kappa t^2 log(d2 / dHat2), b' = kappa (-2 t log(d2 / dHat2) - t^2 / d2), t = d2 - dHat2, for d2 < dHat2
    gradient on corner k = 2 m b' w_k r + m' b grad_k c;  r = P - Q, w = (1, -bary) or (1 - s, s, -(1 - t), -t)
    m, m' the mollifier of c = |u x v|^2 against eps = 1e-2 restLen2_i restLen2_j (EE with rest lengths; otherwise m = 1, m' = 0)

The bounds, with u = 2^-24.  Everything starts from the existing per-pair distance bound delta = K u (S + M) of ref64_proximity.py
(K_PT / K_EE; S = d + the edge lengths, M = the largest coordinate): the float32 distance lies in [d - delta, d + delta].
  b, b'    b is convex and decreasing on (0, dHat2) and both b and b' are monotone there, so their deviation over the interval is taken at
           its ends: Db = max |b(d +- delta) - b(d)|, Db' likewise (to first order |b'| 2 d delta and |b''| 2 d delta; the end values
           are used because delta / d reaches 0.1 at d / dHat = 1e-3).  d - delta <= 0: the bound is infinite, the pair stays in.
           Roundings of the new chain, magnitudes taken at the near end of the interval where they are largest:
             t = d2 - dHat2 1, ratio 1 (an absolute u in the logarithm), logf 2 ulp, t^2 1 (+ 2 from t), the products and the division 1
             each:  b: u kappa t^2 + 7 u |b|, stated 8 u (kappa t^2 + |b|);  b' = kappa (X - Y), X = -2 t log, Y = t^2 / d2:
             2 u |t| + 4 u |X| + 4 u |Y| + the subtraction and kappa 2 u (|X| + |Y|), stated 8 u kappa (|t| + |X| + |Y|).
  w, r     The float32 chain returns the closest points of ONE of the candidates of tri_closest / ee_closest (face, three segments; the
           common perpendicular, four point-segment pairs): one whose float64 distance is within 2 delta of the minimum and whose
           parameters are inside their range up to their own rounding.  All such candidates are enumerated in float64; Dw_k and Dr are
           the largest deviation of a candidate's weights and of its r from the reference's, plus the first-order rounding of the
           candidate's parameters: a segment parameter t = (d . e) / |e|^2 carries ~4 roundings relative to |d| |e|: 4 u S / |e|, stated
           8; barycentrics of the face and (s, t) of the common perpendicular are triple products over |n|^2, ~10-13 roundings relative
           to |n| L S: stated 16 u S L / |n| and 16 u S / (|e| sin(angle)) (the count of ref64_proximity.py); r = P - Q adds the
           rounding of the points, 8 u (S + M), and the parameter errors times the edge lengths.  Dw_k <= 1 and Dr <= 2 d + delta
           whatever happens.  Near a Voronoi boundary the neighbouring candidate qualifies and its closest point is next to the
           reference's, so the bound stays small; between exactly parallel edges the tied candidates have different (s, t): Dw_k
           reaches its cap and the term m b' grad(d2) enters by its size m |b'| 2 d sum |w| -- nothing is special-cased or left out.
  c, m     n = u x v: two products and a difference per component on terms up to |u| |v|, after the roundings of u and v: Dn = 10 u |u| |v|;
           Dc = 2 |n| Dn + Dn^2 + 3 u c.  eps: the rest lengths are float32 sums of squares (4 u each), two products and the constant
           1e-2f: stated 16 u relative.  x = c / eps: Dx = Dc / eps + 17 u x.  m = (2 - x) x is 2-Lipschitz, m' = (2 / eps)(1 - x):
           Dm = 2 Dx + 3 u m,  Dm' = (2 / eps)(Dx + 20 u).  grad c = 2 v x n, 2 n x u: D = 2 |e| (Dn + 4 u |n|).
  corner   T1 = A w_k r, A = 2 m b':  DA = 2 (Dm (|b'| + Db') + m Db') + 2 u |A|;
           DT1 = DA |w_k| d + (|A| + DA)(Dw_k (d + Dr) + |w_k| Dr) + 4 u |T1|
           T2 = B grad_k c, B = m' b:  DB = Dm' (|b| + Db) + |m'| Db + 2 u |B|;  DT2 = DB (|grad c| + D grad c) + |B| D grad c + u |T2|
           and u (|T1| + |T2|) for their sum.  Energy: Dm (|b| + Db) + m Db + u |m b|.
  vertex   the sum of the bounds of its incident (pair, corner) terms plus n_inc u sum |term| for the float32 accumulation.
"""
import numpy as np

import ref64_mesh as rm
import ref64_proximity as rp
from ref64_mesh import U, _dot, _cross, _segment

FLT_MAX, FLT_MIN = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)
K_SEG, K_TRIPLE, K_POINT = 8.0, 16.0, 8.0
# the vacuity guard of tests/test_barrier_gpu.py: the median over the contact vertices of scene `sheets` (dhat of the scene, kappa = 1,
# mollified, rest = the scene) of bound / |g|, measured by tests/test_barrier_cpu.py with the float64 reference alone: 1.715e-03
SHEETS_MEDIAN_BOUND_OVER_G = 1.715e-3


def dhat2_f32(dhat):
    return float(np.float32(dhat) * np.float32(dhat))


def barrier(d2, dhat2, kappa):
    """(b, b') in float64; 0 at and beyond dhat2; b = +inf, b' = 0 at d2 = 0"""
    d2 = np.asarray(d2, np.float64)
    act = (d2 < dhat2) & (d2 > 0)
    x = np.where(act, d2, 0.5 * dhat2)
    t, lg = x - dhat2, np.log(x / dhat2)
    b = np.where(act, -kappa * t * t * lg, np.where(d2 < dhat2, np.inf, 0.0))
    bp = np.where(act, kappa * (-2 * t * lg - t * t / x), 0.0)
    return b, bp


def mollifier(c, eps):
    """(m, m') in float64; eps = 0: (1, 0)"""
    c, eps = np.asarray(c, np.float64), np.broadcast_to(np.asarray(eps, np.float64), np.shape(c))
    on = (eps > 0) & (c < eps)
    e1 = np.where(eps > 0, eps, 1.0)
    x = c / e1
    return np.where(on, (2 - x) * x, 1.0), np.where(on, (2 / e1) * (1 - x), 0.0)


def _norm(x):
    return np.sqrt(_dot(x, x))


def _ee_vertices(v, e, pairs):
    return v[e[pairs[:, 0], 0]], v[e[pairs[:, 0], 1]], v[e[pairs[:, 1], 0]], v[e[pairs[:, 1], 1]]


def rest_len2(verts, edge_list):
    v, e = rp._v64(verts), np.asarray(edge_list, np.int64).reshape(-1, 2)
    d = v[e[:, 1]] - v[e[:, 0]]
    return _dot(d, d)


# ------------------------------------------------------------------------------------------------ the scalar stage of the bound
def _scalar_bounds(d, delta, dhat2, kappa):
    """(b, b', Db, Db') at distance d known to +- delta"""
    lo, hi = np.maximum(d - delta, 0.0), d + delta
    b0, p0 = barrier(d * d, dhat2, kappa)
    bl, pl = barrier(lo * lo, dhat2, kappa)
    bh, ph = barrier(hi * hi, dhat2, kappa)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        db = np.maximum(np.abs(bl - b0), np.abs(bh - b0))
        dp = np.maximum(np.abs(pl - p0), np.abs(ph - p0))
        act = (lo * lo < dhat2) & (lo > 0)
        x = np.where(act, lo * lo, 0.5 * dhat2)
        t, lg = x - dhat2, np.log(x / dhat2)
        rb = np.where(act, 8 * U * (kappa * t * t + np.abs(bl)), 0.0)
        rp_ = np.where(act, 8 * U * kappa * (np.abs(t) + np.abs(2 * t * lg) + t * t / x), 0.0)
    bad = ~(lo > 0) & (d * d < dhat2)     # the interval reaches zero distance
    db = np.where(bad | ~np.isfinite(db), np.inf, db + rb)
    dp = np.where(bad | ~np.isfinite(dp), np.inf, dp + rp_)
    return b0, p0, db, dp


def _spread(d, delta, dc, elig, wc, rc, dwc, drc, wref, rref):
    """Dw [n, 4], Dr [n] over the candidates c (axis 1) that are eligible and within 2 delta of the minimum"""
    ok = elig & (dc <= (d + 2 * delta)[:, None])
    dw = np.where(ok[:, :, None], np.abs(wc - wref[:, None, :]) + dwc, 0.0).max(axis=1)
    dr = np.where(ok, _norm(rc - rref[:, None, :]) + drc, 0.0).max(axis=1)
    return np.minimum(dw, 1.0), np.minimum(dr, 2 * d + delta)


# ------------------------------------------------------------------------------------------------ PT
def pt_pairs64(verts, tris, pairs, dhat2, kappa, M=None):
    """dict(e, g [n, 4, 3], be, bg [n, 4], zero, vert [n, 4]) of the (vertex, triangle) pairs"""
    v, t = rp._v64(verts), np.asarray(tris, np.int64).reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    vert = np.concatenate([pairs[:, :1], t[pairs[:, 1]]], axis=1).reshape(n, 4)
    p, a, b, c = (v[vert[:, k]] for k in range(4))
    d2, cp, bary, _ = rm.tri_closest(p, a, b, c)
    d = np.sqrt(d2)
    M = rp.coord_max(verts) if M is None else M
    ab, ac, bc = b - a, c - a, c - b
    lens = np.stack([_norm(ab), _norm(bc), _norm(ac)], axis=1)
    Lmax = lens.max(axis=1) if n else np.zeros(0)
    S = d + Lmax
    delta = rp.K_PT * U * (S + M) + 1e-37
    r = p - cp
    w = np.concatenate([np.ones((n, 1)), -bary], axis=1)
    b0, p0, db, dp = _scalar_bounds(d, delta, dhat2, kappa)
    g = (2 * p0)[:, None, None] * w[:, :, None] * r[:, None, :]
    # candidates: face, ab, bc, ca
    nrm = _cross(ab, ac)
    nn = _dot(nrm, nrm)
    nn1 = np.where(nn > 0, nn, 1.0)
    pa, pb = p - a, p - b
    b1, b2 = _dot(nrm, _cross(pa, ac)) / nn1, _dot(nrm, _cross(ab, pa)) / nn1
    fb = np.stack([1 - b1 - b2, b1, b2], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        eb = np.where(nn > 0, K_TRIPLE * U * S * Lmax / np.sqrt(nn1), np.inf)
    wc, rc, dc, elig, dwc, drc = np.zeros((n, 4, 4)), np.zeros((n, 4, 3)), np.zeros((n, 4)), np.zeros((n, 4), bool), np.zeros((n, 4, 4)), np.zeros((n, 4))
    wc[:, 0] = np.concatenate([np.ones((n, 1)), -fb], axis=1)
    rc[:, 0] = p - (a + b1[:, None] * ab + b2[:, None] * ac)
    dc[:, 0] = _norm(rc[:, 0])
    elig[:, 0] = (nn > 0) & (fb >= -eb[:, None]).all(axis=1)
    dwc[:, 0, 1:] = np.minimum(eb, 1.0)[:, None]
    drc[:, 0] = 2 * np.minimum(eb, 1.0) * Lmax + K_POINT * U * (S + M)
    for k, (s0, s1, i0, i1) in enumerate(((a, b, 1, 2), (b, c, 2, 3), (c, a, 3, 1))):
        dd, tt = _segment(p, s0, s1)
        wc[:, k + 1, 0] = 1
        wc[:, k + 1, i0], wc[:, k + 1, i1] = -(1 - tt), -tt
        rc[:, k + 1] = p - (s0 + tt[:, None] * (s1 - s0))
        dc[:, k + 1] = np.sqrt(dd)
        elig[:, k + 1] = True
        le = _norm(s1 - s0)
        with np.errstate(divide="ignore", invalid="ignore"):
            et = np.where(le > 0, np.minimum(K_SEG * U * S / np.where(le > 0, le, 1.0), 1.0), 0.0)
        dwc[:, k + 1, i0] = dwc[:, k + 1, i1] = et
        drc[:, k + 1] = et * le + K_POINT * U * (S + M)
    dw, dr = _spread(d, delta, dc, elig, wc, rc, dwc, drc, w, r)
    A, dA = 2 * np.abs(p0), 2 * dp
    aw = np.abs(w)
    with np.errstate(invalid="ignore"):
        bg = dA[:, None] * aw * d[:, None] + (A + dA)[:, None] * (dw * (d + dr)[:, None] + aw * dr[:, None]) + 4 * U * A[:, None] * aw * d[:, None]
    bg = np.where(np.isfinite(bg), bg, np.inf)
    zero = (d2 == 0) & (d2 < dhat2)
    g[zero] = 0.0
    return dict(e=b0, g=g, be=db, bg=bg, zero=zero, vert=vert, d=d, delta=delta)


# ------------------------------------------------------------------------------------------------ EE
def ee_pairs64(verts, edge_list, pairs, dhat2, kappa, rest2=None, M=None):
    """the same of the (edge, edge) pairs; rest2 [ne]: squared rest lengths (None: unmollified)"""
    v, e = rp._v64(verts), np.asarray(edge_list, np.int64).reshape(-1, 2)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    vert = np.concatenate([e[pairs[:, 0]], e[pairs[:, 1]]], axis=1).reshape(n, 4)
    a0, a1, b0_, b1_ = (v[vert[:, k]] for k in range(4))
    d2, s, t, _, _ = rp.ee_closest(a0, a1, b0_, b1_)
    d = np.sqrt(d2)
    M = rp.coord_max(verts) if M is None else M
    u, vv, w0 = a1 - a0, b1_ - b0_, a0 - b0_
    lu, lv = _norm(u), _norm(vv)
    S = d + lu + lv
    delta = rp.K_EE * U * (S + M) + 1e-37
    r = (a0 + s[:, None] * u) - (b0_ + t[:, None] * vv)
    w = np.stack([1 - s, s, -(1 - t), -t], axis=1)
    bb, p0, db, dp = _scalar_bounds(d, delta, dhat2, kappa)
    nrm = _cross(u, vv)
    c = _dot(nrm, nrm)
    ln = np.sqrt(c)
    eps = np.zeros(n) if rest2 is None else 1e-2 * np.asarray(rest2, np.float64)[pairs[:, 0]] * np.asarray(rest2, np.float64)[pairs[:, 1]]
    eps = np.where(eps >= FLT_MIN, eps, 0.0)
    m, mp = mollifier(c, eps)
    gcu, gcv = 2 * _cross(vv, nrm), 2 * _cross(nrm, u)
    gc = np.stack([-gcu, gcu, -gcv, gcv], axis=1)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(bb)
        bsafe = np.where(fin, bb, 0.0)
        T1 = (2 * m * p0)[:, None, None] * w[:, :, None] * r[:, None, :]
        T2 = (mp * bsafe)[:, None, None] * gc
    g = T1 + T2
    # candidates: the common perpendicular, then a0, a1 against b and b0, b1 against a
    nn1 = np.where(c > 0, c, 1.0)
    si, ti = _dot(_cross(vv, w0), nrm) / nn1, _dot(_cross(u, w0), nrm) / nn1
    with np.errstate(divide="ignore", invalid="ignore"):
        sin = np.where(c > 0, ln / np.where(lu * lv > 0, lu * lv, 1.0), 0.0)
        es = np.where(sin > 0, K_TRIPLE * U * S / np.where(sin > 0, lu * sin, 1.0), np.inf)
        et = np.where(sin > 0, K_TRIPLE * U * S / np.where(sin > 0, lv * sin, 1.0), np.inf)
    wc, rc, dc, elig, dwc, drc = np.zeros((n, 5, 4)), np.zeros((n, 5, 3)), np.zeros((n, 5)), np.zeros((n, 5), bool), np.zeros((n, 5, 4)), np.zeros((n, 5))
    sc, tc = np.clip(si, 0, 1), np.clip(ti, 0, 1)
    wc[:, 0] = np.stack([1 - sc, sc, -(1 - tc), -tc], axis=1)
    rc[:, 0] = (w0 + sc[:, None] * u) - tc[:, None] * vv
    dc[:, 0] = _norm(rc[:, 0])
    elig[:, 0] = (c > 0) & (si > -es) & (si < 1 + es) & (ti > -et) & (ti < 1 + et)
    dwc[:, 0, :2], dwc[:, 0, 2:] = np.minimum(es, 1.0)[:, None], np.minimum(et, 1.0)[:, None]
    drc[:, 0] = np.minimum(es, 1.0) * lu + np.minimum(et, 1.0) * lv + K_POINT * U * (S + M)
    for k in range(4):
        if k < 2:
            dd, pp = _segment(a0 if k == 0 else a1, b0_, b1_)
            cs, ct, le, cols = np.full(n, float(k)), pp, lv, (2, 3)
        else:
            dd, pp = _segment(b0_ if k == 2 else b1_, a0, a1)
            cs, ct, le, cols = pp, np.full(n, float(k - 2)), lu, (0, 1)
        wc[:, k + 1] = np.stack([1 - cs, cs, -(1 - ct), -ct], axis=1)
        rc[:, k + 1] = (w0 + cs[:, None] * u) - ct[:, None] * vv
        dc[:, k + 1] = np.sqrt(dd)
        elig[:, k + 1] = True
        ep = np.where(le > 0, np.minimum(K_SEG * U * S / np.where(le > 0, le, 1.0), 1.0), 0.0)
        dwc[:, k + 1, cols[0]] = dwc[:, k + 1, cols[1]] = ep
        drc[:, k + 1] = ep * le + K_POINT * U * (S + M)
    dw, dr = _spread(d, delta, dc, elig, wc, rc, dwc, drc, w, r)
    # c, m, m', grad c
    dn = 10 * U * lu * lv
    dcc = 2 * ln * dn + dn * dn + 3 * U * c
    e1 = np.where(eps > 0, eps, 1.0)
    dx = np.where(eps > 0, dcc / e1 + 17 * U * c / e1, 0.0)
    dm = np.where(eps > 0, np.minimum(2 * dx + 3 * U * m, 1.0), 0.0)
    dmp = np.where(eps > 0, (2 / e1) * (dx + 20 * U), 0.0)
    # (beyond the threshold by more than the error of x the float32 chain is on the constant branch as well)
    far = (eps > 0) & (c / e1 - dx >= 1)
    dm, dmp = np.where(far, 0.0, dm), np.where(far, 0.0, dmp)
    lgc = np.stack([lv * ln, lv * ln, lu * ln, lu * ln], axis=1) * 2
    dgc = np.stack([lv, lv, lu, lu], axis=1) * 2 * (dn + 4 * U * ln)[:, None]
    ap0, ab = np.abs(p0), np.abs(bsafe)
    aw = np.abs(w)
    with np.errstate(invalid="ignore", over="ignore"):
        A = 2 * m * ap0
        dA = 2 * (dm * (ap0 + dp) + m * dp) + 2 * U * A
        bT1 = dA[:, None] * aw * d[:, None] + (A + dA)[:, None] * (dw * (d + dr)[:, None] + aw * dr[:, None]) + 4 * U * A[:, None] * aw * d[:, None]
        B = np.abs(mp) * ab
        dB = dmp * (ab + db) + np.abs(mp) * db + 2 * U * B
        bT2 = dB[:, None] * (lgc + dgc) + B[:, None] * dgc + U * B[:, None] * lgc
        bg = bT1 + bT2 + U * (_norm(T1) + _norm(T2))
        be = dm * (ab + db) + m * db + U * m * ab
    # exactly zero factors stay exactly zero on the device as well: m = 0 with n = 0 (see the header), so 0 * inf does not arise
    bg = np.where(np.isnan(bg), np.inf, bg)
    be = np.where(np.isnan(be), np.inf, be)
    zero = (d2 == 0) & (d2 < dhat2)
    g[zero] = 0.0
    energy = np.where(zero, np.inf, m * bsafe)
    return dict(e=energy, g=g, be=be, bg=bg, zero=zero, vert=vert, d=d, delta=delta, m=m)


# ------------------------------------------------------------------------------------------------ a scene
class Reference:
    """energy, gradient and bounds of a constraint set at positions verts: pt_e, ee_e, energy, grad [nv, 3], pt_be, ee_be, energy_bound,
    vbound [nv], ninc [nv], zero = (pt, ee).  rest2: squared rest lengths per edge, None = unmollified."""

    def __init__(self, verts, tris, pt_pairs, ee_pairs, dhat, kappa, rest2=None, edge_list=None):
        v = rp._v64(verts)
        nv = len(v)
        self.dhat2 = dhat2_f32(dhat)
        e = rp.edges(tris) if edge_list is None else edge_list
        M = rp.coord_max(verts)
        self.pt = pt_pairs64(verts, tris, np.zeros((0, 2), int) if pt_pairs is None else pt_pairs, self.dhat2, kappa, M)
        self.ee = ee_pairs64(verts, e, np.zeros((0, 2), int) if ee_pairs is None else ee_pairs, self.dhat2, kappa, rest2, M)
        self.pt_e, self.ee_e, self.pt_be, self.ee_be = self.pt["e"], self.ee["e"], self.pt["be"], self.ee["be"]
        self.energy = float(self.pt_e.sum() + self.ee_e.sum())
        self.energy_bound = float(self.pt_be.sum() + self.ee_be.sum())
        self.zero = (int(self.pt["zero"].sum()), int(self.ee["zero"].sum()))
        self.grad, self.vbound, self.ninc, mag = np.zeros((nv, 3)), np.zeros(nv), np.zeros(nv, np.int64), np.zeros(nv)
        for q in (self.pt, self.ee):
            idx = q["vert"].ravel()
            np.add.at(self.grad, idx, q["g"].reshape(-1, 3))
            np.add.at(self.vbound, idx, q["bg"].ravel())
            np.add.at(self.ninc, idx, 1)
            np.add.at(mag, idx, (_norm(q["g"]) + np.where(np.isfinite(q["bg"]), q["bg"], 0.0)).ravel())
        self.vbound = self.vbound + self.ninc * U * mag + 1e-37


# ------------------------------------------------------------------------------------------------ autograd
def autograd_energy(verts, tris, edge_list, pt_pairs, ee_pairs, dhat2, kappa, rest2=None):
    """(energy, gradient [nv, 3]) with torch.autograd in float64 through a min-over-candidates distance: PT the plane distance where the
    projection falls inside, and the three point-segment distances; EE the line-line distance where the common perpendicular meets both
    segments, and the four point-segment distances"""
    import torch
    x = torch.tensor(rp._v64(verts), dtype=torch.float64, requires_grad=True)
    t = torch.as_tensor(np.asarray(tris, np.int64).reshape(-1, 3))
    e = torch.as_tensor(np.asarray(edge_list, np.int64).reshape(-1, 2))
    dot = lambda a, b: (a * b).sum(-1)
    big = torch.tensor(float("inf"), dtype=torch.float64)

    def seg(p, s0, s1):
        ed, d = s1 - s0, p - s0
        ee = dot(ed, ed)
        tt = torch.where(ee > 0, dot(d, ed) / torch.where(ee > 0, ee, torch.ones_like(ee)), torch.zeros_like(ee)).clamp(0, 1)
        r = d - tt[:, None] * ed
        return dot(r, r)

    def bar(d2):
        act = (d2 < dhat2) & (d2 > 0)
        y = torch.where(act, d2, torch.full_like(d2, 0.5 * dhat2))
        return torch.where(act, -kappa * (y - dhat2) ** 2 * torch.log(y / dhat2), torch.zeros_like(y))
    total = x.sum() * 0
    if pt_pairs is not None and len(pt_pairs):
        pp = torch.as_tensor(np.asarray(pt_pairs, np.int64))
        p, a, b, c = x[pp[:, 0]], x[t[pp[:, 1], 0]], x[t[pp[:, 1], 1]], x[t[pp[:, 1], 2]]
        n = torch.linalg.cross(b - a, c - a)
        nn = dot(n, n)
        wa, wb, wc = dot(n, torch.linalg.cross(c - b, p - b)), dot(n, torch.linalg.cross(p - a, c - a)), dot(n, torch.linalg.cross(b - a, p - a))
        inside = (nn > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)
        plane = dot(n, p - a) ** 2 / torch.where(nn > 0, nn, torch.ones_like(nn))
        d2 = torch.where(inside, plane, big)
        for s0, s1 in ((a, b), (b, c), (c, a)):
            d2 = torch.minimum(d2, seg(p, s0, s1))
        total = total + bar(d2).sum()
    if ee_pairs is not None and len(ee_pairs):
        pe = torch.as_tensor(np.asarray(ee_pairs, np.int64))
        a0, a1, b0, b1 = x[e[pe[:, 0], 0]], x[e[pe[:, 0], 1]], x[e[pe[:, 1], 0]], x[e[pe[:, 1], 1]]
        u, v, w = a1 - a0, b1 - b0, a0 - b0
        n = torch.linalg.cross(u, v)
        nn = dot(n, n)
        nn1 = torch.where(nn > 0, nn, torch.ones_like(nn))
        s, tt = dot(torch.linalg.cross(v, w), n) / nn1, dot(torch.linalg.cross(u, w), n) / nn1
        inside = (nn > 0) & (s > 0) & (s < 1) & (tt > 0) & (tt < 1)
        d2 = torch.where(inside, dot(w, n) ** 2 / nn1, big)
        for p, s0, s1 in ((a0, b0, b1), (a1, b0, b1), (b0, a0, a1), (b1, a0, a1)):
            d2 = torch.minimum(d2, seg(p, s0, s1))
        m = torch.ones_like(d2)
        if rest2 is not None:
            r2 = torch.as_tensor(np.asarray(rest2, np.float64))
            eps = 1e-2 * r2[pe[:, 0]] * r2[pe[:, 1]]
            on = (eps >= FLT_MIN) & (nn < eps)
            xx = nn / torch.where(eps > 0, eps, torch.ones_like(eps))
            m = torch.where(on, (2 - xx) * xx, m)
        total = total + (m * bar(d2)).sum()
    total.backward()
    return float(total.detach()), x.grad.numpy().copy()


# ------------------------------------------------------------------------------------------------ the float32 replay of the device chain
def _f32(x):
    return np.asarray(x, np.float32)


def barrier32(d2, dhat2, kappa, log=np.log):
    """barrier_eval in numpy float32: (b, b', status 0 inactive / 1 active / 2 zero)"""
    f = np.float32
    d2, dhat2, kappa = _f32(d2), f(dhat2), f(kappa)
    with np.errstate(all="ignore"):
        act = d2 < dhat2
        ratio = d2 / dhat2
        pos = ratio > 0
        safe = np.where(act & pos, ratio, f(0.5))
        t, lg = d2 - dhat2, _f32(log(safe))
        t2 = t * t
        e = (-kappa * t2) * lg
        de = kappa * ((f(-2) * t) * lg - t2 / np.where(act & pos, d2, f(1)))
        ok = np.abs(de) <= f(FLT_MAX)
    status = np.where(~act, 0, np.where(pos & ok, 1, 2)).astype(np.int32)
    return (np.where(status == 1, e, np.where(status == 2, f(np.inf), f(0))).astype(f), np.where(status == 1, de, f(0)).astype(f), status)


def pt32(p, a, b, c, dhat2, kappa, log=np.log):
    """barrier_pt<true>: (energy [n], g [n, 4, 3], status) in float32"""
    f = np.float32
    p, a, b, c = (_f32(x) for x in (p, a, b, c))
    d2, cp, bary, _ = rm.tri_closest(p, a, b, c, degenerate=rm.DEGENERATE32)
    e, bp, st = barrier32(d2, dhat2, kappa, log)
    A = f(2) * bp
    w = np.stack([np.ones_like(A), -bary[:, 0], -bary[:, 1], -bary[:, 2]], axis=1).astype(f)
    with np.errstate(all="ignore"):
        g = (A[:, None] * w)[:, :, None] * (p - cp)[:, None, :]
    g = np.where((st == 1)[:, None, None], g, f(0)).astype(f)
    return e, g, st


def ee_eps32(ri, rj):
    return (np.float32(1e-2) * _f32(ri)) * _f32(rj)


def ee32(a0, a1, b0, b1, dhat2, kappa, eps, log=np.log):
    """barrier_ee<true>: (energy [n], g [n, 4, 3], status) in float32; eps [n] float32, 0 = unmollified"""
    f = np.float32
    a0, a1, b0, b1 = (_f32(x) for x in (a0, a1, b0, b1))
    eps = np.broadcast_to(_f32(eps), a0.shape[:1])
    d2, s, t, _, _ = rp.ee_closest(a0, a1, b0, b1, parallel=rp.PARALLEL32)
    s, t = s.astype(f), t.astype(f)
    bb, bp, st = barrier32(d2, dhat2, kappa, log)
    u, v = a1 - a0, b1 - b0
    n = _cross(u, v)
    c = _dot(n, n)
    with np.errstate(all="ignore"):
        on = (eps >= f(FLT_MIN)) & (c < eps)
        e1 = np.where(on, eps, f(1))
        x = c / e1
        m = np.where(on, (f(2) - x) * x, f(1)).astype(f)
        mp = np.where(on, (f(2) / e1) * (f(1) - x), f(0)).astype(f)
        act = st == 1
        bsafe = np.where(act, bb, f(0))
        energy = np.where(act, m * bsafe, bb).astype(f)
        w = np.stack([f(1) - s, s, -(f(1) - t), -t], axis=1).astype(f)
        A, B = m * (f(2) * bp), mp * bsafe
        dcu, dcv = f(2) * _cross(v, n), f(2) * _cross(n, u)
        diff = (a0 + s[:, None] * u) - (b0 + t[:, None] * v)
        gc = np.stack([-dcu, dcu, -dcv, dcv], axis=1)
        g = B[:, None, None] * gc + (A[:, None] * w)[:, :, None] * diff[:, None, :]
    g = np.where(act[:, None, None], g, f(0)).astype(f)
    return energy, g, st
