"""Float64 restatement and float32 replay of the mesh's internal energy (include/zensim_rocm/elastic_device.hpp,
zpc_amd/csrc/mesh_elastic.hip), numpy only: the rest records of triangles and hinges, the hinge list in the order the library builds it,
StVK membrane and quadratic bending energy with gradient and Hessian-vector product (exact and positive semi-definite), the gather in run
order, the float64 energy total in the order of the reduction kernels, and per-element bounds on the float32 result.

Every function works in the dtype of its input: float64 is the reference, float32 replays the device chain operation by operation (the
translation unit is built without FP contraction; sums of three products are formed left to right).  Only the float32 run applies the
overflow rule (a result beyond the float range: the element contributes exactly zero, status 2).

The bounds.  u = 2^-24; all are ABSOLUTE: E = (F^T F - I) / 2 cancels near rest, so the error scales with u |F|^2 mu and not with the strain.
Vector quantities are bounded in norm.  Inputs (float32 coordinates) are exact; a difference of two of them carries one rounding.

Triangle record.  e1, e2: 1 rounding each.  a = |e1|: 3 u relative.  t1 = e1 / a: 5 u.  b = e2 . t1: 8 u |e2| absolute.  p = e2 - b t1:
16 u |e2| per component, 28 u |e2| in norm, so c = |p| carries 31 u kappa relative, kappa = |e2| / c >= 1 (the aspect of the triangle).
a c: 35 u kappa.  B00 = 1 / a: 4 u.  B11 = 1 / c: 32 u kappa.  B01 = -b / (a c): 8 u kappa / a + 36 u kappa |B01|.  A = a c / 2: 36 u kappa.
Stated with K_REC = 40: every entry of B is off by at most dB = K_REC u kappa |B|_F, A by K_REC u kappa A.

Membrane evaluation, D = [x1 - x0, x2 - x0], f = |D|_F |B|_F >= |F|_F, g = (f^2 + 1) / 2 >= |E_ij|, sm = 2 mu + 2 lam, Smax = sm g >= |S_ij|:
    F = D B           eF  = (2 K_REC kappa + 4) u f                   (dB on both entries of a column, 3 roundings of the column, 1 of D)
    C = F^T F         2 f eF + eF^2 + 3 u f^2 per entry
    E                 dE  = f eF + eF^2 + 2 u (f^2 + 1);   dtr = 2 dE + 2 u g
    S                 dS  = 2 mu dE + lam dtr + 4 u sm g
    energy            be  = A (8 mu g dE + 2 lam g dtr + 4 mu dE^2 + lam dtr^2) + (K_REC kappa + 8) u V,  V = A (4 mu + 2 lam) g^2
    P = F S           Pmax = 2 Smax f;  dP = 2 (dS f + Smax eF + dS eF) + 3 u Pmax
    corners           t1 = A (P0 B00 + P1 B01), t2 = A P1 B11: bt = A |B| (2 dP + Pmax (4 K_REC kappa + 8) u); t0 = -(t1 + t2) adds both and
                      one rounding: every corner is held to  bg = 2 bt + 4 u A |B| Pmax.
Product with z, fz = |[z1 - z0, z2 - z0]|_F |B|_F, eFz = (2 K_REC kappa + 4) u fz:
    dE_z = sym(F^T dF)   ddE = f eFz + fz eF + eF eFz + 4 u f fz;  dtrz = 2 ddE + 2 u f fz;  Szmax = sm f fz;  ddS = 2 mu ddE + lam dtrz + 4 u Szmax
    T = S or S+          the projection onto the positive semi-definite matrices is 1-Lipschitz in the Frobenius norm (2 dS from the
                         entries of S) and its closed form is continuous across its three branches; evaluated in float32 it adds at most
                         10 roundings on quantities up to 2 r <= 4 Smax divided by 2 r:  dT = 2 dS + 32 u Smax, |T_ij| <= 2 Smax
    dP = dF T + F dS     Pzmax = 4 Smax fz + 2 Szmax f;  dPz = 2 (dT fz + 2 Smax eFz + dT eFz) + 2 (ddS f + Szmax eF + ddS eF) + 4 u Pzmax
    corners              as for the gradient: bh = 2 A |B| (2 dPz + Pzmax (4 K_REC kappa + 8) u) + 4 u A |B| Pzmax.

Hinge record.  A cotangent c = (e . a) / |e x a|: the dot product 5 u |e| |a| absolute, the cross product 8 u |e| |a| in norm, its length
11 u chi relative, chi = the largest |e| |a| / |e x a| = 1 / sin of the four angles; dc <= u chi (5 + 12 |c|).  K_i = sums of two: 2 dc + 2 u
cmax.  q = sqrt(3 / (A0 + A1)): 10 u chi relative.  k_i = q K_i: dk = K_HINGE u chi q (1 + cmax), K_HINGE = 48, cmax the largest |c|.
Bending evaluation, w = sum_i k_i x_i:
    w          dw = sum_i (dk + 4 u |k_i|) |x_i|        (absolute in the COORDINATES: the sum cancels, the weights summing to zero)
    energy     kb (|w| dw + dw^2 / 2) + 4 u kb (|w| + dw)^2
    term i     kb (dk (|w| + dw) + |k_i| dw) + 3 u kb |k_i| (|w| + dw)
and the product is the same chain at z.

Vertex.  The gather adds n terms front to back: the bounds of the terms, plus n u (sum of |term| + bound).
"""
import numpy as np

import ref64_proximity as rp
from ref64_mesh import U, _cross, _dot
from ref64_terms import incidence, gather, total      # the gather and the total, in the device's order

K_REC, K_HINGE = 40.0, 48.0
FLT_MAX = float(np.finfo(np.float32).max)
MU, LAM, KB = 1.3, 0.7, 2e-3
SCALES = (1e-3, 1e-1, 1.0)          # displacement scales in units of the mean edge length
# median over the vertices of `sheets` of bound / |force| at the middle displacement scale, gradient of membrane + bending, measured by
# tests/test_elastic_cpu.py on the CPU (the float64 force and the bounds above); asserted at twice this value there and on the device
SHEETS_MEDIAN_BOUND_OVER_G = 8.114e-3
IDLE, ACTIVE, OVERFLOW, DEGENERATE = 0, 1, 2, 3


def _norm(x):
    return np.sqrt(_dot(x, x))


def _finite(x):
    return np.abs(x) <= np.finfo(x.dtype).max      # (False for NaN)


# ------------------------------------------------------------------------------------------------ rest records
def tri_rest(X0, X1, X2):
    """(record [n, 4] = (B00, B01, B11, A), status [n]) in the dtype of X0; a degenerate triangle has a zero record and status 3"""
    X0 = np.asarray(X0)
    dt = X0.dtype.type
    with np.errstate(all="ignore"):
        e1, e2 = X1 - X0, X2 - X0
        a = np.sqrt(_dot(e1, e1))
        ok = (a > 0) & _finite(a)
        t1 = e1 / a[:, None]
        b = _dot(e2, t1)
        p = e2 - b[:, None] * t1
        c = np.sqrt(_dot(p, p))
        ok &= (c > 0) & _finite(c)
        ac = a * c
        ok &= ac > 0
        rec = np.stack([dt(1) / a, -b / ac, dt(1) / c, dt(0.5) * ac], axis=1)
        ok &= _finite(rec).all(axis=1) & (rec[:, 3] > 0)
    return np.where(ok[:, None], rec, dt(0)).astype(X0.dtype), np.where(ok, ACTIVE, DEGENERATE).astype(np.int32)


def hinge_rest(X0, X1, X2, X3, details=False):
    """(record [n, 4] = k, status [n]) in the dtype of X0; details: also (q, cmax, chi) for the bounds"""
    X0 = np.asarray(X0)
    dt = X0.dtype.type
    with np.errstate(all="ignore"):
        e, a2, a3, b2, b3 = X1 - X0, X2 - X0, X3 - X0, X1 - X2, X1 - X3
        n0, n1 = _cross(e, a2), _cross(e, a3)
        s0, s1 = np.sqrt(_dot(n0, n0)), np.sqrt(_dot(n1, n1))
        ok = (s0 > 0) & _finite(s0) & (s1 > 0) & _finite(s1)
        c01, c02, c03, c04 = _dot(e, a2) / s0, _dot(e, a3) / s1, _dot(e, b2) / s0, _dot(e, b3) / s1
        q = np.sqrt(dt(3) / (dt(0.5) * s0 + dt(0.5) * s1))
        k = np.stack([q * (c03 + c04), q * (c01 + c02), q * (-c01 - c03), q * (-c02 - c04)], axis=1)
        ok &= _finite(k).all(axis=1)
        rec = np.where(ok[:, None], k, dt(0)).astype(X0.dtype)
        st = np.where(ok, ACTIVE, DEGENERATE).astype(np.int32)
        if not details:
            return rec, st
        le = _norm(e)
        chi = np.max([le * _norm(a2) / s0, le * _norm(a3) / s1, le * _norm(b2) / s0, le * _norm(b3) / s1], axis=0)
        cmax = np.max(np.abs([c01, c02, c03, c04]), axis=0)
    return rec, st, q, cmax, chi


def hinges(tris):
    """(hinges [nh, 4] int64, non-manifold edges): every unique edge of ref64_proximity.edges with exactly two incident triangles, in that
    order; a row is the edge's (v0 < v1), then the opposite vertex of the incident triangle with the smaller index, then the other's"""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    inc = {}
    for ti, tri in enumerate(t.tolist()):
        for k in range(3):
            u, v = tri[k], tri[(k + 1) % 3]
            if u != v:
                inc.setdefault((min(u, v), max(u, v)), []).append(tri[(k + 2) % 3])
    out, bad = [], 0
    for e in map(tuple, rp.edges(t).tolist()):
        o = inc[e]
        if len(o) == 2:
            out.append((e[0], e[1], o[0], o[1]))
        bad += len(o) > 2
    return np.array(out, np.int64).reshape(-1, 4), bad


# ------------------------------------------------------------------------------------------------ evaluation
def _columns(rec, y):
    d1, d2 = y[:, 1] - y[:, 0], y[:, 2] - y[:, 0]
    return rec[:, 0, None] * d1, rec[:, 1, None] * d1 + rec[:, 2, None] * d2


def _corners(rec, P0, P1):
    A = rec[:, 3, None]
    t1 = A * (P0 * rec[:, 0, None] + P1 * rec[:, 1, None])
    t2 = A * (P1 * rec[:, 2, None])
    return np.stack([-(t1 + t2), t1, t2], axis=1)


def _settle(dtype, idle, values, finite):
    """the overflow rule of the float32 chain (float64: idle elements zeroed, nothing else): returns the status and the values"""
    if dtype == np.float32:
        ok = ~idle & finite
        st = np.where(idle, IDLE, np.where(ok, ACTIVE, OVERFLOW)).astype(np.int32)
    else:
        ok, st = ~idle, np.where(idle, IDLE, ACTIVE).astype(np.int32)
    return st, [np.where(ok.reshape((-1,) + (1,) * (v.ndim - 1)), v, v.dtype.type(0)).astype(v.dtype) for v in values]


def tri_eval(rec, x, mu, lam, z=None, psd=False):
    """membrane energy e [n], gradient g [n, 3, 3] and (z [n, 3, 3] given) product h [n, 3, 3] of triangles with records rec at the corner
    positions x [n, 3, 3], in the dtype of rec, with statuses st_e, st_g, st_h; also F0, F1, S (00, 01, 11) and T (the projected stress)"""
    rec = np.asarray(rec)
    dt, dtype = rec.dtype.type, rec.dtype
    x = np.asarray(x, dtype)
    mu, lam = dt(mu), dt(lam)
    idle = rec[:, 3] == 0
    with np.errstate(all="ignore"):
        F0, F1 = _columns(rec, x)
        E00, E11, E01 = dt(0.5) * (_dot(F0, F0) - dt(1)), dt(0.5) * (_dot(F1, F1) - dt(1)), dt(0.5) * _dot(F0, F1)
        tr = E00 + E11
        mu2, lt = dt(2) * mu, lam * tr
        S00, S11, S01 = mu2 * E00 + lt, mu2 * E11 + lt, mu2 * E01
        e = rec[:, 3] * (mu * ((E00 * E00 + E11 * E11) + dt(2) * (E01 * E01)) + (dt(0.5) * lam) * (tr * tr))
        g = _corners(rec, S00[:, None] * F0 + S01[:, None] * F1, S01[:, None] * F0 + S11[:, None] * F1)
        r = dict(F0=F0, F1=F1, S=np.stack([S00, S01, S11], axis=1), E=np.stack([E00, E01, E11], axis=1))
        r["st_e"], (r["e"],) = _settle(dtype, idle, [e], _finite(e))
        r["st_g"], (r["eg"], r["g"]) = _settle(dtype, idle, [e, g], _finite(e) & _finite(g).all(axis=(1, 2)))
        if z is not None:
            z = np.asarray(z, dtype)
            T00, T01, T11 = S00, S01, S11
            if psd:
                m, hd = dt(0.5) * (S00 + S11), dt(0.5) * (S00 - S11)
                rr = np.sqrt(hd * hd + S01 * S01)
                keep, none = m - rr >= 0, m + rr <= 0
                q, lo = (m + rr) / (dt(2) * rr), m - rr
                pick = lambda full, mixed: np.where(keep, full, np.where(none, dt(0), mixed))
                T00, T11, T01 = pick(S00, q * (S00 - lo)), pick(S11, q * (S11 - lo)), pick(S01, q * S01)
            dF0, dF1 = _columns(rec, z)
            dE00, dE11 = _dot(F0, dF0), _dot(F1, dF1)
            dE01 = dt(0.5) * (_dot(F0, dF1) + _dot(F1, dF0))
            lt = lam * (dE00 + dE11)
            dS00, dS11, dS01 = mu2 * dE00 + lt, mu2 * dE11 + lt, mu2 * dE01
            P0 = (T00[:, None] * dF0 + T01[:, None] * dF1) + (dS00[:, None] * F0 + dS01[:, None] * F1)
            P1 = (T01[:, None] * dF0 + T11[:, None] * dF1) + (dS01[:, None] * F0 + dS11[:, None] * F1)
            h = _corners(rec, P0, P1)
            r["st_h"], (r["h"],) = _settle(dtype, idle, [h], _finite(h).all(axis=(1, 2)))
            r["T"] = np.stack([T00, T01, T11], axis=1)
    return r


def _hinge_w(k, y):
    return ((k[:, 0, None] * y[:, 0] + k[:, 1, None] * y[:, 1]) + k[:, 2, None] * y[:, 2]) + k[:, 3, None] * y[:, 3]


def hinge_eval(rec, x, kb, z=None):
    """bending energy e [n], gradient g [n, 4, 3] and (z given) product h [n, 4, 3] of hinges with records rec at x [n, 4, 3]"""
    rec = np.asarray(rec)
    dt, dtype = rec.dtype.type, rec.dtype
    x = np.asarray(x, dtype)
    kb = dt(kb)
    kk = (kb[:, None] if np.ndim(kb) else kb) * rec      # (kb may be one number per hinge)
    idle = (rec == 0).all(axis=1)
    with np.errstate(all="ignore"):
        w = _hinge_w(rec, x)
        e = (dt(0.5) * kb) * _dot(w, w)
        g = kk[:, :, None] * w[:, None, :]
        r = dict(w=w)
        r["st_e"], (r["e"],) = _settle(dtype, idle, [e], _finite(e))
        r["st_g"], (r["eg"], r["g"]) = _settle(dtype, idle, [e, g], _finite(e) & _finite(g).all(axis=(1, 2)))
        if z is not None:
            wz = _hinge_w(rec, np.asarray(z, dtype))
            h = kk[:, :, None] * wz[:, None, :]
            r["st_h"], (r["h"],) = _settle(dtype, idle, [h], _finite(h).all(axis=(1, 2)))
            r["wz"] = wz
    return r


# ------------------------------------------------------------------------------------------------ bounds (float64 in, see the module docstring)
def tri_bounds(X, x, rec, mu, lam, z=None):
    """(be [n], bg [n], bh [n] or None): bounds on the energy and on every corner term of the float32 gradient and product of triangles
    with float64 records rec at rest corners X and corners x [n, 3, 3]; zero for an idle triangle"""
    X, x = np.asarray(X, np.float64), np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        c = 1.0 / rec[:, 2]
        kap = np.maximum(_norm(X[:, 2] - X[:, 0]) / c, 1.0)
        nB, A = np.sqrt(rec[:, 0] ** 2 + rec[:, 1] ** 2 + rec[:, 2] ** 2), rec[:, 3]
        frob = lambda y: np.sqrt(_dot(y[:, 1] - y[:, 0], y[:, 1] - y[:, 0]) + _dot(y[:, 2] - y[:, 0], y[:, 2] - y[:, 0]))
        f = frob(x) * nB
        kf = (2 * K_REC * kap + 4) * U
        eF, g, sm = kf * f, (f * f + 1) / 2, 2 * mu + 2 * lam
        Smax = sm * g
        dE = f * eF + eF * eF + 2 * U * (f * f + 1)
        dtr = 2 * dE + 2 * U * g
        dS = 2 * mu * dE + lam * dtr + 4 * U * sm * g
        V = A * (4 * mu + 2 * lam) * g * g
        be = A * (8 * mu * g * dE + 2 * lam * g * dtr + 4 * mu * dE * dE + lam * dtr * dtr) + (K_REC * kap + 8) * U * V
        Pmax = 2 * Smax * f
        dP = 2 * (dS * f + Smax * eF + dS * eF) + 3 * U * Pmax
        kc = (4 * K_REC * kap + 8) * U
        bg = 2 * A * nB * (2 * dP + Pmax * kc) + 4 * U * A * nB * Pmax
        bh = None
        if z is not None:
            fz = frob(np.asarray(z, np.float64)) * nB
            eFz = kf * fz
            ddE = f * eFz + fz * eF + eF * eFz + 4 * U * f * fz
            dtrz = 2 * ddE + 2 * U * f * fz
            Szmax = sm * f * fz
            ddS = 2 * mu * ddE + lam * dtrz + 4 * U * Szmax
            dT = 2 * dS + 32 * U * Smax
            Pzmax = 4 * Smax * fz + 2 * Szmax * f
            dPz = 2 * (dT * fz + 2 * Smax * eFz + dT * eFz) + 2 * (ddS * f + Szmax * eF + ddS * eF) + 4 * U * Pzmax
            bh = 2 * A * nB * (2 * dPz + Pzmax * kc) + 4 * U * A * nB * Pzmax
    idle = rec[:, 3] == 0
    zero = lambda b: None if b is None else np.where(idle, 0.0, b)
    return zero(be), zero(bg), zero(bh)


def hinge_bounds(X, x, kb, z=None):
    """(be [n], bg [n, 4], bh [n, 4] or None) for hinges with rest corners X and corners x [n, 4, 3] (float64 in)"""
    X, x = np.asarray(X, np.float64), np.asarray(x, np.float64)
    rec, st, q, cmax, chi = hinge_rest(X[:, 0], X[:, 1], X[:, 2], X[:, 3], details=True)
    with np.errstate(all="ignore"):
        dk = K_HINGE * U * chi * q * (1 + cmax)
        ak = np.abs(rec)

        def at(y):
            w = _norm(_hinge_w(rec, y))
            dw = ((dk[:, None] + 4 * U * ak) * _norm(y)).sum(axis=1)
            top = w + dw
            return w, dw, kb * (dk[:, None] * top[:, None] + ak * dw[:, None]) + 3 * U * kb * ak * top[:, None]
        w, dw, bg = at(x)
        be = kb * (w * dw + dw * dw / 2) + 4 * U * kb * (w + dw) ** 2
        bh = None if z is None else at(np.asarray(z, np.float64))[2]
    idle = st != ACTIVE
    zero = lambda b: None if b is None else np.where(idle.reshape((-1,) + (1,) * (b.ndim - 1)), 0.0, b)
    return zero(be), zero(bg), zero(bh)


# ------------------------------------------------------------------------------------------------ a scene
def displaced(verts, tris, seed, scale):
    """rest + a seeded displacement of `scale` mean edge lengths, rounded to float32"""
    v = np.asarray(verts, np.float32)
    e = rp.edges(tris)
    mean = float(np.linalg.norm(v[e[:, 1]].astype(np.float64) - v[e[:, 0]], axis=1).mean()) if len(e) else 1.0
    return (v.astype(np.float64) + scale * mean * np.random.default_rng(3000 + seed).standard_normal(v.shape)).astype(np.float32)


def compressed(verts, s=0.5):
    """uniform scaling by s about the centroid, rounded to float32"""
    v = np.asarray(verts, np.float64)
    c = v.mean(axis=0) if len(v) else 0.0
    return (c + s * (v - c)).astype(np.float32)


class Rest:
    """the rest shape of a mesh in dtype: tri_record, hinges, hinge_record, vertex_area and the counts, with both incidences"""

    def __init__(self, rest_verts, tris, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.X = np.asarray(np.asarray(rest_verts, np.float32), dtype)
        self.tris = np.asarray(tris, np.int64).reshape(-1, 3)
        self.nv = len(self.X)
        self.hinges, self.nonmanifold = hinges(self.tris)
        t, h = self.tris, self.hinges
        self.tri_record, st = tri_rest(self.X[t[:, 0]], self.X[t[:, 1]], self.X[t[:, 2]])
        self.hinge_record, sh = hinge_rest(self.X[h[:, 0]], self.X[h[:, 1]], self.X[h[:, 2]], self.X[h[:, 3]])
        self.counts = (int((st == DEGENERATE).sum()), int((sh == DEGENERATE).sum()), self.nonmanifold)
        self.tri_inc, self.hinge_inc = incidence(t, self.nv), incidence(h, self.nv)
        third = self.tri_record[:, 3] / self.dtype.type(3)
        self.vertex_area = gather(self.nv, [(self.tri_inc[0], self.tri_inc[1], np.repeat(third, 3))], self.dtype)

    def assemble(self, tri_terms, hinge_terms):
        """the per-vertex sums of [nt, 3, 3] and [nh, 4, 3] terms: the triangle run, then the hinge run, in run order"""
        return gather(self.nv, [(self.tri_inc[0], self.tri_inc[1], tri_terms.reshape(-1, 3)),
                                (self.hinge_inc[0], self.hinge_inc[1], hinge_terms.reshape(-1, 3))], self.dtype)

    def evaluate(self, verts, mu, lam, kb, z=None, psd=False, tri_record=None, hinge_record=None):
        """(triangle dict, hinge dict, grad, hx or None) at verts; the records may be given (the device's own)"""
        x = np.asarray(np.asarray(verts, np.float32), self.dtype)
        zz = None if z is None else np.asarray(np.asarray(z, np.float32), self.dtype)
        t, h = self.tris, self.hinges
        T = tri_eval(self.tri_record if tri_record is None else np.asarray(tri_record, self.dtype), x[t], mu, lam, None if zz is None else zz[t], psd)
        H = hinge_eval(self.hinge_record if hinge_record is None else np.asarray(hinge_record, self.dtype), x[h], kb, None if zz is None else zz[h])
        if not (mu > 0 or lam > 0):
            T = {k: (np.zeros_like(v) if k in ("e", "eg", "g", "h") else v) for k, v in T.items()}
        if not kb > 0:
            H = {k: (np.zeros_like(v) if k in ("e", "eg", "g", "h") else v) for k, v in H.items()}
        grad = self.assemble(T["g"], H["g"])
        return T, H, grad, (None if zz is None else self.assemble(T["h"], H["h"]))

    def vertex_bounds(self, verts, mu, lam, kb, T, H, z=None):
        """(bound on grad [nv], bound on hx [nv] or None) for the float32 result against the float64 dicts T, H of evaluate"""
        x = np.asarray(np.asarray(verts, np.float32), np.float64)
        zz = None if z is None else np.asarray(np.asarray(z, np.float32), np.float64)
        t, h = self.tris, self.hinges
        X = self.X.astype(np.float64)
        _, bg, bh = tri_bounds(X[t], x[t], self.tri_record, mu, lam, None if zz is None else zz[t])
        _, hg, hh = hinge_bounds(X[h], x[h], kb, None if zz is None else zz[h])
        if not (mu > 0 or lam > 0):
            bg, bh = np.zeros_like(bg), (None if bh is None else np.zeros_like(bh))
        if not kb > 0:
            hg, hh = np.zeros_like(hg), (None if hh is None else np.zeros_like(hh))
        out = []
        for tb, hb, key in ((bg, hg, "g"), (bh, hh, "h")):
            if tb is None:
                out.append(None)
                continue
            tb3, size_t, size_h = np.repeat(tb, 3), _norm(T[key]).reshape(-1), _norm(H[key]).reshape(-1)
            runs = lambda a, b: gather(self.nv, [(self.tri_inc[0], self.tri_inc[1], a), (self.hinge_inc[0], self.hinge_inc[1], b)], np.float64)
            b, size = runs(tb3, hb.reshape(-1)), runs(size_t + tb3, size_h + hb.reshape(-1))
            n = np.diff(self.tri_inc[0]) + np.diff(self.hinge_inc[0])
            out.append(b + n * U * size)
        return out
