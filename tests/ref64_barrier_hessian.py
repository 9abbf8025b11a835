"""Float64 restatement of the mesh barrier Hessian-vector product (barrier_pt_hvp / barrier_ee_hvp of include/zensim_rocm/barrier_device.hpp,
zs_rocm_mesh_barrier_hessian_product), on top of ref64_barrier / ref64_proximity / ref64_mesh: the closed forms per pair and per eligible
candidate, a second float64 route through torch.autograd's double backward, the float32 replay of the device chain, and the bounds.

Closed form (the header has the derivation).  One function, hvp_core, in the dtype of its input: float64 is the reference, float32 replays
the device operation by operation.  A candidate is (w [4], r = P - Q, up to two free parameters with rows dw/dlambda and vectors
dr/dlambda); hess d2 . v = 2 w_k (W v) - F^T A^-1 F v, H_b v = b'' (g . v) g + b' hess d2 . v, and the mollified edge-edge product on top.

Candidates.  The Hessian of d2 jumps across Voronoi boundaries although the gradient does not (a vertex region has 2 W^T W, the edge next to
it subtracts F^T A^-1 F), so the float32 chain may legitimately land on a neighbouring feature.  The candidates are those of
ref64_barrier: PT the face and the three segments, EE the common perpendicular and the four point-segment pairs (and, between nearly
parallel edges, the two-parameter form at the reference's closest points: ee_candidates64 says why); a segment candidate
comes in two states, parameter free (interior) and clamped (an end point), the state float64 finds always, the other one where the raw
parameter is within its own rounding of 0 or 1.  Eligible as in ref64_barrier._spread: inside the range up to the parameter's rounding
and within 2 delta of the minimum distance.  `own` marks the reference's candidate.  A pair's error is the smallest over its eligible
candidates of the largest corner error over that candidate's bound: nothing is left out.

Bounds, u = 2^-24, per candidate, reusing delta, Db', Dw, Dr, Dm, Dm', Dn of ref64_barrier (Dw, Dr here are the candidate's own parameter
and point roundings dwc / drc; the spread to other candidates is what the candidate rule is for).  |x_k| is taken per corner.
  b''      monotone on (0, dHat2) (b''' < 0), so Db'' = the larger deviation at the ends of the interval, plus the roundings of
           kappa ((-2 lg - 4 q) + q^2), q = t / d2: stated 8 u kappa (1 + |2 lg| + |4 q| + q^2) at the near end.  The interval of a candidate
           at distance d_c is [d_c - D, d_c + D], D = d_c - d + delta: the float32 distance of the candidate the chain realised is the
           float32 minimum, within delta of the reference's d <= d_c.  An interval that reaches zero: infinite.
  W x      sum_k w_k x_k: DWx = sum_k Dw_k |x_k| + 4 u sum_k |w_k| |x_k|
  g_k      2 w_k r: Dg_k = 2 (Dw_k (d + Dr) + |w_k| Dr) + 2 u |g_k|
  g . x    2 r . W x: Dgx = 2 (Dr (|Wx| + DWx) + d DWx) + 4 u 2 d sum_k |w_k| |x_k|
  T_a      b'' (g . x) g_k: the product rule  Db'' |gx| |g_k| + (|b''| + Db'') (Dgx (|g_k| + Dg_k) + |gx| Dg_k) + 3 u |T_a|
  free     r_j is a difference of two vertices: Dr_j = 2 u |r_j|;  D_j = sum_k dw_jk x_k: DD_j = 2 u sum_k |dw_jk| |x_k|
           F_j = 2 (r_j . Wx + r . D_j): DF_j = 2 (Dr_j (|Wx| + DWx) + |r_j| DWx + Dr (|D_j| + DD_j) + d DD_j) + 5 u 2 (|r_j| |Wx| + d |D_j|)
           one free parameter: y = F / A, A = 2 |r_j|^2: Dy = DF / A + 8 u |y|
           two: y_1 = (A_22 F_1 - A_12 F_2) / det, det = 4 |r_1 x r_2|^2.  The deviation of A^-1: the cross product carries
           Dn = 10 u |r_1| |r_2| (the count of ref64_barrier), so det has the relative error e = 2 Dn / |n| + 4 u = 20 u / sin + 4 u, and
           the numerator's terms are divided by det = 4 |r_1|^2 |r_2|^2 sin^2: the relative error of y grows as 1 / sin^2 of the angle
           between the edges.  Dy_1 = (A_22 DF_1 + 2 |r_1| |r_2| DF_2 + 8 u (A_22 |F_1| + 2 |r_1| |r_2| |F_2|)) / det / (1 - e) + |y_1| e / (1 - e);
           e >= 1 (sin below 1.2e-6): infinite.  A candidate whose free system is degenerate in float64 (det = 0) has the clamped
           form and an infinite bound.
           F^T y on corner k = 2 sum_j y_j (w_k r_j + dw_jk r):
           Dft_k = 2 sum_j (Dy_j (|w_k| |r_j| + |dw_jk| d) + (|y_j| + Dy_j)(Dw_k |r_j| + |w_k| Dr_j + |dw_jk| Dr)) + 6 u 2 sum_j |y_j| (|w_k| |r_j| + |dw_jk| d)
  T_b      exact: b' (2 w_k Wx - ft_k), with D(2 w_k Wx) = 2 (Dw_k (|Wx| + DWx) + |w_k| DWx) + 4 u |w_k| |Wx|:
           Db' |2 w_k Wx - ft_k| + (|b'| + Db')(D(2 w_k Wx) + Dft_k) + 2 u |b'| (2 |w_k| |Wx| + |ft_k|);  psd: the same with |b'| ft_k alone.
           H_b x on the corner: DT_a + DT_b + u (|T_a| + |T_b|).
  EE       m H_b x:  Dm (|H_b x| + DH_b) + m DH_b + u m |H_b x|.  c1 = m' b': Dc1 = Dm' (|b'| + Db') + |m'| Db' + u |c1|; c3 = b m' likewise.
           du = x_1 - x_0: Ddu = u |du|.  grad c . x = dcu . du + dcv . dv, |dcu| <= G_u = 2 |v| |n|, D dcu = 2 |v| (Dn + 4 u |n|) (as
           ref64_barrier): Dgcx = D dcu |du| + D dcv |dv| + G_u Ddu + G_v Ddv + 4 u (G_u |du| + G_v |dv|).
           m'' = -2 / eps^2 where c < eps: relative 35 u (eps carries 16 u, twice, and three operations) -- and the whole of 2 / eps^2
           where c / eps is within its error Dx of 1, because m'' jumps there (m and m' are continuous; the float32 chain may be on
           either side).  dn = du x v + u x dv, |dn| <= N = |du| |v| + |u| |dv|, D dn = 10 u N.  hess c . x on the u side
           2 (dv x n + v x dn): D = 2 (|dv| Dn + |v| 10 u N) + 12 u (|dv| |n| + |v| N), the v side with u and v exchanged; psd keeps
           2 v x dn: D = 20 u |v| N + 8 u |v| N.  Each product by the product rule as above, 4 u of the sum of the magnitudes for the sums.
  vertex   the reference is the sum of the pairs' own candidates; a pair's bound against its own candidate is the largest over its
           eligible candidates of |Hx_candidate - Hx_own| + that candidate's bound (the spread, as ref64_barrier._spread does for w and
           r); the vertex bound is the sum over its incidences plus n_inc u sum |term| for the float32 accumulation.
"""
import numpy as np

import ref64_barrier as rb
import ref64_mesh as rm
import ref64_proximity as rp
from ref64_mesh import U, _dot, _cross, _segment

FLT_MAX, FLT_MIN = rb.FLT_MAX, rb.FLT_MIN
# the vacuity guard of tests/test_barrier_hessian_gpu.py: the median over the contact vertices of scene `sheets` (dhat of the scene,
# kappa = 1, mollified, exact product, direction = direction(nv, 1)) of bound / |Hx|, measured by tests/test_barrier_hessian_cpu.py with
# the float64 reference alone: 1.162e-02.  Above the 1e-2 the gradient's bound stays under: the vertex bound carries the spread over the
# candidates, and a pair next to a Voronoi boundary has two values of hess d2 that differ by a term of the size of the Hessian itself
SHEETS_MEDIAN_BOUND_OVER_HX = 1.162e-2


def direction(nv, seed):
    """a seeded unit-scale direction [nv, 3], rounded to float32 (the numbers the device gets)"""
    return np.random.default_rng(1000 + seed).standard_normal((nv, 3)).astype(np.float32)


def _norm(x):
    return np.sqrt(_dot(x, x))


def barrier3(d2, dhat2, kappa):
    """(b, b', b'') in float64; 0 at and beyond dhat2 and at d2 = 0 (b = +inf there)"""
    d2 = np.asarray(d2, np.float64)
    b, bp = rb.barrier(d2, dhat2, kappa)
    act = (d2 < dhat2) & (d2 > 0)
    x = np.where(act, d2, 0.5 * dhat2)
    q = (x - dhat2) / x
    return b, bp, np.where(act, kappa * (-2 * np.log(x / dhat2) - 4 * q + q * q), 0.0)


# ------------------------------------------------------------------------------------------------ the closed form, any dtype
def _lin(c, x):
    return c[:, 0, None] * x[:, 0] + c[:, 1, None] * x[:, 1] + c[:, 2, None] * x[:, 2] + c[:, 3, None] * x[:, 3]


def hvp_core(w, r, f1, f2, d1, d2, r1, r2, x, bp, bpp, psd):
    """barrier_hvp_core: (h [n, 4, 3], g . x [n], parts) in the dtype of r; parts: what the bounds need"""
    dt = r.dtype.type
    two = dt(2)
    with np.errstate(all="ignore"):
        Wx, D1, D2 = _lin(w, x), _lin(d1, x), _lin(d2, x)
        gx = two * _dot(r, Wx)
        F1, F2 = two * (_dot(r1, Wx) + _dot(r, D1)), two * (_dot(r2, Wx) + _dot(r, D2))
        A11, A22, A12 = two * _dot(r1, r1), two * _dot(r2, r2), two * _dot(r1, r2)
        c12 = _cross(r1, r2)
        det = dt(4) * _dot(c12, c12)
        both = f1 & f2
        ok2, ok1a, ok1b = both & (det > 0), f1 & ~f2 & (A11 > 0), f2 & ~f1 & (A22 > 0)
        ds, a1s, a2s = np.where(ok2, det, dt(1)), np.where(ok1a, A11, dt(1)), np.where(ok1b, A22, dt(1))
        y1 = np.where(ok2, (A22 * F1 - A12 * F2) / ds, np.where(ok1a, F1 / a1s, dt(0))).astype(r.dtype)
        y2 = np.where(ok2, (A11 * F2 - A12 * F1) / ds, np.where(ok1b, F2 / a2s, dt(0))).astype(r.dtype)
        cg, abp = bpp * gx, np.abs(bp)
        w3, r3 = w[:, :, None], r[:, None, :]
        gk = (two * w3) * r3
        ft = two * (y1[:, None, None] * (w3 * r1[:, None, :] + d1[:, :, None] * r3) + y2[:, None, None] * (w3 * r2[:, None, :] + d2[:, :, None] * r3))
        Ta = cg[:, None, None] * gk
        if psd:
            Tb = abp[:, None, None] * ft
        else:
            Tb = bp[:, None, None] * ((two * w3) * Wx[:, None, :] - ft)
        h = Ta + Tb
    return h, gx, dict(Wx=Wx, D1=D1, D2=D2, F1=F1, F2=F2, y1=y1, y2=y2, ft=ft, Ta=Ta, Tb=Tb, gk=gk, det=det, degenerate=both & ~ok2)


def pt_slots(feature, a, b, c):
    """(f1, f2, d1 [n, 4], d2, r1 [n, 3], r2) of a triangle feature: slot 1 = bary1 of the face or the parameter of the edge, slot 2 = bary2"""
    dt = a.dtype.type
    face, eab, ebc, eca = feature == rm.FACE, feature == rm.EDGE_AB, feature == rm.EDGE_BC, feature == rm.EDGE_CA
    z, o = np.zeros(len(a), a.dtype), np.ones(len(a), a.dtype)
    fa = face | eab
    d1 = np.stack([z, np.where(fa, o, np.where(eca, -o, z)), np.where(fa, -o, np.where(ebc, o, z)), np.where(ebc, -o, np.where(eca, o, z))], axis=1)
    d2 = np.stack([z, np.where(face, o, z), z, np.where(face, -o, z)], axis=1)
    r1 = np.where(fa[:, None], a - b, np.where(ebc[:, None], b - c, np.where(eca[:, None], c - a, dt(0)))).astype(a.dtype)
    r2 = np.where(face[:, None], a - c, dt(0)).astype(a.dtype)
    return fa | ebc | eca, face, d1, d2, r1, r2


def ee_slots(fs, ft, u, b0, b1):
    z, o = np.zeros(len(u), u.dtype), np.ones(len(u), u.dtype)
    d1 = np.stack([np.where(fs, -o, z), np.where(fs, o, z), z, z], axis=1)
    d2 = np.stack([z, z, np.where(ft, o, z), np.where(ft, -o, z)], axis=1)
    return d1, d2, np.where(fs[:, None], u, u.dtype.type(0)).astype(u.dtype), np.where(ft[:, None], b0 - b1, u.dtype.type(0)).astype(u.dtype)


def ee_mollified(hb, gx, w, r, u, v, x, bb, bp, eps, psd):
    """the mollifier on top of H_b x, as barrier_ee_hvp: (h, parts); eps [n], 0 = unmollified; any dtype"""
    dt = r.dtype.type
    two = dt(2)
    with np.errstate(all="ignore"):
        n = _cross(u, v)
        c = _dot(n, n)
        on = (eps >= dt(FLT_MIN)) & (c < eps)
        e1 = np.where(on, eps, dt(1))
        xx = c / e1
        m = np.where(on, (two - xx) * xx, dt(1)).astype(r.dtype)
        mp = np.where(on, (two / e1) * (dt(1) - xx), dt(0)).astype(r.dtype)
        du, dv = x[:, 1] - x[:, 0], x[:, 3] - x[:, 2]
        dn = _cross(du, v) + _cross(u, dv)
        vdn, dnu = _cross(v, dn), _cross(dn, u)
        c3 = bb * mp
        s = lambda a: a[:, None]
        if psd:
            tu, tv = s(c3) * (two * vdn), s(c3) * (two * dnu)
            mh = m[:, None, None] * hb
            h = np.stack([mh[:, 0] - tu, mh[:, 1] + tu, mh[:, 2] - tv, mh[:, 3] + tv], axis=1)
            return h.astype(r.dtype), dict(m=m, mp=mp, c=c, on=on)
        vn, nu, dvn, ndu = _cross(v, n), _cross(n, u), _cross(dv, n), _cross(n, du)
        dcu, dcv = two * vn, two * nu
        gcx = _dot(dcu, du) + _dot(dcv, dv)
        c1 = mp * bp
        c2 = np.where(on, bb * ((dt(-2) * (gcx / e1)) / e1), dt(0)).astype(r.dtype)
        c1c, c1g = c1 * gcx, c1 * gx
        tu = s(c1g) * dcu + (s(c2) * dcu + s(c3) * (two * (dvn + vdn)))
        tv = s(c1g) * dcv + (s(c2) * dcv + s(c3) * (two * (dnu + ndu)))
        P = m[:, None, None] * hb + c1c[:, None, None] * ((two * w[:, :, None]) * r[:, None, :])
        h = np.stack([P[:, 0] - tu, P[:, 1] + tu, P[:, 2] - tv, P[:, 3] + tv], axis=1)
    return h.astype(r.dtype), dict(m=m, mp=mp, c=c, on=on, gcx=gcx)


# ------------------------------------------------------------------------------------------------ the float32 replay of the device chain
def barrier32_3(d2, dhat2, kappa, log=np.log):
    """barrier_eval2 in numpy float32: (b, b', b'', status)"""
    f = np.float32
    b, bp, st = rb.barrier32(d2, dhat2, kappa, log)
    d2, dhat2, kappa = rb._f32(d2), f(dhat2), f(kappa)
    with np.errstate(all="ignore"):
        act = st == 1
        t, lg = d2 - dhat2, rb._f32(log(np.where(act, d2 / dhat2, f(0.5))))
        q = t / np.where(act, d2, f(1))
        dd = kappa * ((f(-2) * lg - f(4) * q) + q * q)
        bad = act & ~(np.abs(dd) <= f(FLT_MAX))
    st = np.where(bad, 2, st).astype(np.int32)
    return (np.where(bad, f(np.inf), b).astype(f), np.where(bad, f(0), bp).astype(f), np.where(st == 1, dd, f(0)).astype(f), st)


def _finish32(h, st):
    """barrier_hvp_finish and the zeros of the pairs that are not active"""
    with np.errstate(invalid="ignore"):
        ok = (np.abs(h) <= np.float32(FLT_MAX)).all(axis=(1, 2))
    st = np.where((st == 1) & ~ok, 2, st).astype(np.int32)
    return np.where((st == 1)[:, None, None], h, np.float32(0)).astype(np.float32), st


def pt_hvp32(p, a, b, c, x, dhat2, kappa, psd, log=np.log):
    """barrier_pt_hvp<psd>: (h [n, 4, 3], status) in float32"""
    p, a, b, c, x = (rb._f32(v) for v in (p, a, b, c, x))
    d2, cp, bary, feat = rm.tri_closest(p, a, b, c, degenerate=rm.DEGENERATE32)
    bb, bp, bpp, st = barrier32_3(d2, dhat2, kappa, log)
    f1, f2, d1, d2_, r1, r2 = pt_slots(feat, a, b, c)
    w = np.stack([np.ones_like(bp), -bary[:, 0], -bary[:, 1], -bary[:, 2]], axis=1).astype(np.float32)
    h, _, _ = hvp_core(w, (p - cp).astype(np.float32), f1, f2, d1, d2_, r1, r2, x, bp, bpp, psd)
    return _finish32(h, st)


def ee_hvp32(a0, a1, b0, b1, x, dhat2, kappa, eps, psd, log=np.log):
    """barrier_ee_hvp<psd>: (h [n, 4, 3], status) in float32; eps [n] float32, 0 = unmollified"""
    f = np.float32
    a0, a1, b0, b1, x = (rb._f32(v) for v in (a0, a1, b0, b1, x))
    eps = np.broadcast_to(rb._f32(eps), a0.shape[:1])
    d2, s, t, cat, _ = rp.ee_closest(a0, a1, b0, b1, parallel=rp.PARALLEL32)
    s, t = s.astype(f), t.astype(f)
    bb, bp, bpp, st = barrier32_3(d2, dhat2, kappa, log)
    fs, ft = cat // 3 == rp.INTERIOR, cat % 3 == rp.INTERIOR
    u, v = a1 - a0, b1 - b0
    d1, d2_, r1, r2 = ee_slots(fs, ft, u, b0, b1)
    w = np.stack([f(1) - s, s, -(f(1) - t), -t], axis=1).astype(f)
    r = ((a0 + s[:, None] * u) - (b0 + t[:, None] * v)).astype(f)
    hb, gx, _ = hvp_core(w, r, fs, ft, d1, d2_, r1, r2, x, bp, bpp, psd)
    bsafe = np.where(st == 1, bb, f(0))
    h, _ = ee_mollified(hb, gx, w, r, u, v, x, bsafe, bp, eps, psd)
    return _finish32(h, st)


# ------------------------------------------------------------------------------------------------ the scalar stage of the bound
def _scalar3(d, delta, dhat2, kappa):
    """(b, b', b'', Db, Db', Db'') at distance d known to +- delta"""
    b0, p0, db, dp = rb._scalar_bounds(d, delta, dhat2, kappa)
    lo, hi = np.maximum(d - delta, 0.0), d + delta
    q0, ql, qh = (barrier3(z * z, dhat2, kappa)[2] for z in (d, lo, hi))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dq = np.maximum(np.abs(ql - q0), np.abs(qh - q0))
        act = (lo * lo < dhat2) & (lo > 0)
        x = np.where(act, lo * lo, 0.5 * dhat2)
        qq, lg = (x - dhat2) / x, np.log(x / dhat2)
        rq = np.where(act, 8 * U * kappa * (1 + np.abs(2 * lg) + np.abs(4 * qq) + qq * qq), 0.0)
    bad = ~(lo > 0) & (d * d < dhat2)
    dq = np.where(bad | ~np.isfinite(dq), np.inf, dq + rq)
    return b0, p0, q0, db, dp, dq


def _core_bound(w, dw, r, dr, f1, f2, d1, d2, r1, r2, x, bp, dbp, bpp, dbpp, psd):
    """(h [n, 4, 3], bound [n, 4], g . x, Dgx, |g_k|, Dg_k) of one candidate in float64, by the rules of the docstring"""
    h, gx, P = hvp_core(w, r, f1, f2, d1, d2, r1, r2, x, bp, bpp, psd)
    with np.errstate(all="ignore"):
        ax, aw, d = _norm(x), np.abs(w), _norm(r)
        nWx = _norm(P["Wx"])
        mag = (aw * ax).sum(axis=1)
        DWx = (dw * ax).sum(axis=1) + 4 * U * mag
        ag = 2 * aw * d[:, None]
        Dg = 2 * (dw * (d + dr)[:, None] + aw * dr[:, None]) + 2 * U * ag
        agx = np.abs(gx)
        Dgx = 2 * (dr * (nWx + DWx) + d * DWx) + 8 * U * d * mag
        abpp, abp = np.abs(bpp), np.abs(bp)
        nTa, nTb = _norm(P["Ta"]), _norm(P["Tb"])
        DTa = dbpp[:, None] * agx[:, None] * ag + (abpp + dbpp)[:, None] * (Dgx[:, None] * (ag + Dg) + agx[:, None] * Dg) + 3 * U * nTa
        # the free system
        Dy, ay, l, dl, nD, DD, ad = [], [], [], [], [], [], []
        for rj, dj, Dj in ((r1, d1, P["D1"]), (r2, d2, P["D2"])):
            l.append(_norm(rj))
            dl.append(2 * U * l[-1])
            nD.append(_norm(Dj))
            ad.append(np.abs(dj))
            DD.append(2 * U * (ad[-1] * ax).sum(axis=1))
        DF = [2 * (dl[j] * (nWx + DWx) + l[j] * DWx + dr * (nD[j] + DD[j]) + d * DD[j]) + 10 * U * (l[j] * nWx + d * nD[j]) for j in range(2)]
        aF = [np.abs(P["F1"]), np.abs(P["F2"])]
        ay = [np.abs(P["y1"]), np.abs(P["y2"])]
        both = f1 & f2
        n12 = _norm(_cross(r1, r2))
        e = np.where(n12 > 0, 20 * U * l[0] * l[1] / np.where(n12 > 0, n12, 1.0) + 4 * U, np.inf)
        det = np.where(both & (n12 > 0), 4 * n12 * n12, 1.0)
        A = [2 * l[0] * l[0], 2 * l[1] * l[1]]
        for j in range(2):
            o = 1 - j
            two = (A[o] * DF[j] + 2 * l[0] * l[1] * DF[o] + 8 * U * (A[o] * aF[j] + 2 * l[0] * l[1] * aF[o])) / det / (1 - e) + ay[j] * e / (1 - e)
            two = np.where(e < 1, two, np.inf)
            one = DF[j] / np.where(A[j] > 0, A[j], 1.0) + 8 * U * ay[j]
            fj = f1 if j == 0 else f2
            Dy.append(np.where(both, two, np.where(fj, one, 0.0)))
        aft = _norm(P["ft"])
        Dft = np.zeros_like(aw)
        for j in range(2):
            lever = aw * l[j][:, None] + ad[j] * d[:, None]
            term = Dy[j][:, None] * lever + (ay[j] + Dy[j])[:, None] * (dw * l[j][:, None] + aw * dl[j][:, None] + ad[j] * dr[:, None])
            Dft = Dft + 2 * np.where((ay[j] + Dy[j] > 0)[:, None], term, 0.0) + 12 * U * ay[j][:, None] * lever
        if psd:
            DTb = dbp[:, None] * aft + (abp + dbp)[:, None] * Dft + 2 * U * abp[:, None] * aft
        else:
            D2w = 2 * (dw * (nWx + DWx)[:, None] + aw * DWx[:, None]) + 4 * U * aw * nWx[:, None]
            hd = _norm((2 * w)[:, :, None] * P["Wx"][:, None, :] - P["ft"])
            DTb = dbp[:, None] * hd + (abp + dbp)[:, None] * (D2w + Dft) + 2 * U * abp[:, None] * (2 * aw * nWx[:, None] + aft)
        bound = DTa + DTb + U * (nTa + nTb)
        bound = np.where(P["degenerate"][:, None] | np.isnan(bound), np.inf, bound)
    return h, bound, gx, Dgx, ag, Dg


# ------------------------------------------------------------------------------------------------ PT
def pt_candidates64(verts, tris, pairs, xdir, dhat2, kappa, psd, M=None):
    """dict(h [n, C, 4, 3], bound [n, C, 4], elig [n, C], own [n], vert [n, 4], zero [n]) of the (vertex, triangle) pairs for the
    direction xdir [nv, 3]; C = 7 candidates: the face, then (free, clamped) of the segments ab, bc, ca"""
    v, t = rp._v64(verts), np.asarray(tris, np.int64).reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    vert = np.concatenate([pairs[:, :1], t[pairs[:, 1]]], axis=1).reshape(n, 4)
    p, a, b, c = (v[vert[:, k]] for k in range(4))
    x = np.asarray(xdir, np.float64)[vert]
    d2ref, cpref, baryref, featref = rm.tri_closest(p, a, b, c)
    dref = np.sqrt(d2ref)
    M = rp.coord_max(verts) if M is None else M
    ab, ac, bc = b - a, c - a, c - b
    Lmax = np.stack([_norm(ab), _norm(bc), _norm(ac)], axis=1).max(axis=1) if n else np.zeros(0)
    S = dref + Lmax
    delta = rp.K_PT * U * (S + M) + 1e-37
    C = 7
    H, B, E, nfree, W = np.zeros((n, C, 4, 3)), np.zeros((n, C, 4)), np.zeros((n, C), bool), np.zeros((n, C), int), np.zeros((n, C, 4))
    dcand = np.zeros((n, C))

    def put(k, w, dw, r, dr, feat, elig):
        dc = _norm(r)
        _, bp, bpp, _, dbp, dbpp = _scalar3(dc, np.maximum(dc - dref, 0.0) + delta, dhat2, kappa)
        f1, f2, d1, d2, r1, r2 = pt_slots(feat, a, b, c)
        H[:, k], B[:, k] = _core_bound(w, dw, r, dr, f1, f2, d1, d2, r1, r2, x, bp, dbp, bpp, dbpp, psd)[:2]
        E[:, k], nfree[:, k], W[:, k], dcand[:, k] = elig, f1.astype(int) + f2.astype(int), w, dc
    # the face
    nrm = _cross(ab, ac)
    nn = _dot(nrm, nrm)
    nn1 = np.where(nn > 0, nn, 1.0)
    pa = p - a
    b1, b2 = _dot(nrm, _cross(pa, ac)) / nn1, _dot(nrm, _cross(ab, pa)) / nn1
    fb = np.stack([1 - b1 - b2, b1, b2], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        eb = np.where(nn > 0, rb.K_TRIPLE * U * S * Lmax / np.sqrt(nn1), np.inf)
    dw = np.zeros((n, 4))
    dw[:, 1:] = np.minimum(eb, 1.0)[:, None]
    put(0, np.concatenate([np.ones((n, 1)), -fb], axis=1), dw, p - (a + b1[:, None] * ab + b2[:, None] * ac),
        2 * np.minimum(eb, 1.0) * Lmax + rb.K_POINT * U * (S + M), np.full(n, rm.FACE), (nn > 0) & (fb >= -eb[:, None]).all(axis=1))
    # the segments: parameter free, parameter clamped
    for k, (s0, s1, i0, i1, fe, f0, f1_) in enumerate(((a, b, 1, 2, rm.EDGE_AB, rm.VERT_A, rm.VERT_B), (b, c, 2, 3, rm.EDGE_BC, rm.VERT_B, rm.VERT_C),
                                                       (c, a, 3, 1, rm.EDGE_CA, rm.VERT_C, rm.VERT_A))):
        ed = s1 - s0
        le = _norm(ed)
        le1 = np.where(le > 0, le, 1.0)
        raw = np.where(le > 0, _dot(p - s0, ed) / (le1 * le1), 0.0)
        et = np.where(le > 0, np.minimum(rb.K_SEG * U * S / le1, 1.0), 0.0)
        near = (np.abs(raw) <= et) | (np.abs(raw - 1) <= et)
        inside = (raw > 0) & (raw < 1)
        tt = np.clip(raw, 0, 1)
        w = np.zeros((n, 4))
        w[:, 0], w[:, i0], w[:, i1] = 1, -(1 - tt), -tt
        dw = np.zeros((n, 4))
        dw[:, i0] = dw[:, i1] = et
        r, dr = p - (s0 + tt[:, None] * ed), et * le + rb.K_POINT * U * (S + M)
        put(1 + 2 * k, w, dw, r, dr, np.full(n, fe), (inside | near) & (le > 0))
        put(2 + 2 * k, w, dw, r, dr, np.where(tt < 0.5, f0, f1_), ~inside | near)
    E &= dcand <= (dref + 2 * delta)[:, None]
    # the reference's own candidate: same weights, same number of free parameters
    wref = np.concatenate([np.ones((n, 1)), -baryref], axis=1)
    nref = np.where(featref == rm.FACE, 2, np.where(featref >= rm.EDGE_AB, 1, 0))
    match = (np.abs(W - wref[:, None, :]).max(axis=2) <= 1e-9) & (nfree == nref[:, None])
    own = np.argmax(match, axis=1) if n else np.zeros(0, int)
    assert match.any(axis=1).all()
    zero = (d2ref == 0) & (d2ref < dhat2)
    H[zero] = 0.0
    return dict(h=H, bound=B, elig=E | (np.arange(C)[None, :] == own[:, None]), own=own, vert=vert, zero=zero, d=dref, delta=delta)


# ------------------------------------------------------------------------------------------------ EE
def ee_candidates64(verts, edge_list, pairs, xdir, dhat2, kappa, psd, rest2=None, M=None):
    """the same of the (edge, edge) pairs; C = 10: the common perpendicular, then (free, clamped) of a0, a1 against b and b0, b1 against a,
    then both parameters free at the reference's closest points (nearly parallel edges, see below)"""
    v, e = rp._v64(verts), np.asarray(edge_list, np.int64).reshape(-1, 2)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    vert = np.concatenate([e[pairs[:, 0]], e[pairs[:, 1]]], axis=1).reshape(n, 4)
    a0, a1, b0, b1 = (v[vert[:, k]] for k in range(4))
    x = np.asarray(xdir, np.float64)[vert]
    d2ref, sref, tref, catref, _ = rp.ee_closest(a0, a1, b0, b1)
    dref = np.sqrt(d2ref)
    M = rp.coord_max(verts) if M is None else M
    u, vv, w0 = a1 - a0, b1 - b0, a0 - b0
    lu, lv = _norm(u), _norm(vv)
    S = dref + lu + lv
    delta = rp.K_EE * U * (S + M) + 1e-37
    nrm = _cross(u, vv)
    c = _dot(nrm, nrm)
    ln = np.sqrt(c)
    eps = np.zeros(n) if rest2 is None else 1e-2 * np.asarray(rest2, np.float64)[pairs[:, 0]] * np.asarray(rest2, np.float64)[pairs[:, 1]]
    eps = np.where(eps >= FLT_MIN, eps, 0.0)
    m, mp = rb.mollifier(c, eps)
    # c, m, m', m'' and their deviations (ref64_barrier.ee_pairs64)
    dn = 10 * U * lu * lv
    dcc = 2 * ln * dn + dn * dn + 3 * U * c
    e1 = np.where(eps > 0, eps, 1.0)
    xx = c / e1
    dx = np.where(eps > 0, dcc / e1 + 17 * U * xx, 0.0)
    dm = np.where(eps > 0, np.minimum(2 * dx + 3 * U * m, 1.0), 0.0)
    dmp = np.where(eps > 0, (2 / e1) * (dx + 20 * U), 0.0)
    far = (eps > 0) & (xx - dx >= 1)
    dm, dmp = np.where(far, 0.0, dm), np.where(far, 0.0, dmp)
    on = (eps > 0) & (c < eps)
    mpp = np.where(on, -2 / (e1 * e1), 0.0)
    dmpp = np.where(eps > 0, np.where(np.abs(xx - 1) <= dx, 2 / (e1 * e1), 35 * U * np.abs(mpp)), 0.0)
    Gu, Gv = 2 * lv * ln, 2 * lu * ln
    dGu, dGv = 2 * lv * (dn + 4 * U * ln), 2 * lu * (dn + 4 * U * ln)
    du, dv = x[:, 1] - x[:, 0], x[:, 3] - x[:, 2]
    adu, adv = _norm(du), _norm(dv)
    N = adu * lv + lu * adv
    C = 10
    H, B, E, nfree, W = np.zeros((n, C, 4, 3)), np.zeros((n, C, 4)), np.zeros((n, C), bool), np.zeros((n, C), int), np.zeros((n, C, 4))
    dcand = np.zeros((n, C))

    def put(k, cs, ct, dw, dr, fs, ft, elig):
        w = np.stack([1 - cs, cs, -(1 - ct), -ct], axis=1)
        r = (w0 + cs[:, None] * u) - ct[:, None] * vv
        dc = _norm(r)
        bb, bp, bpp, db, dbp, dbpp = _scalar3(dc, np.maximum(dc - dref, 0.0) + delta, dhat2, kappa)
        d1, d2, r1, r2 = ee_slots(fs, ft, u, b0, b1)
        hb, bhb, gx, Dgx, ag, Dg = _core_bound(w, dw, r, dr, fs, ft, d1, d2, r1, r2, x, bp, dbp, bpp, dbpp, psd)
        with np.errstate(all="ignore"):
            fin = np.isfinite(bb)
            bsafe = np.where(fin, bb, 0.0)
            h, _ = ee_mollified(hb, gx, w, r, u, vv, x, bsafe, bp, eps, psd)
            ab_, abp = np.abs(bsafe), np.abs(bp)
            nhb = _norm(hb)
            bound = dm[:, None] * (nhb + bhb) + m[:, None] * bhb + U * m[:, None] * nhb
            total = m[:, None] * nhb
            c3, dc3 = np.abs(mp) * ab_, dmp * (ab_ + db) + np.abs(mp) * db + U * np.abs(mp) * ab_
            side = lambda su, sv: np.stack([su, su, sv, sv], axis=1)
            if psd:
                mg = side(2 * lv * N, 2 * lu * N)
                dmg = side(28 * U * lv * N, 28 * U * lu * N)
                bound = bound + dc3[:, None] * (mg + dmg) + c3[:, None] * dmg + U * c3[:, None] * mg
                total = total + c3[:, None] * mg
            else:
                c1, dc1 = np.abs(mp) * abp, dmp * (abp + dbp) + np.abs(mp) * dbp + U * np.abs(mp) * abp
                gcb = Gu * adu + Gv * adv                                  # |grad c . x| is at most this
                agcx = np.abs(_dot(2 * _cross(vv, nrm), du) + _dot(2 * _cross(nrm, u), dv))
                Dgcx = dGu * adu + dGv * adv + U * gcb + 4 * U * gcb
                G, dG = side(Gu, Gv), side(dGu, dGv)
                agx = np.abs(gx)[:, None]
                t1 = dc1[:, None] * agcx[:, None] * ag + (c1 + dc1)[:, None] * (Dgcx[:, None] * (ag + Dg) + agcx[:, None] * Dg) + 3 * U * c1[:, None] * agcx[:, None] * ag
                t2 = dc1[:, None] * agx * G + (c1 + dc1)[:, None] * (Dgx[:, None] * (G + dG) + agx * dG) + 3 * U * c1[:, None] * agx * G
                ampp = np.abs(mpp)
                mag3 = (ab_ * ampp * agcx)[:, None] * G
                t3 = (db * ampp * agcx)[:, None] * G + (ab_ + db)[:, None] * ((dmpp * agcx)[:, None] * G + (ampp + dmpp)[:, None] * (Dgcx[:, None] * (G + dG) + agcx[:, None] * dG)) + 6 * U * mag3
                mg = side(2 * (adv * ln + lv * N), 2 * (adu * ln + lu * N))
                dmg = side(2 * (adv * dn + 10 * U * lv * N) + 12 * U * (adv * ln + lv * N), 2 * (adu * dn + 10 * U * lu * N) + 12 * U * (adu * ln + lu * N))
                t4 = dc3[:, None] * (mg + dmg) + c3[:, None] * dmg + U * c3[:, None] * mg
                bound = bound + t1 + t2 + t3 + t4
                total = total + c1[:, None] * (agcx[:, None] * ag + agx * G) + mag3 + c3[:, None] * mg
            bound = bound + 4 * U * total
            bound = np.where(np.isnan(bound), np.inf, bound)
        H[:, k], B[:, k], E[:, k], nfree[:, k], W[:, k], dcand[:, k] = h, bound, elig, fs.astype(int) + ft.astype(int), w, dc
    # the common perpendicular
    nn1 = np.where(c > 0, c, 1.0)
    si, ti = _dot(_cross(vv, w0), nrm) / nn1, _dot(_cross(u, w0), nrm) / nn1
    with np.errstate(divide="ignore", invalid="ignore"):
        sin = np.where(c > 0, ln / np.where(lu * lv > 0, lu * lv, 1.0), 0.0)
        es = np.where(sin > 0, rb.K_TRIPLE * U * S / np.where(sin > 0, lu * sin, 1.0), np.inf)
        et = np.where(sin > 0, rb.K_TRIPLE * U * S / np.where(sin > 0, lv * sin, 1.0), np.inf)
    dw = np.zeros((n, 4))
    dw[:, :2], dw[:, 2:] = np.minimum(es, 1.0)[:, None], np.minimum(et, 1.0)[:, None]
    yes = np.ones(n, bool)
    put(0, np.clip(si, 0, 1), np.clip(ti, 0, 1), dw, np.minimum(es, 1.0) * lu + np.minimum(et, 1.0) * lv + rb.K_POINT * U * (S + M), yes, yes,
        (c > 0) & (si > -es) & (si < 1 + es) & (ti > -et) & (ti < 1 + et))
    # both parameters free at the reference's closest points: where the edges are nearly parallel the float32 chain's (s, t) are not those
    # of float64 (s = (v x w) . n / |n|^2 with n off by Dn: (v x w) has the component |v| d across n, so s moves by |v| d Dn / |n|^2 =
    # 10 u d / (|u| sin^2), and by 2 s Dn / |n| = 20 u / sin through the denominator), yet they are a pair of points of the segments
    # within delta of the minimum: the two-parameter form with weights anywhere within that tolerance
    with np.errstate(divide="ignore", invalid="ignore"):
        sn = np.where(sin > 0, sin, 1.0)
        es2 = np.where(sin > 0, es + 10 * U * dref / np.where(lu > 0, lu, 1.0) / (sn * sn) + 20 * U / sn, np.inf)
        et2 = np.where(sin > 0, et + 10 * U * dref / np.where(lv > 0, lv, 1.0) / (sn * sn) + 20 * U / sn, np.inf)
    dw = np.zeros((n, 4))
    dw[:, :2], dw[:, 2:] = np.minimum(es2, 1.0)[:, None], np.minimum(et2, 1.0)[:, None]
    put(9, sref, tref, dw, np.minimum(np.minimum(es2, 1.0) * lu + np.minimum(et2, 1.0) * lv + rb.K_POINT * U * (S + M), 2 * dref + delta), yes, yes,
        (c > 0) & (si > -es2) & (si < 1 + es2) & (ti > -et2) & (ti < 1 + et2))
    for k in range(4):
        pt_, s0, s1, le = ((a0, b0, b1, lv), (a1, b0, b1, lv), (b0, a0, a1, lu), (b1, a0, a1, lu))[k]
        ed = s1 - s0
        le1 = np.where(le > 0, le, 1.0)
        raw = np.where(le > 0, _dot(pt_ - s0, ed) / (le1 * le1), 0.0)
        ep = np.where(le > 0, np.minimum(rb.K_SEG * U * S / le1, 1.0), 0.0)
        near = (np.abs(raw) <= ep) | (np.abs(raw - 1) <= ep)
        inside = (raw > 0) & (raw < 1)
        pp = np.clip(raw, 0, 1)
        dw = np.zeros((n, 4))
        if k < 2:
            cs, ct, cols = np.full(n, float(k)), pp, (2, 3)
        else:
            cs, ct, cols = pp, np.full(n, float(k - 2)), (0, 1)
        dw[:, cols[0]] = dw[:, cols[1]] = ep
        dr = ep * le + rb.K_POINT * U * (S + M)
        no = np.zeros(n, bool)
        put(1 + 2 * k, cs, ct, dw, dr, no if k < 2 else yes, yes if k < 2 else no, (inside | near) & (le > 0))
        put(2 + 2 * k, cs, ct, dw, dr, no, no, ~inside | near)
    E &= dcand <= (dref + 2 * delta)[:, None]
    wref = np.stack([1 - sref, sref, -(1 - tref), -tref], axis=1)
    nref = (catref // 3 == rp.INTERIOR).astype(int) + (catref % 3 == rp.INTERIOR).astype(int)
    match = (np.abs(W - wref[:, None, :]).max(axis=2) <= 1e-9) & (nfree == nref[:, None])
    own = np.argmax(match, axis=1) if n else np.zeros(0, int)
    assert match.any(axis=1).all()
    zero = (d2ref == 0) & (d2ref < dhat2)
    H[zero] = 0.0
    return dict(h=H, bound=B, elig=E | (np.arange(C)[None, :] == own[:, None]), own=own, vert=vert, zero=zero, d=dref, delta=delta, m=m)


def pair_ratio(got, q):
    """per pair: the smallest over the eligible candidates of the largest corner error over its bound (0 where the error is exactly zero or
    the bound infinite, inf for an error against a zero bound); also whether every eligible candidate of the pair is unbounded"""
    with np.errstate(invalid="ignore", divide="ignore"):
        err = _norm(np.asarray(got, np.float64)[:, None] - q["h"])
        r = np.where((err == 0) | np.isinf(q["bound"]), 0.0, err / q["bound"]).max(axis=2)
    r = np.where(q["elig"], r, np.inf)
    unb = (np.isinf(q["bound"]).any(axis=2) | ~q["elig"]).all(axis=1)
    return (r.min(axis=1) if r.shape[0] else np.zeros(0)), unb


def some_unbounded(q):
    """per pair: an eligible candidate has an infinite bound, so the pair passes whatever the device returned"""
    return (np.isinf(q["bound"]).any(axis=2) & q["elig"]).any(axis=1)


def own(q):
    """(h [n, 4, 3] of the reference's own candidate, spread bound [n, 4]: the largest over the eligible candidates of
    |h_candidate - h_own| + the candidate's bound)"""
    n = len(q["own"])
    i = np.arange(n)
    h = q["h"][i, q["own"]]
    with np.errstate(invalid="ignore"):
        s = np.where(q["elig"][:, :, None], _norm(q["h"] - h[:, None]) + q["bound"], 0.0)
    s = np.where(np.isnan(s), np.inf, s)
    return h, (s.max(axis=1) if n else np.zeros((0, 4)))


# ------------------------------------------------------------------------------------------------ a scene
class Reference:
    """H x and its bounds of a constraint set at positions verts for the direction xdir [nv, 3]: pt / ee (the candidate dicts), hx [nv, 3],
    pair_terms [npt + nee, 4, 3] (own candidates), vbound [nv], ninc [nv], zero = (pt, ee)"""

    def __init__(self, verts, tris, pt_pairs, ee_pairs, dhat, kappa, xdir, rest2=None, edge_list=None, psd=False):
        nv = len(rp._v64(verts))
        self.dhat2 = rb.dhat2_f32(dhat)
        e = rp.edges(tris) if edge_list is None else edge_list
        M = rp.coord_max(verts)
        xdir = np.asarray(np.asarray(xdir, np.float32), np.float64)
        self.pt = pt_candidates64(verts, tris, np.zeros((0, 2), int) if pt_pairs is None else pt_pairs, xdir, self.dhat2, kappa, psd, M)
        self.ee = ee_candidates64(verts, e, np.zeros((0, 2), int) if ee_pairs is None else ee_pairs, xdir, self.dhat2, kappa, psd, rest2, M)
        self.zero = (int(self.pt["zero"].sum()), int(self.ee["zero"].sum()))
        self.hx, self.vbound, self.ninc, mag = np.zeros((nv, 3)), np.zeros(nv), np.zeros(nv, np.int64), np.zeros(nv)
        terms = []
        for q in (self.pt, self.ee):
            h, s = own(q)
            terms.append(h)
            idx = q["vert"].ravel()
            np.add.at(self.hx, idx, h.reshape(-1, 3))
            np.add.at(self.vbound, idx, s.ravel())
            np.add.at(self.ninc, idx, 1)
            np.add.at(mag, idx, (_norm(h) + np.where(np.isfinite(s), s, 0.0)).ravel())
        self.pair_terms = np.concatenate(terms)
        self.vbound = self.vbound + self.ninc * U * mag + 1e-37


# ------------------------------------------------------------------------------------------------ autograd, twice
def autograd_hvp(verts, tris, edge_list, pt_pairs, ee_pairs, dhat2, kappa, rest2, dirs):
    """[H x for x in dirs] with torch.autograd's double backward in float64 through the min-over-candidates energy of
    ref64_barrier.autograd_energy (a copy that keeps the graph)"""
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
    out = []
    if not total.requires_grad or total.grad_fn is None:
        return [np.zeros(tuple(x.shape)) for _ in dirs]
    g, = torch.autograd.grad(total, x, create_graph=True)
    if not g.requires_grad:
        return [np.zeros(tuple(x.shape)) for _ in dirs]
    for dvec in dirs:
        hv, = torch.autograd.grad((g * torch.as_tensor(np.asarray(dvec, np.float64))).sum(), x, retain_graph=True, allow_unused=True)
        out.append(np.zeros(tuple(x.shape)) if hv is None else hv.numpy().copy())
    return out
