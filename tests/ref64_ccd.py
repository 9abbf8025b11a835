"""Float64 restatement of the additive CCD of include/zensim_rocm/ccd_device.hpp (zpc_amd/csrc/mesh_ccd.hip, TriMesh.max_step), numpy
only, on top of ref64_proximity / ref64_mesh: accd() in float64 is the reference, accd(f32=True) replays the device chain operation by
operation in float32 (the translation units are built without FP contraction), directions() are the test directions of a scene, and
check() holds a returned step t -- a float32 number taken as exact -- against the two properties below.  Distances are float64, from the
float32 inputs, at x + t p.

Notation: u = 2^-24, sl = slack, d0 = the float64 distance at t = 0, l_p = the float64 bound on the relative speed (mean of the four rows
subtracted; PT |q_0| + max |q_1..3|, EE max |q_0,1| + max |q_2,3|), beta = K u (S + M) the bound of ref64_proximity on one float32
distance (K = 32 PT, 64 EE), taken with S and M at their largest over the step: the distance at most max(d0, d(t)), the edge lengths at
most their larger end value (the length of a linearly moving edge is convex in t), M over x and x + t_max p.

P1, conservative.  (a) The Lipschitz walk tau = 0, tau += d(tau) / l_p finds d > 0 at every stop and reaches t within
ceil(max_iter / 0.9) + 1 steps: no contact anywhere in [0, t], certified without trusting the loop under test.  The device never steps
further than the walk would while d >= 9 beta (its step is 0.9 d32 / l_p32, d32 <= d + beta, l_p32 >= l_p), and tau + d(tau) / l_p is
monotone in tau, so the walk that starts level stays ahead; 1 / 0.9 and the first step are the issue's allowance.
(b) d(t) >= sl d0 - C1 beta.  Every t > 0 the loop returns was accepted: its float32 distance was >= g32 = fl(sl32 d0_32), except the
first increment, which is taken unchecked.
    accepted point:   d(t) >= d32(t) - beta - 4 u M        (the device measures at fl(x + fl(t p)): 2 u M per corner, two corners)
                           >= g32 - 1.125 beta              (4 u M = beta / 8 at K = 32)
                      g32  >= sl (d0 - beta)(1 - u)  >=  sl d0 - sl beta - beta / 32
                      d(t) >= sl d0 - (1.125 + sl + 1 / 32) beta  >=  sl d0 - 2.2 beta
    first increment:  t_l = fl(fl((1 - sl) d0_32) / l_p32) <= (1 - sl)(d0 + beta)(1 + 2 u) / l_p, the distance falls by at most l_p t_l:
                      d(t_l) >= sl d0 - beta - 2 u d0 >= sl d0 - 1.07 beta
    C1 = 3.
P2, not vacuous, for a pair that stopped at a break (t < t_max, neither capped nor zero distance): d(t) <= 10 sl d0 + C2 beta.  The break
means d32(t') < g32 at t' = t + fl(fl(0.9f d32(t)) / l_p32), and the distance falls by at most l_p (t' - t) <= 0.9 (1 + 2 u)(d(t) + beta)
(0.9f < 0.9):
    d(t) <= d(t') + 0.9 (1 + 2 u)(d(t) + beta),   d(t') <= g32 + 1.125 beta
    d(t) (0.1 - 1.8 u) <= sl d0_32 (1 + u) + 2.03 beta
    d(t) <= 10 (1 + 18 u)(sl (d0 + beta)(1 + u) + 2.03 beta) <= 10 sl d0 + 190 u sl d0 + (10 sl + 20.4) beta,   u d0 <= beta / 32
    C2 = 22 + 16 sl.
It says nothing at sl = 0.1 (ten times the gap is the starting distance), so it is tested at sl = 0.01.
Below resolution: a pair with sl d0 <= 2 beta.  For it only 0 <= t <= t_max, finiteness and d > 0 along the walk of P1 (a) are
asserted (the float32 distance is mostly error there, so the loop's steps are not held to the walk's budget); check() counts them.
The float64 reference is held to the same properties with beta replaced by the float64 rounding 2^-40 (S + M).
"""
import zlib

import numpy as np

import ref64_mesh as rm
import ref64_proximity as rp
from ref64_mesh import U, tri_closest

OK, ZERO, CAPPED = 0, 1, 2
LP_UP32, LP_TINY32, ADVANCE32 = np.float32(1 + 2.0 ** -21), np.float32(1e-10), np.float32(0.9)
FLT_MAX = np.finfo(np.float32).max
C1 = 3.0


def c2(slack):
    return 22.0 + 16.0 * float(np.float32(slack))


def distance(Y, ee, f32=False):
    """distance of the pairs Y [n, 4, 3] (point, a, b, c / a0, a1, b0, b1) in the dtype of Y; f32: the device's thresholds"""
    if ee:
        d2 = rp.ee_closest(Y[:, 0], Y[:, 1], Y[:, 2], Y[:, 3], rp.PARALLEL32 if f32 else 0.0)[0]
    else:
        d2 = tri_closest(Y[:, 0], Y[:, 1], Y[:, 2], Y[:, 3], rm.DEGENERATE32 if f32 else 0.0)[0]
    return np.sqrt(d2)


def speed_bound(P, ee, f32=False):
    """l_p of the rows P [n, 4, 3]: exact mean in float64, the device's chain (rounded up) in float32"""
    if f32:
        f = np.float32
        m = ((P[:, 0] + P[:, 1]) + (P[:, 2] + P[:, 3])) * f(0.25)
        q = P - m[:, None, :]
        n = np.sqrt((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2])
        amax = np.abs(q).max(axis=(1, 2)) if len(q) else np.zeros(0, f)
    else:
        q = P - P.mean(axis=1, keepdims=True)
        n = np.sqrt((q * q).sum(axis=2))
    lp = (np.maximum(n[:, 0], n[:, 1]) + np.maximum(n[:, 2], n[:, 3])) if ee else (n[:, 0] + np.maximum(n[:, 1], np.maximum(n[:, 2], n[:, 3])))
    if f32:
        lp = np.where(amax < LP_TINY32, f(4) * amax, lp * LP_UP32).astype(f)
    return lp


def accd(X, P, ee, slack=0.1, t_max=1.0, max_iter=256, f32=False):
    """additive CCD of the pairs X, P [n, 4, 3] (float32 numbers): dict(t, status, evals, early, d0, lp, first) in float64, or with f32 the
    device's chain in float32.  early: left at the early out; first: the first increment"""
    f = np.float32 if f32 else np.float64
    X, P = (np.asarray(np.asarray(a, np.float32), f).reshape(-1, 4, 3) for a in (X, P))
    n = len(X)
    sl, tm = f(np.float32(slack)), f(np.float32(t_max))
    adv_c = ADVANCE32 if f32 else 0.9
    t, status, evals = np.zeros(n, f), np.zeros(n, np.int32), np.zeros(n, np.int32)
    fin = np.isfinite(X).all(axis=(1, 2)) & np.isfinite(P).all(axis=(1, 2))
    Xs, Ps = np.where(fin[:, None, None], X, f(0)), np.where(fin[:, None, None], P, f(0))
    with np.errstate(all="ignore"):
        lp = speed_bound(Ps, ee, f32)
        ok = fin & (lp <= FLT_MAX)
        still = ok & (lp == 0)
        t[still] = tm
        d0 = distance(Xs, ee, f32)
        ok &= ~still & (d0 <= FLT_MAX)
        zero = ok & (d0 == 0)
        status[zero] = ZERO
        ok &= ~zero
        g = sl * d0
        tl = ((f(1) - sl) * d0) / np.where(lp == 0, f(1), lp)
        early = ok & (tl >= tm)
        t[early] = tm
        first = np.where(ok, tl, f(0))
        act = np.nonzero(ok & ~early)[0]
        while len(act):
            tt = t[act] + tl[act]
            tt = np.where(tt >= tm, tm, tt)       # the evaluation is clamped to t_max, so the gap is known there
            d = distance(X[act] + tt[:, None, None] * P[act], ee, f32)
            evals[act] += 1
            stop = ~(d >= g[act]) & ((t[act] > 0) | np.isnan(d))
            ia, tt, d = act[~stop], tt[~stop], d[~stop]
            t[ia] = tt
            reach = tt >= tm
            tl[ia] = (f(adv_c) * d) / lp[ia]
            cap = ~reach & (evals[ia] >= max_iter)
            status[ia[cap]] = CAPPED
            act = ia[~reach & ~cap]
    return dict(t=t, status=status, evals=evals, early=early, d0=d0, lp=lp, first=first)


# ------------------------------------------------------------------------------------------------ pairs of a scene, directions
def corners(tris, edge_list, pairs, ee):
    """vertex numbers [n, 4] of (vertex, triangle) or (edge, edge) pairs"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if ee:
        e = np.asarray(edge_list, np.int64).reshape(-1, 2)
        return np.concatenate([e[pairs[:, 0]], e[pairs[:, 1]]], axis=1)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    return np.concatenate([pairs[:, :1], t[pairs[:, 1]]], axis=1)


DIRECTIONS = ("translate", "zero", "random", "approach", "slide", "shrink")


def direction(name, verts, which):
    """the test direction `which` of scene `name` [nv, 3] float32, seeded by the scene's name; None where it is not defined (approach: the
    two-sheet scenes only)"""
    v = np.asarray(verts, np.float32)
    n = len(v)
    g = np.random.default_rng(zlib.crc32(name.encode()))
    rnd = g.uniform(-0.02, 0.02, (n, 3))
    half = np.arange(n) >= n // 2
    if which == "translate":
        p = np.broadcast_to(np.array([0.013, -0.021, 0.017]), (n, 3))
    elif which == "zero":
        p = np.zeros((n, 3))
    elif which == "random":
        p = rnd
    elif which == "approach":
        if name not in ("sheets", "regular"):
            return None
        p = rnd + half[:, None] * np.array([0.0, 0.0, -0.06])
    elif which == "slide":
        p = half[:, None] * np.array([0.1, 0.0, 0.0])
    elif which == "shrink":
        p = 0.3 * (0.5 - v.astype(np.float64))
    else:
        raise KeyError(which)
    return np.ascontiguousarray(p, np.float32)


def scene_pairs(name, radius=None):
    """(verts, tris, edges, pt pairs, ee pairs, dhat): the float64 brute force of the scene at radius / 2 (ref64_proximity keeps every pair
    within twice its argument), radius defaulting to the scene's dHat"""
    v, t, dhat = rp.scene(name)
    R = rp.Reference(v, t, 0.5 * (dhat if radius is None else radius))
    return v, t, R.edges, R.pt, R.ee, dhat


# ------------------------------------------------------------------------------------------------ the two properties
def _sizes(X, P, ee, t_max):
    """(edge term of S, largest coordinate) at their largest over [0, t_max]"""
    E = np.zeros(len(X))
    for Y in (X, X + float(t_max) * P):
        if ee:
            e = np.linalg.norm(Y[:, 1] - Y[:, 0], axis=1) + np.linalg.norm(Y[:, 3] - Y[:, 2], axis=1)
        else:
            e = np.maximum(np.maximum(np.linalg.norm(Y[:, 2] - Y[:, 1], axis=1), np.linalg.norm(Y[:, 3] - Y[:, 2], axis=1)),
                           np.linalg.norm(Y[:, 1] - Y[:, 3], axis=1))
        E = np.maximum(E, e)
    return E


def walk(X, P, ee, t, budget):
    """P1 (a): (reached, positive) per pair -- the float64 Lipschitz walk from 0 reaches t within budget steps, all distances on it > 0"""
    n = len(X)
    lp = speed_bound(P, ee)
    tau, positive = np.zeros(n), np.ones(n, bool)
    act = np.nonzero(tau < t)[0]
    for _ in range(int(budget)):
        if not len(act):
            break
        d = distance(X[act] + tau[act, None, None] * P[act], ee)
        positive[act[~(d > 0)]] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            tau[act] = np.where(d > 0, tau[act] + d / lp[act], tau[act])
        act = act[(d > 0) & (tau[act] < t[act])]
    return ~(tau < t), positive


def check(X, P, ee, res, slack, t_max, max_iter, M=None, exact=False):
    """holds res (of accd(f32=True), of the device, or with exact of accd in float64) against P1 and P2; X, P [n, 4, 3] float32 numbers.
    Returns dict(ok, p1, p2, below, hits, n_break): ok = every assertion holds, p1 / p2 = the worst shortfall in units of its bound
    (<= 1 passes), below = pairs under resolution, hits = pairs with t < t_max"""
    X, P = (np.asarray(np.asarray(a, np.float32), np.float64).reshape(-1, 4, 3) for a in (X, P))
    t = np.asarray(res["t"]).astype(np.float64)
    status = np.asarray(res["status"])
    n = len(X)
    sl, tm = float(np.float32(slack)), float(np.float32(t_max))
    out = dict(ok=True, p1=0.0, p2=0.0, below=0, hits=int((t < tm).sum()), n_break=0, resolved=np.zeros(len(X), bool))
    if not n:
        return out
    fin = np.isfinite(X).all(axis=(1, 2)) & np.isfinite(P).all(axis=(1, 2))
    ok = np.isfinite(t).all() and (t >= 0).all() and (t <= tm).all() and (t[~fin] == 0).all()
    X, P, t, status = X[fin], P[fin], t[fin], status[fin]
    d0 = distance(X, ee)
    dt = distance(X + t[:, None, None] * P, ee)
    if M is None:
        M = np.maximum(np.abs(X).max(axis=(1, 2)), np.abs(X + tm * P).max(axis=(1, 2)))    # the pair's own largest coordinate
    k = (2.0 ** -40) if exact else (rp.K_EE if ee else rp.K_PT) * U
    beta = k * (np.maximum(d0, dt) + _sizes(X, P, ee, tm) + M) + (0.0 if exact else 1e-37)
    below = (sl * d0 <= 2 * beta) & (d0 > 0)
    reached, positive = walk(X, P, ee, t, np.ceil(max_iter / 0.9) + 1)
    late = np.nonzero(below & ~reached & positive)[0]
    if len(late):       # under resolution the float32 distance is mostly error and the loop's steps are not the walk's: d > 0 is what is asked
        positive[late] = walk(X[late], P[late], ee, t[late], 1 << 14)[1]
        reached[late] = True
    ok = ok and bool((reached & positive).all()) and bool(((status == ZERO) == (d0 == 0)).all() or not exact)
    out["below"] = int((below & (t < tm)).sum())
    res_ok = ~below & (d0 > 0)
    out["resolved"][np.nonzero(fin)[0][res_ok]] = True
    if res_ok.any():
        out["p1"] = float(((sl * d0 - dt)[res_ok] / (C1 * beta[res_ok])).max())
    brk = res_ok & (t < tm) & (status == OK)
    out["n_break"] = int(brk.sum())
    if brk.any():
        out["p2"] = float(((dt - 10 * sl * d0)[brk] / (c2(slack) * beta[brk])).max())
    out["ok"] = bool(ok and out["p1"] <= 1 and out["p2"] <= 1)
    return out
