"""Replay of the mesh incremental potential (zpc_amd/csrc/mesh_potential.hip, include/zensim_rocm/potential_device.hpp), numpy only, in
the device's order and in a dtype of choice: float32 replays the device operation by operation (the translation unit is built without FP
contraction), float64 is the reference.

    E(x) = 1/2 (x - xt)^T M (x - xt) + scale (Psi_elastic(x) + B(x) + D(x - start))

    inertia       per free vertex d = x - xt, e = (0.5 mass) ((d0 d0 + d1 d1) + d2 d2); zero at a fixed vertex
    gradient      g = mass d + scale acc, acc the sum over up to four runs per vertex (ref64_terms.gather), the zero row at a fixed vertex
    parts         float32: each part the float64 fixed-order total of its float32 energies (ref64_terms.total); float64: plain sums
    compose       E = parts[0] + (double) scale ((parts[1] + parts[2]) + parts[3])
    search        the backtracking line search of the header, its decisions in float64; energy_at(x_k, u_k) -> E_k is the caller's
    Potential     E and g in dtype on a ref64_solve.System from the evaluations of ref64_elastic / ref64_barrier / ref64_friction
"""
import numpy as np

import ref64_barrier as rb
import ref64_elastic as rl
import ref64_friction as rf
import ref64_mesh as rm
import ref64_proximity as rp
import ref64_solve as rs
import ref64_terms as rt

FLAGS = ("running", "accepted", "max_trials", "not_descent", "not_finite")


def inertia(x, target, mass, fx, dtype=np.float32):
    """(e [nv], d [nv, 3]) of potential_inertia; fx [nv] bool: the fixed vertices (ref64_solve.fixed_mask)"""
    dt = np.dtype(dtype).type
    x, target, m = np.asarray(x, dtype), np.asarray(target, dtype), np.asarray(mass, dtype)
    with np.errstate(all="ignore"):
        d = x - target
        e = (dt(0.5) * m) * ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return np.where(fx, dt(0), e).astype(dtype), d


def gradient(d, mass, scale, acc, fx, dtype=np.float32):
    """potential_gradient: g = mass d + scale acc, zero rows at fixed vertices"""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        g = np.asarray(mass, dtype)[:, None] * np.asarray(d, dtype) + dt(scale) * np.asarray(acc, dtype)
    return np.where(fx[:, None], dt(0), g).astype(dtype)


def total(energies, dtype=np.float32):
    """one part from its per-element energies (a list of arrays, one behind the other)"""
    e = np.concatenate([np.asarray(a).reshape(-1) for a in energies]) if len(energies) else np.zeros(0)
    with np.errstate(all="ignore"):
        return float(rt.total(e)) if np.dtype(dtype) == np.float32 else float(np.asarray(e, np.float64).sum())


def compose(parts, scale):
    """potential_energy; scale as the float32 the device holds"""
    with np.errstate(all="ignore"):
        return float(np.float64(parts[0]) + np.float64(np.float32(scale)) * ((np.float64(parts[1]) + np.float64(parts[2])) + np.float64(parts[3])))


def slope(g, p, fx):
    """g . p as the solve's dot, fixed vertices contributing 0"""
    return rs.dot(g, np.where(fx[:, None], 0, np.asarray(p)).astype(np.asarray(g).dtype))


def trial(x, p, t, fx, dtype=np.float32):
    """potential_trial: x + t p per component, x at a fixed vertex"""
    x, p = np.asarray(x, dtype), np.asarray(p, dtype)
    with np.errstate(all="ignore"):
        return np.where(fx[:, None], x, x + np.dtype(dtype).type(t) * p).astype(dtype)


def armijo(ek, e0, c1, tk, slope_):
    """potential_armijo, c1 and tk float32"""
    with np.errstate(all="ignore"):
        return bool(np.isfinite(ek) and ek <= e0 + (np.float64(np.float32(c1)) * np.float64(np.float32(tk))) * np.float64(slope_))


def search(energy_at, x, p, e0, slope_, t_max, fx, start=None, c1=1e-4, shrink=0.5, max_trials=30, dtype=np.float32):
    """the line search of mesh_potential.hip: dict(x, t, energy, slope, trials, energies [trials + 1] float64, flag).  energy_at(x_k, u_k)
    -> E_k (u_k None without start); t_k is a float32 whatever dtype the positions have"""
    f = np.float32
    x = np.asarray(x, dtype)
    hist = [float(e0)]
    out = lambda flag, xk, t, e: dict(x=xk, t=float(t), energy=float(e), slope=float(slope_), trials=len(hist) - 1, energies=np.array(hist, np.float64),
                                      flag=flag)
    with np.errstate(all="ignore"):
        t = f(t_max)
        if not (np.isfinite(e0) and np.isfinite(slope_) and np.isfinite(t) and t > 0):
            return out("not_finite", x.copy(), 0.0, e0)
        if not slope_ < 0:
            return out("not_descent", x.copy(), 0.0, e0)
        for _ in range(max_trials):
            xk = trial(x, p, t, fx, dtype)
            uk = None if start is None else (xk - np.asarray(start, dtype)).astype(dtype)
            ek = float(energy_at(xk, uk))
            hist.append(ek)
            if armijo(ek, e0, c1, t, slope_):
                return out("accepted", xk, t, ek)
            t = f(shrink) * t
    return out("max_trials", x.copy(), 0.0, e0)


def pt64(p, a, b, c, dhat2, kappa):
    """(energy [n], g [n, 4, 3]) of (vertex, triangle) pairs at float64 corner positions: b(d2) and 2 b' w (p - closest point)"""
    d2, cp, bary, _ = rm.tri_closest(p, a, b, c)
    bb, bp = rb.barrier(d2, dhat2, kappa)
    w = np.concatenate([np.ones((len(d2), 1)), -bary], axis=1)
    return bb, (2 * bp)[:, None, None] * w[:, :, None] * (p - cp)[:, None, :]


def ee64(a0, a1, b0, b1, dhat2, kappa, eps):
    """the same of (edge, edge) pairs with the mollifier of nearly parallel edges (eps [n], 0: none): m b and m 2 b' w r + m' b grad c"""
    d2, s, t, _, _ = rp.ee_closest(a0, a1, b0, b1)
    bb, bp = rb.barrier(d2, dhat2, kappa)
    u, v = a1 - a0, b1 - b0
    n = rm._cross(u, v)
    m, mp = rb.mollifier(rm._dot(n, n), np.where(eps >= rb.FLT_MIN, eps, 0.0))
    w = np.stack([1 - s, s, -(1 - t), -t], axis=1)
    r = (a0 + s[:, None] * u) - (b0 + t[:, None] * v)
    gcu, gcv = 2 * rm._cross(v, n), 2 * rm._cross(n, u)
    gc = np.stack([-gcu, gcu, -gcv, gcv], axis=1)
    with np.errstate(invalid="ignore"):
        bsafe = np.where(np.isfinite(bb), bb, 0.0)
        g = (2 * m * bp)[:, None, None] * w[:, :, None] * r[:, None, :] + (mp * bsafe)[:, None, None] * gc
        return np.where(np.isfinite(bb), m * bsafe, np.inf), g


class Potential:
    """E and its gradient in dtype on a ref64_solve.System S (its mass, scale, fixed and terms; its linearization point is not used), the
    inertia target and the positions start at the start of the step (friction is taken at u = x - start)"""

    def __init__(self, S, target, start=None):
        self.S, self.dtype = S, S.dtype
        self.target = np.asarray(np.asarray(target, np.float32), S.dtype)
        self.start = None if start is None else np.asarray(np.asarray(start, np.float32), S.dtype)
        if S.friction is not None and start is None:
            raise ValueError("friction needs start")
        self.fx = rs.fixed_mask(np.asarray(S.mass, S.dtype), S.fixed)

    def elements(self, x, u, grad=True):
        """per term that is present: (its per-element energies as a list of arrays, its runs for ref64_terms.gather); grad: the energies and
        terms of the gradient operations, else the energies of the energy operations and no runs"""
        S, f32 = self.S, self.dtype == np.float32
        out = {}
        if S.elastic is not None:
            mu, lam, kb = S.elastic
            R = S.rest      # (not R.evaluate: it rounds the positions to float32, and a float64 difference quotient moves them by less)
            T, H = rl.tri_eval(R.tri_record, x[R.tris], mu, lam), rl.hinge_eval(R.hinge_record, x[R.hinges], kb)
            if not (mu > 0 or lam > 0):
                T = {k: np.zeros_like(v) for k, v in T.items()}
            if not kb > 0:
                H = {k: np.zeros_like(v) for k, v in H.items()}
            k = "eg" if grad else "e"
            out["elastic"] = ([T[k], H[k]], [S.rest.tri_inc + (T["g"].reshape(-1, 3),), S.rest.hinge_inc + (H["g"].reshape(-1, 3),)])
        if S.barrier is not None:
            b = S.barrier
            dhat2, r2, npt = rb.dhat2_f32(b["dhat"]), b.get("rest2"), len(b["pt"])
            if f32:
                P = np.asarray(x, np.float32)[b["vert"]]
                eps = np.zeros(len(b["ee"]), np.float32) if r2 is None else rb.ee_eps32(np.asarray(r2, np.float32)[b["ee"][:, 0]],
                                                                                         np.asarray(r2, np.float32)[b["ee"][:, 1]])
                ep, gp, _ = rb.pt32(P[:npt, 0], P[:npt, 1], P[:npt, 2], P[:npt, 3], dhat2, b["kappa"])
                ee, ge, _ = rb.ee32(P[npt:, 0], P[npt:, 1], P[npt:, 2], P[npt:, 3], dhat2, b["kappa"], eps)
            else:
                P = x[b["vert"]]
                eps = np.zeros(len(b["ee"])) if r2 is None else (np.float64(np.float32(1e-2)) * np.asarray(np.asarray(r2, np.float32), np.float64)[
                    b["ee"][:, 0]]) * np.asarray(np.asarray(r2, np.float32), np.float64)[b["ee"][:, 1]]
                ep, gp = pt64(P[:npt, 0], P[:npt, 1], P[:npt, 2], P[:npt, 3], dhat2, b["kappa"])
                ee, ge = ee64(P[npt:, 0], P[npt:, 1], P[npt:, 2], P[npt:, 3], dhat2, b["kappa"], eps)
            out["barrier"] = ([ep, ee], [b["inc"] + (np.concatenate([gp, ge]).reshape(-1, 3),)])
        if S.friction is not None:
            fr = S.friction
            r = (rf.evaluate32 if f32 else rf.evaluate64)(fr["record"], np.asarray(u, self.dtype)[fr["vert"]], fr["mu"], fr["eps_v"])
            npt = len(fr["pt"])
            e = r["eg" if (grad and f32) else "e"]
            out["friction"] = ([e[:npt], e[npt:]], [fr["inc"] + (np.asarray(r["g"]).reshape(-1, 3),)])
        return out

    def evaluate(self, x, grad=True):
        """dict(parts [4] float64, energy, grad [nv, 3] or None) at x"""
        S, dtype = self.S, self.dtype
        x = np.asarray(x, dtype)
        u = None if self.start is None else (x - self.start).astype(dtype)
        el = self.elements(x, u, grad)
        e_in, d = inertia(x, self.target, S.mass, self.fx, dtype)
        parts = [total([e_in], dtype)] + [total(el[k][0], dtype) if k in el else 0.0 for k in ("elastic", "barrier", "friction")]
        g = None
        if grad:
            runs = [r for k in ("elastic", "barrier", "friction") if k in el for r in el[k][1]]
            acc = rt.gather(S.nv, runs, dtype) if runs else np.zeros((S.nv, 3), dtype)
            g = gradient(d, S.mass, S.scale, acc, self.fx, dtype)
        return dict(parts=np.array(parts, np.float64), energy=compose(parts, S.scale), grad=g)

    def energy_at(self, xk, uk=None):
        return self.evaluate(xk, grad=False)["energy"]

    def line_search(self, x, p, t_max, c1=1e-4, shrink=0.5, max_trials=30):
        x, p = np.asarray(x, self.dtype), np.asarray(p, self.dtype)
        v = self.evaluate(x)
        return search(self.energy_at, x, p, v["energy"], slope(v["grad"], p, self.fx), t_max, self.fx, self.start, c1, shrink, max_trials, self.dtype)


# ------------------------------------------------------------------------------------------------ the cases of the tests
# the line-search cases on `sheets` at displaced positions along multiples of the Newton direction d (the PCG solution of A d = -g), all
# with t_max = 1: name -> (multiple of d, keywords of the search, flag, trials).  Chosen on the CPU with the float64 replay
# (tests/test_potential_cpu.py asserts them): d itself is accepted at the first trial; 8 d overshoots -- the trials at t = 1 and 1 / 2 raise
# the energy -- and is accepted at t = 1 / 4, the third trial; with one trial allowed the same search ends with max_trials; -d ascends.  The
# fifth case, a NaN in the target, is not_finite before any trial.
SEARCH_CASES = {"newton": (1.0, {}, "accepted", 1), "overshoot": (8.0, {}, "accepted", 3), "one_trial": (8.0, dict(max_trials=1), "max_trials", 1),
                "ascent": (-1.0, {}, "not_descent", 0)}


def step_arrays(verts, tris):
    """(x, target, start) float32 of the tests' implicit step on a scene: x = displaced(.., 1e-1), start = x - small_displacement (the
    friction displacement of the solve tests), target = x plus a seeded offset of 1e-3"""
    x = rl.displaced(verts, tris, 1, 1e-1)
    start = x - rs.small_displacement(len(x))
    target = (x.astype(np.float64) + 1e-3 * np.random.default_rng(90).standard_normal(x.shape)).astype(np.float32)
    return x, target, start.astype(np.float32)
