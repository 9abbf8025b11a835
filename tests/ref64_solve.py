"""Replay of the mesh Newton system (zpc_amd/csrc/mesh_solve.hip, include/zensim_rocm/solve_device.hpp), numpy only, in the device's
order and in a dtype of choice: float32 replays the device operation by operation (the translation unit is built without FP contraction),
float64 is the reference.

    combine / inverse   the per-vertex 3 x 3 blocks (xx, xy, xz, yy, yz, zz): scale ((elastic + barrier) + friction) plus the mass on the
                        diagonal; adjugate over determinant with the scalar Jacobi fallback, operation by operation as the header has it
    dot                 sum_v ((a0 b0 + a1 b1) + a2 b2) in float64: 256 vertices per workgroup, an LDS tree, then one workgroup over the
                        partials (thread t adds t, t + 256, .. front to back, the same tree)
    operator            q = mass x + scale acc, acc the float sum over up to four runs per vertex (ref64_terms.gather), zero at a fixed vertex
    pcg                 the solver of the .hip file's header comment, the scalars rounded to dtype once
    System              the operator in dtype from the evaluations of ref64_elastic / ref64_barrier_hessian / ref64_friction: the per-element
                        products, the blocks from unit directions per element (what the device does) and from unit directions per vertex
                        (the definition), the dense matrix column by column and the energy of the incremental potential's terms.
"""
import numpy as np

import ref64_barrier as rb
import ref64_barrier_hessian as rbh
import ref64_elastic as rl
import ref64_friction as rf
import ref64_mesh as rm
import ref64_proximity as rp
import ref64_terms as rt

FLAGS = ("running", "converged", "max_iters", "breakdown", "not_finite")
SLOT = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # (i, j) of the six stored entries


def strip(a, b, seed=5):
    """(a + 1) x (b + 1) vertices, spacing 0.004, jittered in all three coordinates; two triangles per cell (the strips of the elastic
    tests): nv = (a + 1) (b + 1)"""
    h = 0.004
    i, j = np.meshgrid(np.arange(a + 1), np.arange(b + 1), indexing="ij")
    v = np.stack([0.2 + h * i, 0.2 + h * j, np.full(i.shape, 0.5)], axis=-1).reshape(-1, 3)
    v = v + 0.4 * h * (np.random.default_rng(seed).random(v.shape) - 0.5)
    idx = lambda p, q: p * (b + 1) + q
    t = []
    for p in range(a):
        for q in range(b):
            t += [(idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)), (idx(p, q), idx(p + 1, q + 1), idx(p, q + 1))]
    return v.astype(np.float32), np.array(t, np.int32)


# ------------------------------------------------------------------------------------------------ blocks
def mass_ok(mass):
    m = np.asarray(mass)
    with np.errstate(invalid="ignore"):
        return (m > 0) & (m <= np.finfo(m.dtype).max)


def fixed_mask(mass, fixed):
    f = ~mass_ok(mass)
    return f if fixed is None else f | (np.asarray(fixed) != 0)


def combine(el, ba, fr, scale, mass, dtype=np.float32):
    """block_combine: [nv, 6]"""
    dt = np.dtype(dtype).type
    el, ba, fr, m = (np.asarray(a, dtype) for a in (el, ba, fr, mass))
    with np.errstate(all="ignore"):
        D = dt(scale) * ((el + ba) + fr)
        for k in (0, 3, 5):
            D[:, k] = D[:, k] + m
    return D


def inverse(D, mass, dtype=np.float32):
    """block_inverse: (inverse [n, 6], fallback [n] bool)"""
    dt = np.dtype(dtype).type
    D, mass = np.asarray(D, dtype), np.asarray(mass, dtype)
    fin = lambda x: np.abs(x) <= np.finfo(dtype).max
    with np.errstate(all="ignore"):
        a, b, c, d, e, f = (D[:, k] for k in range(6))
        c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
        c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
        det = (a * c00 + b * c01) + c * c02
        inv = np.stack([c00, c01, c02, c11, c12, c22], axis=1) / det[:, None]
        ok = (det > 0) & fin(det) & fin(inv).all(axis=1)
        rm_ = dt(1) / mass
        diag = np.stack([a, d, f], axis=1)
        q = dt(1) / diag
        r = np.where((diag > 0) & fin(diag) & fin(q), q, rm_[:, None])
        z = np.zeros_like(a)
        fb = np.stack([r[:, 0], z, z, r[:, 1], z, r[:, 2]], axis=1)
    return np.where(ok[:, None], inv, fb).astype(dtype), ~ok


def precondition(D, mass, fixed=None, dtype=np.float32):
    """what solve_block_combine_kernel leaves in `inverse`: (inverse with zero blocks at fixed vertices, fallbacks, masses treated as fixed)"""
    inv, fb = inverse(D, mass, dtype)
    fx = fixed_mask(np.asarray(mass, dtype), fixed)
    return np.where(fx[:, None], np.dtype(dtype).type(0), inv).astype(dtype), int((fb & ~fx).sum()), int((~mass_ok(np.asarray(mass, dtype))).sum())


def apply_block(B, r):
    """block_apply: z = B r, every row left to right, in the dtype of B"""
    with np.errstate(all="ignore"):
        return np.stack([(B[:, 0] * r[:, 0] + B[:, 1] * r[:, 1]) + B[:, 2] * r[:, 2], (B[:, 1] * r[:, 0] + B[:, 3] * r[:, 1]) + B[:, 4] * r[:, 2],
                         (B[:, 2] * r[:, 0] + B[:, 4] * r[:, 1]) + B[:, 5] * r[:, 2]], axis=1)


def block_matrix(B):
    """[n, 6] -> [n, 3, 3]"""
    B = np.asarray(B)
    return np.stack([B[:, [0, 1, 2]], B[:, [1, 3, 4]], B[:, [2, 4, 5]]], axis=1)


# ------------------------------------------------------------------------------------------------ dot, operator, solve
def _tree(s):
    s = s.copy()
    h = 128
    while h:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0]


def dot(a, b):
    """the solver's dot product of two [nv, 3] arrays: float64, in the order of solve_block_sum / solve_scalar_kernel"""
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    with np.errstate(all="ignore"):
        d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        parts = -(-len(d) // 256)
        pad = np.zeros(256 * parts)
        pad[:len(d)] = d
        partial = np.array([_tree(row) for row in pad.reshape(parts, 256)])
        s = np.zeros(256)
        rows = np.zeros(256 * max(1, -(-parts // 256)))
        rows[:parts] = partial
        for row in rows.reshape(-1, 256):
            s = s + row
        return float(_tree(s))


def operator(runs, mass, scale, fixed, dtype=np.float32):
    """x -> q = mass x + scale acc; runs(x) -> the list of (starts, entries, terms [.., 3]) of ref64_terms.gather for the direction x"""
    dt = np.dtype(dtype).type
    m = np.asarray(mass, dtype)
    fx = fixed_mask(m, fixed)

    def multiply(x):
        x = np.asarray(x, dtype)
        rr = runs(x)
        acc = rt.gather(len(m), rr, dtype) if rr else np.zeros((len(m), 3), dtype)
        with np.errstate(all="ignore"):
            q = m[:, None] * x + dt(scale) * acc
        return np.where(fx[:, None], dt(0), q).astype(dtype)
    return multiply


def pcg(multiply, inv, b, x0=None, max_iters=100, tol=np.inf, rel_tol=1e-3, dtype=np.float32):
    """the solve of mesh_solve.hip: dict(x, iters, residuals [iters + 1], flag); inv [nv, 6] or None (no preconditioner: z = r)"""
    dt = np.dtype(dtype).type
    b = np.asarray(b, dtype)
    x = np.zeros_like(b) if x0 is None else np.asarray(x0, dtype).copy()
    prec = (lambda r: r.copy()) if inv is None else (lambda r: apply_block(np.asarray(inv, dtype), r).astype(dtype))
    fmax = float(np.finfo(np.float32).max)
    tol, rel_tol = dt(min(float(tol), fmax)), dt(min(float(rel_tol), fmax))
    out = lambda flag, it, hist: dict(x=x, iters=it, residuals=np.array(hist, dtype), flag=flag)
    with np.errstate(all="ignore"):
        r = b - multiply(x)
        z = prec(r)
        p = z.copy()
        rz = dot(r, z)
        if not (np.isfinite(rz) and rz >= 0):
            return out("not_finite", 0, [])
        res = dt(np.sqrt(rz))
        hist = [res]
        local = min(rel_tol * res, tol)
        if res <= local:
            return out("converged", 0, hist)
        for k in range(max_iters):
            q = multiply(p)
            pq = dot(p, q)
            if not np.isfinite(pq):
                return out("not_finite", k, hist)
            if not pq > 0:
                return out("breakdown", k, hist)
            alpha = dt(rz / pq)
            x = (x + alpha * p).astype(dtype)
            r = (r - alpha * q).astype(dtype)
            z = prec(r)
            rz1 = dot(r, z)
            if not (np.isfinite(rz1) and rz1 >= 0):
                return out("not_finite", k, hist)
            beta = dt(rz1 / rz)
            rz = rz1
            res = dt(np.sqrt(rz))
            hist.append(res)
            if res <= local:
                return out("converged", k + 1, hist)
            p = (z + beta * p).astype(dtype)
        return out("max_iters", max_iters, hist)


# ------------------------------------------------------------------------------------------------ the terms in dtype
def pt_hvp64(p, a, b, c, x, dhat2, kappa):
    """H+ x of (vertex, triangle) pairs in float64: the closed form of ref64_barrier_hessian at the float64 closest point"""
    d2, cp, bary, feat = rm.tri_closest(p, a, b, c)
    _, bp, bpp = rbh.barrier3(d2, dhat2, kappa)
    f1, f2, d1, d2_, r1, r2 = rbh.pt_slots(feat, a, b, c)
    w = np.stack([np.ones_like(bp), -bary[:, 0], -bary[:, 1], -bary[:, 2]], axis=1)
    h, _, _ = rbh.hvp_core(w, p - cp, f1, f2, d1, d2_, r1, r2, x, bp, bpp, True)
    return np.where(((d2 < dhat2) & (d2 > 0))[:, None, None], h, 0.0)


def ee_hvp64(a0, a1, b0, b1, x, dhat2, kappa, eps):
    d2, s, t, cat, _ = rp.ee_closest(a0, a1, b0, b1)
    bb, bp, bpp = rbh.barrier3(d2, dhat2, kappa)
    act = (d2 < dhat2) & (d2 > 0)
    fs, ft = cat // 3 == rp.INTERIOR, cat % 3 == rp.INTERIOR
    u, v = a1 - a0, b1 - b0
    d1, d2_, r1, r2 = rbh.ee_slots(fs, ft, u, b0, b1)
    w = np.stack([1 - s, s, -(1 - t), -t], axis=1)
    r = (a0 + s[:, None] * u) - (b0 + t[:, None] * v)
    hb, gx, _ = rbh.hvp_core(w, r, fs, ft, d1, d2_, r1, r2, x, bp, bpp, True)
    h, _ = rbh.ee_mollified(hb, gx, w, r, u, v, x, np.where(act, bb, 0.0), bp, eps, True)
    return np.where(act[:, None, None], h, 0.0)


class System:
    """A = diag(mass) + scale (H+_elastic + H+_barrier + H_friction) in dtype.  elastic = (mu, lam, kb); barrier = dict(pt [n, 2], ee
    [m, 2], dhat, kappa, rest2 [ne] or None); friction = dict(pt, ee, record [n + m, 8], mu, eps_v); every term optional.  linearize(verts,
    u) sets the point."""

    def __init__(self, rest_verts, tris, mass, scale, elastic=None, barrier=None, friction=None, fixed=None, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.tris = np.asarray(tris, np.int64).reshape(-1, 3)
        self.nv = len(rest_verts)
        self.mass, self.scale, self.fixed = np.asarray(np.asarray(mass, np.float32), dtype), float(np.float32(scale)), fixed
        self.elastic, self.barrier, self.friction = elastic, barrier, friction
        self.edges = rp.edges(self.tris)
        if elastic is not None:
            self.rest = rl.Rest(rest_verts, self.tris, dtype)
        for term in (barrier, friction):
            if term is not None:
                pt = np.asarray(term["pt"] if term["pt"] is not None else np.zeros((0, 2)), np.int64).reshape(-1, 2)
                ee = np.asarray(term["ee"] if term["ee"] is not None else np.zeros((0, 2)), np.int64).reshape(-1, 2)
                term["pt"], term["ee"] = pt, ee
                term["vert"] = np.concatenate([np.concatenate([pt[:, :1], self.tris[pt[:, 1]]], axis=1),
                                               np.concatenate([self.edges[ee[:, 0]], self.edges[ee[:, 1]]], axis=1)]).reshape(-1, 4)
                term["inc"] = rt.incidence(term["vert"], self.nv)

    def linearize(self, verts, u=None):
        self.x = np.asarray(np.asarray(verts, np.float32), self.dtype)
        self.u = None if u is None else np.asarray(np.asarray(u, np.float32), self.dtype)

    # per-element products for corner directions z [n, N, 3] -> [n, N, 3]
    def _tri(self, z):
        mu, lam, _ = self.elastic
        if not (mu > 0 or lam > 0):
            return np.zeros(z.shape, self.dtype)
        return rl.tri_eval(self.rest.tri_record, self.x[self.tris], mu, lam, z, True)["h"]

    def _hinge(self, z):
        kb = self.elastic[2]
        if not kb > 0:
            return np.zeros(z.shape, self.dtype)
        return rl.hinge_eval(self.rest.hinge_record, self.x[self.rest.hinges], kb, z)["h"]

    def _barrier(self, z):
        b = self.barrier
        npt = len(b["pt"])
        p = self.x[b["vert"]]
        dhat2 = rb.dhat2_f32(b["dhat"])
        r2 = b.get("rest2")
        ee = b["ee"]
        if self.dtype == np.float32:
            eps = np.zeros(len(ee), np.float32) if r2 is None else rb.ee_eps32(np.asarray(r2, np.float32)[ee[:, 0]], np.asarray(r2, np.float32)[ee[:, 1]])
            hp = rbh.pt_hvp32(p[:npt, 0], p[:npt, 1], p[:npt, 2], p[:npt, 3], z[:npt], dhat2, b["kappa"], True)[0]
            he = rbh.ee_hvp32(p[npt:, 0], p[npt:, 1], p[npt:, 2], p[npt:, 3], z[npt:], dhat2, b["kappa"], eps, True)[0]
        else:
            r2f = None if r2 is None else np.asarray(np.asarray(r2, np.float32), np.float64)
            eps = np.zeros(len(ee)) if r2 is None else (np.float64(np.float32(1e-2)) * r2f[ee[:, 0]]) * r2f[ee[:, 1]]
            hp = pt_hvp64(p[:npt, 0], p[:npt, 1], p[:npt, 2], p[:npt, 3], z[:npt], dhat2, b["kappa"])
            he = ee_hvp64(p[npt:, 0], p[npt:, 1], p[npt:, 2], p[npt:, 3], z[npt:], dhat2, b["kappa"], eps)
        return np.concatenate([hp, he]).astype(self.dtype)

    def _friction(self, z):
        f = self.friction
        ev = rf.evaluate32 if self.dtype == np.float32 else rf.evaluate64
        return np.asarray(ev(f["record"], self.u[f["vert"]], f["mu"], f["eps_v"], z)["h"], self.dtype)

    def _kinds(self):
        """(per-element product, element vertex lists [n, N], incidence) of every run, in the device's order"""
        out = []
        if self.elastic is not None:
            out += [(self._tri, self.tris, self.rest.tri_inc), (self._hinge, self.rest.hinges, self.rest.hinge_inc)]
        if self.barrier is not None:
            out.append((self._barrier, self.barrier["vert"], self.barrier["inc"]))
        if self.friction is not None:
            out.append((self._friction, self.friction["vert"], self.friction["inc"]))
        return out

    def runs(self, x):
        x = np.asarray(x, self.dtype)
        return [(inc[0], inc[1], fn(x[elems]).reshape(-1, 3)) for fn, elems, inc in self._kinds()]

    def multiply(self, x):
        return operator(self.runs, self.mass, self.scale, self.fixed, self.dtype)(x)

    def term_blocks(self):
        """the per-term blocks the device's way: [elastic, barrier, friction] as [nv, 6] (zeros for an absent term), from every element's
        own corner blocks at unit directions per corner, gathered in run order"""
        def kind_runs(fn, elems, inc):
            n, N = elems.shape
            blk = np.zeros((n, N, 6), self.dtype)
            for c in range(N):
                for j in range(3):
                    z = np.zeros((n, N, 3), self.dtype)
                    z[:, c, j] = 1
                    h = fn(z)
                    for k, (i, jj) in enumerate(SLOT):
                        if jj == j:
                            blk[:, c, k] = h[:, c, i]
            return (inc[0], inc[1], blk.reshape(-1, 6))
        zero = np.zeros((self.nv, 6), self.dtype)
        kinds = self._kinds()
        out, at = [], 0
        for present, count in ((self.elastic, 2), (self.barrier, 1), (self.friction, 1)):
            if present is None:
                out.append(zero.copy())
            else:
                out.append(rt.gather(self.nv, [kind_runs(*k) for k in kinds[at:at + count]], self.dtype))
                at += count
        return out

    def term_blocks_by_products(self, vertices):
        """the definition: entry (i, j) at v = component i at v of the term's product with the unit direction e_{v,j}; [elastic, barrier,
        friction] as [len(vertices), 6]"""
        kinds = self._kinds()
        groups, at = [], 0
        for present, count in ((self.elastic, 2), (self.barrier, 1), (self.friction, 1)):
            groups.append(kinds[at:at + count] if present is not None else [])
            at += count if present is not None else 0
        out = [np.zeros((len(vertices), 6), self.dtype) for _ in groups]
        for row, v in enumerate(vertices):
            for j in range(3):
                x = np.zeros((self.nv, 3), self.dtype)
                x[v, j] = 1
                for g, group in enumerate(groups):
                    if group:
                        hx = rt.gather(self.nv, [(inc[0], inc[1], fn(x[elems]).reshape(-1, 3)) for fn, elems, inc in group], self.dtype)
                        for k, (i, jj) in enumerate(SLOT):
                            if jj == j:
                                out[g][row, k] = hx[v, i]
        return out

    def blocks(self):
        el, ba, fr = self.term_blocks()
        D = combine(el, ba, fr, self.scale, self.mass, self.dtype)
        inv, fallbacks, bad = precondition(D, self.mass, self.fixed, self.dtype)
        return dict(elastic=el, barrier=ba, friction=fr, combined=D, inverse=inv, fallbacks=fallbacks, fixed_masses=bad)

    def dense(self):
        """A [3 nv, 3 nv], column by column"""
        n = 3 * self.nv
        A = np.zeros((n, n), self.dtype)
        for k in range(n):
            e = np.zeros(n, self.dtype)
            e[k] = 1
            A[:, k] = self.multiply(e.reshape(-1, 3)).reshape(-1)
        return A

    def energy(self, verts, u=None):
        """float64: the elastic, barrier and friction energy at verts (friction at the displacement u, records lagged)"""
        x = np.asarray(verts, np.float64)
        e = 0.0
        if self.elastic is not None:
            mu, lam, kb = self.elastic
            R = self.rest if self.dtype == np.float64 else rl.Rest(self.rest.X, self.tris, np.float64)
            e += float(rl.tri_eval(R.tri_record, x[self.tris], mu, lam)["e"].sum()) if mu > 0 or lam > 0 else 0.0
            e += float(rl.hinge_eval(R.hinge_record, x[R.hinges], kb)["e"].sum()) if kb > 0 else 0.0
        if self.barrier is not None:
            b = self.barrier
            npt, p, dhat2 = len(b["pt"]), x[b["vert"]], rb.dhat2_f32(b["dhat"])
            e += float(rb.barrier(rm.tri_closest(p[:npt, 0], p[:npt, 1], p[:npt, 2], p[:npt, 3])[0], dhat2, b["kappa"])[0].sum())
            q = p[npt:]
            d2 = rp.ee_closest(q[:, 0], q[:, 1], q[:, 2], q[:, 3])[0]
            n = rm._cross(q[:, 1] - q[:, 0], q[:, 3] - q[:, 2])
            r2 = b.get("rest2")
            eps = np.zeros(len(q)) if r2 is None else 1e-2 * np.asarray(r2, np.float64)[b["ee"][:, 0]] * np.asarray(r2, np.float64)[b["ee"][:, 1]]
            e += float((rb.mollifier(rm._dot(n, n), eps)[0] * rb.barrier(d2, dhat2, b["kappa"])[0]).sum())
        if self.friction is not None:
            f = self.friction
            uu = np.asarray(u, np.float64)
            e += float(rf.evaluate64(f["record"], uu[f["vert"]], f["mu"], f["eps_v"])["e"].sum())
        return e


# ------------------------------------------------------------------------------------------------ the cases of the tests
# stiffnesses at which the three terms and the mass all count on the scenes of ref64_proximity (coordinates in [0.2, 0.8]): masses of
# DENSITY x vertex area, SCALE = h^2 for h = 0.1
DENSITY, SCALE, MU, LAM, KB, KAPPA, FRICTION_MU, EPS_V = 1e3, 1e-2, 1e3 * rl.MU, 1e3 * rl.LAM, rl.KB, 1e3, 0.3, 1e-3
SMALL = ("tiny2", "sheets5")


def scene(name):
    """(verts, tris, dhat): a scene of ref64_proximity, a strip (dhat = 1.5 spacings), or sheets5 = two 5 x 5-vertex sheets, slightly
    jittered, 2 / 3 dhat apart"""
    if name == "sheets5":
        dhat = 0.03
        v0, t0 = rp.grid_sheet(5, 0.5, 0.05, 1)
        v1, t1 = rp.grid_sheet(5, 0.5 + 2.0 / 3.0 * dhat, 0.05, 2)
        return np.concatenate([v0, v1]), np.concatenate([t0, t1 + len(v0)]).astype(np.int32), dhat
    if name.startswith("strip"):
        return strip(*map(int, name[5:].split("x"))) + (0.006,)
    return rp.scene(name)


def pairs_within(verts, tris, dhat):
    """the (vertex, triangle) and (edge, edge) pairs closer than dhat, brute force in float64 (any list serves a linear system)"""
    pt = rp.pt_candidates(verts, tris, dhat)
    pt = pt[rp.pt_distance(verts, tris, pt)[0] < dhat]
    e = rp.edges(tris)
    ee = rp.ee_candidates(verts, e, dhat)
    return pt, ee[rp.ee_distance(verts, e, ee)[0] < dhat]


def lag32(verts, tris, pt, ee, dhat, kappa, rest2):
    """the friction records [npt + nee, 8] of the float32 replay at verts"""
    v, t, e = np.asarray(verts, np.float32), np.asarray(tris, np.int64).reshape(-1, 3), rp.edges(tris)
    P = v[np.concatenate([pt[:, :1], t[pt[:, 1]]], axis=1).reshape(-1, 4)]
    Q = v[np.concatenate([e[ee[:, 0]], e[ee[:, 1]]], axis=1).reshape(-1, 4)]
    dhat2 = rb.dhat2_f32(dhat)
    eps = rb.ee_eps32(np.asarray(rest2, np.float32)[ee[:, 0]], np.asarray(rest2, np.float32)[ee[:, 1]])
    return np.concatenate([rf.lag_pt32(P[:, 0], P[:, 1], P[:, 2], P[:, 3], dhat2, kappa)[0],
                           rf.lag_ee32(Q[:, 0], Q[:, 1], Q[:, 2], Q[:, 3], dhat2, kappa, eps)[0]])


def lag64(verts, tris, pt, ee, dhat, kappa, rest2):
    """the friction records of the float64 reference at verts: unit normals to float64 rounding"""
    dhat2 = rb.dhat2_f32(dhat)
    return np.concatenate([rf.lag_pt64(verts, tris, pt, dhat2, kappa)["rec"], rf.lag_ee64(verts, rp.edges(tris), ee, dhat2, kappa, rest2)["rec"]])


def small_displacement(nv, seed=5, size=1e-3):
    return (size * np.random.default_rng(seed).standard_normal((nv, 3))).astype(np.float32)


def masses(verts, tris):
    return (DENSITY * rl.Rest(verts, tris, np.float64).vertex_area).astype(np.float32)


def cpu_system(name, dtype=np.float64, terms=("elastic", "barrier", "friction")):
    """a System with all three terms on a scene, linearized at displaced(.., 1e-1) and a small u; pairs and records at the rest positions"""
    v, t, dhat = scene(name)
    pt, ee = pairs_within(v, t, dhat)
    rest2 = rb.rest_len2(v, rp.edges(t)).astype(np.float32)
    S = System(v, t, masses(v, t), SCALE, elastic=(MU, LAM, KB) if "elastic" in terms else None,
               barrier=dict(pt=pt, ee=ee, dhat=dhat, kappa=KAPPA, rest2=rest2) if "barrier" in terms else None,
               friction=dict(pt=pt, ee=ee, record=(lag32 if np.dtype(dtype) == np.float32 else lag64)(v, t, pt, ee, dhat, KAPPA, rest2), mu=FRICTION_MU,
                             eps_v=EPS_V) if "friction" in terms else None,
               dtype=dtype)
    S.linearize(rl.displaced(v, t, 1, 1e-1), small_displacement(len(v)))
    return S
