"""Float64 restatement of the sparse level-set collider with a per-point error bound, in the manner of tests/ref64.py.

What is restated (from the reference's geometry/SparseGrid.hpp:520-545 and geometry/Collider.h:80-110, no text of theirs):

    getSignedDistance(x)   linear-kernel sample of "sdf" over the 2^3 cells around X = (x - origin) / h; a cell of an absent block
                           contributes the background value (the kernels return eight EQUAL values as that value, which is the exact
                           sum; the restatement needs no such rule)
    getNormal(x)           diff_i = (sdf(x + eps e_i) - sdf(x - eps e_i)) / (eps + eps), eps = h / 4, then diff / |diff|
    getMaterialVelocity(x) the same sample of the three "v" channels (background for absent cells), or 0 without "v"
    resolveCollision(x, v) X = R^T (x - b) / s; inside when sdf(X) < 0; v_object = omega x (x - b) + (s'/s)(x - b) + R s v_m(X) + b';
                           Sticky: v = v_object; else v -= v_object, n = R normal(X), proj = n . v, Slip (or Separate and proj < 0):
                           v -= proj n; v += v_object

Discrete decisions and inputs.  Everything up to the local position t = X - floor(X) of a sample is a short chain of IEEE float32
operations without contraction (the kernels' translation units are built with it off): x - b, the three-term rows of R^T, the product
with fl(1 / s), x +- eps, (x - origin) / h, floor and the subtraction.  numpy's float32 performs the same operations with the same
roundings, so the chain is REPRODUCED, not approximated (as ref64.py reproduces the transfers' arena), and the float32 t of every
sample is an exact input.  From there on the answer is exact arithmetic and every point is checked against its own bound:

    sample    sum over 8 cells of ((w0 w1) w2) value, w = (1 - t, t): 1 - t rounds once, two products, the product with the value
              (<= 6 u per term), 7 additions:                                        b_s = 13 u T,  T = sum |w value|
    diff_i    (s1 - s2) / (2 eps): the subtraction and the division round once each, 2 eps = h / 2 is exact:
                                                                                     b_d = (b_s1 + b_s2) / (2 eps) + 2 u |diff_i|
    normal    l = sqrt(sum diff^2): three squares, two additions, the root (<= 4 u l) plus sum |diff_j| b_dj / l;
              n_i = diff_i / l:                                                      b_n = b_di / l + |n_i| b_l / l + u |n_i|
              (first order in b / l: meaningful where the gradient is not small; the callers look at |diff| >= 0.5 only)
    v_object  every path from an input to a component crosses <= 8 roundings (1 / s, s'/s, the products, R s, (R s) v_m, the
              additions):                                                            b_vo = 8 u M + sum_j |R_dj s| b_vm_j
              M = the sum of the magnitudes of the terms
    response  w = v - v_object (u |w| + b_vo); n = R nm (3 u sum |R_dj nm_j| + sum |R_dj| b_nm_j); proj = n . w (3 u sum |n_d w_d| +
              sum (|n_d| b_w_d + |w_d| b_n_d)); v = w - proj n (2 u (|w_d| + |proj n_d|) + b_w_d + |n_d| b_proj + |proj| b_n_d);
              v += v_object (u |v| + b_vo).  Separate with |proj| <= b_proj: the other branch differs by proj n, which is added.

plus 2^-126 per value for denormals.  numpy only.
"""
import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
C_SAMPLE = 13
f32 = np.float32


class LevelSet64:
    """the cells of a sparse level set (keys [nb, 3] block origins, cells [nb * 512, C]: zpc_amd.levelset.select_blocks) as a lookup
    with the background outside the stored blocks; channel 0 = sdf, 1..3 = v"""

    def __init__(self, keys, cells, origin, h, background):
        self.origin, self.h, self.background = np.asarray(origin, f32), f32(h), f32(background)
        self.nch = cells.shape[1]
        keys = np.asarray(keys, np.int64).reshape(-1, 3)
        self.lo = keys.min(0) if len(keys) else np.zeros(3, np.int64)
        hi = keys.max(0) + 8 if len(keys) else np.zeros(3, np.int64) + 8
        self.dense = np.full(tuple(hi - self.lo) + (self.nch,), np.float64(self.background))
        tiles = np.asarray(cells, np.float64).reshape(-1, 8, 8, 8, self.nch)
        for k, t in zip(keys, tiles):
            o = k - self.lo
            self.dense[o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8] = t

    def value(self, idx):
        """[n, 3] integer cell coordinates -> [n, C] float64 values"""
        rel = idx - self.lo
        ok = ((rel >= 0) & (rel < np.array(self.dense.shape[:3]))).all(1)
        out = np.full((idx.shape[0], self.nch), np.float64(self.background))
        r = rel[ok]
        out[ok] = self.dense[r[:, 0], r[:, 1], r[:, 2]]
        return out

    def sample(self, x):
        """x [n, 3] float32 (level-set world space) -> (value [n, C], bound [n, C]) from the reproduced float32 local positions"""
        x = np.asarray(x, f32)
        X = (x - self.origin) / self.h                 # float32, one subtraction and one division per axis
        fl = np.floor(X)
        t = (X - fl).astype(f32)                       # float32 subtraction, as the kernel's
        base = fl.astype(np.int64)
        t = t.astype(np.float64)
        w = np.stack([1.0 - t, t], axis=-1)            # [n, 3, 2], exact from the float32 t
        val = np.zeros((x.shape[0], self.nch))
        T = np.zeros((x.shape[0], self.nch))
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    wt = (w[:, 0, i] * w[:, 1, j] * w[:, 2, k])[:, None]
                    c = self.value(base + np.array([i, j, k]))
                    val += wt * c
                    T += np.abs(wt * c)
        return val, C_SAMPLE * U * T + FLT_MIN

    def sdf(self, x):
        v, b = self.sample(x)
        return v[:, 0], b[:, 0]

    def velocity(self, x):
        if self.nch < 4:
            z = np.zeros((np.asarray(x).shape[0], 3))
            return z, z.copy()
        v, b = self.sample(x)
        return v[:, 1:4], b[:, 1:4]

    def normal(self, x):
        """(normal [n, 3], bound [n, 3], gradient length [n])"""
        x = np.asarray(x, f32)
        eps = f32(self.h / f32(4))
        d = np.zeros((x.shape[0], 3))
        bd = np.zeros((x.shape[0], 3))
        for i in range(3):
            v1, v2 = x.copy(), x.copy()
            v1[:, i] = x[:, i] + eps                   # float32
            v2[:, i] = x[:, i] - eps
            s1, b1 = self.sdf(v1)
            s2, b2 = self.sdf(v2)
            two = float(eps) * 2
            d[:, i] = (s1 - s2) / two
            bd[:, i] = (b1 + b2) / two + 2 * U * np.abs(d[:, i]) + FLT_MIN
        l = np.sqrt((d ** 2).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            n = d / l[:, None]
            bl = (np.abs(d) * bd).sum(1) / l + 4 * U * l
            bn = bd / l[:, None] + np.abs(n) * (bl / l)[:, None] + U * np.abs(n) + FLT_MIN
        return n, bn, l


def to_material32(col, x):
    """(x - b, X) of ColliderDev::to_material in float32, operation by operation"""
    x = np.asarray(x, f32)
    b, R = np.array(col.b[:], f32), np.array(col.R[:], f32)
    one_over_s = f32(1) / f32(col.s)
    xmb = x - b
    X = np.stack([((R[d] * xmb[:, 0] + R[3 + d] * xmb[:, 1]) + R[6 + d] * xmb[:, 2]) * one_over_s for d in range(3)], axis=1)
    return xmb.astype(f32), X.astype(f32)


def resolve64(col, ls, x, v):
    """Collider<LevelSet>::resolveCollision on float32 points x and velocities v.  Returns (inside [n] bool from the float64 sdf,
    sdf [n], b_sdf [n], v_out [n, 3] float64 (the input where not inside), b_v [n, 3], gradient length [n] of the inside points of a Slip /
    Separate collider, NaN elsewhere)."""
    x, v = np.asarray(x, f32), np.asarray(v, f32)
    xmb32, X = to_material32(col, x)
    sd, bsd = ls.sdf(X)
    inside = sd < 0
    out, bout, grad = v.astype(np.float64).copy(), np.zeros(v.shape), np.full(x.shape[0], np.nan)
    if not inside.any():
        return inside, sd, bsd, out, bout, grad
    X, v = X[inside], v[inside]                      # the response is evaluated at the inside points only
    xmb = xmb32[inside].astype(np.float64)
    R = np.array(col.R[:], np.float64).reshape(3, 3)
    s, dsdt = float(col.s), float(col.dsdt)
    om, dbdt = np.array(col.omega[:], np.float64), np.array(col.dbdt[:], np.float64)
    k = dsdt / s
    vm, bvm = ls.velocity(X)
    cross = np.cross(om[None, :], xmb)
    crossM = np.abs(om[[1, 2, 0]] * xmb[:, [2, 0, 1]]) + np.abs(om[[2, 0, 1]] * xmb[:, [1, 2, 0]])
    u = vm @ (R * s).T
    vo = cross + k * xmb + u + dbdt
    M = crossM + np.abs(k * xmb) + np.abs(vm) @ np.abs(R * s).T + np.abs(dbdt)
    bvo = 8 * U * M + bvm @ np.abs(R * s).T + FLT_MIN
    if col.type == 0:
        res, bres = vo, bvo
    else:
        nm, bnm, l = ls.normal(X)
        grad[inside] = l
        w = v.astype(np.float64) - vo
        bw = U * np.abs(w) + bvo
        n = nm @ R.T
        bn = 3 * U * (np.abs(nm) @ np.abs(R).T) + bnm @ np.abs(R).T
        proj = (n * w).sum(1)
        bp = 3 * U * np.abs(n * w).sum(1) + (np.abs(n) * bw + np.abs(w) * bn).sum(1)
        take = np.ones_like(proj, bool) if col.type == 1 else proj < 0
        p = np.where(take, proj, 0.0)[:, None]
        v1 = w - p * n
        bv1 = np.where(take[:, None], 2 * U * (np.abs(w) + np.abs(p * n)) + bw + np.abs(n) * bp[:, None] + np.abs(p) * bn, bw)
        if col.type == 2:   # a projection the rounding decides: the other branch differs by proj n
            amb = np.abs(proj) <= bp
            bv1 = bv1 + np.where(amb[:, None], (np.abs(proj) + bp)[:, None] * (np.abs(n) + bn), 0.0)
        res = v1 + vo
        bres = U * np.abs(res) + bv1 + bvo + FLT_MIN
    out[inside] = res
    bout[inside] = bres
    return inside, sd, bsd, out, bout, grad
