"""Float64 restatement of the triangle-mesh queries (include/zensim_rocm/distance_device.hpp, mesh_device.hpp, zpc_amd/csrc/mesh.hip),
numpy only: brute force over all triangles, the exact Voronoi-region closest point, the pseudonormal sign (Baerentzen & Aanaes 2005:
face normal, sum of the adjacent face normals on an edge, angle-weighted sum at a vertex) and a per-point bound on the float32 result.

The bound.  The device chain from the inputs (exact float32 numbers, taken over as they are) to the distance is, with
S = the largest |p - vertex| of the triangle (<= d + longest edge) and u = 2^-24:
    differences p - a, b - a, ..         1 rounding each, u S
    cross product / edge dot products    3 roundings on terms of size S^2 (relative: 3 u)
    triple products, n . pa              5 roundings, division by |n|^2 or |e|^2: 1, clamped t, d - t e: 2, squares and their sum: 3
    sqrt                                 1
about 12 roundings one after the other on quantities of relative size S, and the squared distance halves its relative error under the
root only away from zero, so the absolute error of d is at most ~12 u S.  Added to that: the pruning test of the tree walk
(box_distance: 6 roundings on S) can drop a triangle that is nearer by that much, 6 u S; a triangle below the degeneracy threshold
(sin of the angle at a below 3.2e-7 = 5.3 u) is measured to its edges, which lie within 5.3 u x edge <= 6 u S of it; the closest point
a + t e and lattice positions origin + voxel * i are rounded to u M each (M = the largest coordinate), 4 u M with the float32 lattice of
from_mesh against the float64 one here.  Sum: 24 u S + 4 u M, stated as
    b = 32 u (S + M) + 1e-37            (denormal floor: products of differences below 1e-19 underflow)
The constant is not fitted to the GPU: tests/test_mesh_cpu.py replays the same chain in numpy float32 on the CPU and finds it within b.
"""
import numpy as np

U = 2.0 ** -24
K_BOUND = 32.0
VERT_A, VERT_B, VERT_C, EDGE_AB, EDGE_BC, EDGE_CA, FACE = range(7)
DEGENERATE32 = 1e-13


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _segment(p, u, v):
    dt = p.dtype.type
    e, d = v - u, p - u
    ee, de = _dot(e, e), _dot(d, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, de / np.where(ee > 0, ee, dt(1)), dt(0)).astype(p.dtype)
    t = np.clip(t, dt(0), dt(1))
    r = d - t[..., None] * e
    return _dot(r, r), t


def tri_closest(p, a, b, c, degenerate=0.0):
    """squared distance, closest point, barycentrics, feature of points p [n, 3] against triangles a, b, c ([3] or [n, 3]), in the dtype of
    p: float64 with degenerate = 0 is the reference, float32 with DEGENERATE32 replays the device chain operation by operation"""
    dt = p.dtype.type
    a, b, c = (np.broadcast_to(np.asarray(x, p.dtype), p.shape) for x in (a, b, c))
    ab, ac, bc = b - a, c - a, c - b
    n = _cross(ab, ac)
    nn = _dot(n, n)
    face_ok = nn > dt(degenerate) * _dot(ab, ab) * _dot(ac, ac)
    pa, pb = p - a, p - b
    wc, wa, wb = _dot(n, _cross(ab, pa)), _dot(n, _cross(bc, pb)), _dot(n, _cross(pa, ac))
    face = face_ok & (wa >= 0) & (wb >= 0) & (wc >= 0)
    nn1 = np.where(face, nn, dt(1))
    h = _dot(n, pa)
    d2f = h * h / nn1
    b1, b2 = wb / nn1, wc / nn1
    baryf = np.stack([dt(1) - b1 - b2, b1, b2], axis=-1)
    cpf = a + (b1[..., None] * ab + b2[..., None] * ac)
    d0, t0 = _segment(p, a, b)
    d1, t1 = _segment(p, b, c)
    d2, t2 = _segment(p, c, a)
    one, zero = np.ones_like(t0), np.zeros_like(t0)
    s0 = (d0 <= d1) & (d0 <= d2)
    s1 = ~s0 & (d1 <= d2)
    d2e = np.where(s0, d0, np.where(s1, d1, d2))
    barye = np.where(s0[..., None], np.stack([one - t0, t0, zero], -1),
                     np.where(s1[..., None], np.stack([zero, one - t1, t1], -1), np.stack([t2, zero, one - t2], -1)))
    cpe = np.where(s0[..., None], a + t0[..., None] * ab, np.where(s1[..., None], b + t1[..., None] * bc, c + t2[..., None] * (a - c)))

    def feat(t, lo, hi, mid):
        return np.where(t <= 0, lo, np.where(t >= 1, hi, mid))
    fe = np.where(s0, feat(t0, VERT_A, VERT_B, EDGE_AB), np.where(s1, feat(t1, VERT_B, VERT_C, EDGE_BC), feat(t2, VERT_C, VERT_A, EDGE_CA)))
    return (np.where(face, d2f, d2e), np.where(face[..., None], cpf, cpe), np.where(face[..., None], baryf, barye),
            np.where(face, FACE, fe).astype(np.int32))


class Mesh64:
    def __init__(self, verts, tris, vel=None):
        self.v = np.asarray(np.asarray(verts, np.float32), np.float64)   # the float32 numbers the device gets
        self.t = np.asarray(tris, np.int64).reshape(-1, 3)
        self.vel = None if vel is None else np.asarray(np.asarray(vel, np.float32), np.float64)
        a, b, c = (self.v[self.t[:, k]] for k in range(3))
        n = _cross(b - a, c - a)
        l = np.linalg.norm(n, axis=1)
        lab, lac = _dot(b - a, b - a), _dot(c - a, c - a)
        self.zero_area = ~(l * l > DEGENERATE32 * lab * lac)     # the device's rule, in float64
        self.fn = np.where(self.zero_area[:, None], 0.0, n / np.where(self.zero_area, 1.0, l)[:, None])

        def ang(u, w):
            return np.arctan2(np.linalg.norm(_cross(u, w), axis=1), _dot(u, w))
        self.angles = np.where(self.zero_area[:, None], 0.0, np.stack([ang(b - a, c - a), ang(c - b, a - b), ang(a - c, b - c)], axis=1))
        self.vn = np.zeros_like(self.v)
        for k in range(3):
            np.add.at(self.vn, self.t[:, k], self.angles[:, k, None] * self.fn)
        edges = {}
        for ti, tri in enumerate(self.t.tolist()):
            for e in range(3):
                u, w = tri[e], tri[(e + 1) % 3]
                edges.setdefault((min(u, w), max(u, w)), []).append((ti, e, u < w))
        self.en = np.zeros((len(self.t), 3, 3))
        self.stats = dict(boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0, zero_area_triangles=int(self.zero_area.sum()), bad_indices=0)
        for (u, w), lst in edges.items():
            s = sum(self.fn[ti] for ti, _, _ in lst)
            for ti, e, _ in lst:
                self.en[ti, e] = s
            if len(lst) == 1:
                self.stats["boundary_edges"] += 1
            elif len(lst) > 2:
                self.stats["nonmanifold_edges"] += 1
            elif u != w and lst[0][2] == lst[1][2]:
                self.stats["inconsistent_edges"] += 1
        self.longest_edge = float(max(np.linalg.norm(b - a, axis=1).max(), np.linalg.norm(c - b, axis=1).max(),
                                      np.linalg.norm(a - c, axis=1).max())) if len(self.t) else 0.0
        self.M = float(np.abs(self.v).max()) if len(self.v) else 0.0

    def tri_distance(self, p, tri):
        """distance of point i to triangle tri[i]"""
        p = np.asarray(p, np.float64)
        t = self.t[tri]
        return np.sqrt(tri_closest(p, self.v[t[:, 0]], self.v[t[:, 1]], self.v[t[:, 2]])[0])

    def pseudonormal(self, tri, feature):
        t = self.t[tri]
        vert = self.vn[t[np.arange(len(tri)), np.clip(feature, 0, 2)]]
        edge = self.en[tri, np.clip(feature - EDGE_AB, 0, 2)]
        return np.where((feature == FACE)[:, None], self.fn[tri], np.where((feature >= EDGE_AB)[:, None], edge, vert))

    def bound(self, p, d):
        p = np.asarray(p, np.float64)
        return K_BOUND * U * (np.abs(d) + self.longest_edge + np.maximum(np.abs(p).max(axis=-1), self.M)) + 1e-37

    def query(self, p, ambiguity=False):
        """brute force: dict(d, sdf, tri, cp, bary, feature, b[, amb]); equal distances go to the smaller triangle number.  amb: the largest
        distance between the closest point and that of any triangle within 2 b of the minimum (how far a result inside the bound may move
        the closest point)"""
        p = np.asarray(np.asarray(p, np.float32), np.float64)
        n = len(p)
        best = np.full(n, np.inf)
        tri = np.full(n, -1, np.int64)
        cp, bary, feat = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, -1, np.int32)
        for ti, (i0, i1, i2) in enumerate(self.t.tolist()):
            d2, c, w, f = tri_closest(p, self.v[i0], self.v[i1], self.v[i2])
            m = d2 < best
            best[m], tri[m], cp[m], bary[m], feat[m] = d2[m], ti, c[m], w[m], f[m]
        d = np.sqrt(best)
        out = dict(d=d, tri=tri, cp=cp, bary=bary, feature=feat, b=self.bound(p, d))
        if len(self.t):
            s = _dot(p - cp, self.pseudonormal(tri, feat))
            out["sdf"] = np.where(s < 0, -d, d)
            if self.vel is not None:
                out["vel"] = sum(bary[:, k, None] * self.vel[self.t[tri, k]] for k in range(3))
        if ambiguity:
            amb = np.zeros(n)
            for i0, i1, i2 in self.t.tolist():
                d2, c, _, _ = tri_closest(p, self.v[i0], self.v[i1], self.v[i2])
                m = np.sqrt(d2) <= d + 2 * out["b"]
                amb[m] = np.maximum(amb[m], np.linalg.norm(c[m] - cp[m], axis=1))
            out["amb"] = amb
        return out


# ------------------------------------------------------------------------------------------------ test meshes (outward orientation)
def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (i >> d) & 1 else lo)[d] for d in range(3)] for i in range(8)], np.float32)   # vertex i: bit d = upper side of axis d
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]      # -z +z(4..) ... each outward
    t = []
    for a, b, c, d in q:
        t += [(a, b, c), (a, c, d)]
    t = np.array(t, np.int32)
    centre = 0.5 * (lo + hi)
    for i, (a, b, c) in enumerate(t.tolist()):   # orient every triangle outward
        n = np.cross(v[b].astype(np.float64) - v[a], v[c].astype(np.float64) - v[a])
        if np.dot(n, v[[a, b, c]].mean(0) - centre) < 0:
            t[i] = (a, c, b)
    return v, t


def box_sdf(x, lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    q = np.abs(x - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(axis=-1), 0)


def icosphere(level, radius=1.0, centre=(0, 0, 0)):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nt = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    return (np.array(v) * radius + np.asarray(centre, np.float64)).astype(np.float32), np.array(t, np.int32)


def torus(nu, nv, R=0.3, r=0.1, centre=(0, 0, 0)):
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3) + np.asarray(centre)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    t = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            t += [(a, b, c), (a, c, d)]
    return v.astype(np.float32), np.array(t, np.int32)
