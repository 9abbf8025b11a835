"""Float64 restatement of the transition between two sparse level sets (TransitionLevelSetView, include/zensim_rocm/levelset_device.hpp)
with a per-point error bound, built on tests/ref64_levelset.py.

What is restated (from the reference's geometry/LevelSet.h, no text of theirs): with two level sets src and dst, a keyframe spacing
stepDt and a phase alpha,

    v  = (src.getMaterialVelocity(x) + dst.getMaterialVelocity(x)) * 0.5          (a level set without "v" gives 0)
    x0 = x - (alpha * stepDt) * v           x1 = x + ((1 - alpha) * stepDt) * v
    call(x) = (1 - alpha) * src.call(x0) + alpha * dst.call(x1)                   for getSignedDistance, getNormal, getMaterialVelocity

Reproduced part.  Everything up to x0 and x1 is a chain of IEEE float32 operations in the order the header documents, without
contraction: the two velocity samples ((x - origin) / h, floor, t = X - floor, the weights 1 - t and t, the eight terms
((w0 w1) w2) value added in the order first axis slowest starting from 0, and eight EQUAL values giving that value), their sum, the
product with 0.5, the two scalar products alpha * stepDt and (1 - alpha) * stepDt, their products with v, the subtraction and the
addition.  numpy's float32 performs the same operations with the same roundings, so x0 and x1 are exact inputs of what follows, as the
local positions are in ref64_levelset.py.  (Should a device ever not reproduce the chain bit for bit, no constant below is to be
loosened: each bound gets a position term instead, the position error times the largest cell-to-cell difference of the stencil
divided by h.  The chain has been reproducible so far and the term is not present.)

Bounds.  The two level sets' answers at x0 and x1 come from LevelSet64 with their own bounds b0 and b1.  The weights are the float32
numbers w0 = fl(1 - alpha) and w1 = alpha, exact inputs.  The device forms fl(fl(w0 a0) + fl(w1 a1)) from its own a0, a1 within b0, b1
of the exact ones: the products round once each (u |w a|), the sum once (u |result| <= u (|w0 a0| + |w1 a1|)), so to first order the
error is below w0 b0 + w1 b1 + 2 u (|w0 a0| + |w1 a1|); the restatement takes 3 u for the second-order terms (b u, u^2), which are
smaller than u (|w0 a0| + |w1 a1|) by the factor b / |a| + u << 1 wherever a bound means anything:

    blend     b = |w0| b0 + |w1| b1 + 3 u (|w0 a0| + |w1 a1|) + 2^-126

for the distance, every component of the normal and every component of the velocity.  The gradient length reported for a normal is
the smaller of the two level sets' (the callers leave points below 0.5 out of the normal checks, as ref64_levelset.py's do).
Transition64 has the interface resolve64 asks of a level set (sdf, velocity, normal), so the collider response and its bounds are
ref64_levelset.resolve64's with the blended quantities.  numpy only.
"""
import numpy as np

from ref64_levelset import U, FLT_MIN, LevelSet64

f32 = np.float32
C_BLEND = 3


def velocity32(ls, x):
    """LevelSetView::getMaterialVelocity in float32, operation by operation: x [n, 3] float32 -> [n, 3] float32 (0 without "v")"""
    x = np.asarray(x, f32)
    if ls.nch < 4:
        return np.zeros(x.shape, f32)
    X = (x - ls.origin) / ls.h
    fl = np.floor(X)
    t = (X - fl).astype(f32)
    base = fl.astype(np.int64)
    w = np.stack([f32(1) - t, t], axis=-1).astype(f32)            # [n, 3, 2]
    vals = [ls.value(base + np.array([o >> 2, (o >> 1) & 1, o & 1]))[:, 1:4].astype(f32) for o in range(8)]   # the cells are float32 values
    same = np.ones(x.shape, bool)
    total = np.zeros(x.shape, f32)
    for o in range(8):
        wt = ((w[:, 0, o >> 2] * w[:, 1, (o >> 1) & 1]) * w[:, 2, o & 1]).astype(f32)
        total = (total + (wt[:, None] * vals[o]).astype(f32)).astype(f32)
        same &= vals[o] == vals[0]
    return np.where(same, vals[0], total).astype(f32)


class Transition64:
    """the blend of LevelSet64 src and dst; sdf / velocity / normal at float32 points of level-set world space, as LevelSet64's"""

    def __init__(self, src, dst, step_dt, alpha):
        self.src, self.dst = src, dst
        self.step_dt, self.alpha = f32(step_dt), f32(alpha)
        self.w0, self.w1 = float(f32(1) - self.alpha), float(self.alpha)
        self.has_velocity = src.nch >= 4 or dst.nch >= 4

    def displaced32(self, x):
        """(x0, x1) float32, the documented chain"""
        x = np.asarray(x, f32)
        v = ((velocity32(self.src, x) + velocity32(self.dst, x)).astype(f32) * f32(0.5)).astype(f32)
        a0 = f32(self.alpha * self.step_dt)
        a1 = f32(f32(f32(1) - self.alpha) * self.step_dt)
        x0 = (x - (a0 * v).astype(f32)).astype(f32)
        x1 = (x + (a1 * v).astype(f32)).astype(f32)
        return x0, x1

    def _blend(self, a0, b0, a1, b1):
        t0, t1 = self.w0 * a0, self.w1 * a1
        return t0 + t1, abs(self.w0) * b0 + abs(self.w1) * b1 + C_BLEND * U * (np.abs(t0) + np.abs(t1)) + FLT_MIN

    def sdf(self, x):
        x0, x1 = self.displaced32(x)
        return self._blend(*self.src.sdf(x0), *self.dst.sdf(x1))

    def velocity(self, x):
        x0, x1 = self.displaced32(x)
        return self._blend(*self.src.velocity(x0), *self.dst.velocity(x1))

    def normal(self, x):
        """(blended normal [n, 3], bound [n, 3], the smaller of the two gradient lengths [n])"""
        x0, x1 = self.displaced32(x)
        n0, b0, l0 = self.src.normal(x0)
        n1, b1, l1 = self.dst.normal(x1)
        n, b = self._blend(n0, b0, n1, b1)
        return n, b, np.minimum(l0, l1)

    def sample_positions(self, x):
        """every float32 position either level set is sampled at for a point x: [(level set, positions)], for the input conditions"""
        x = np.asarray(x, f32)
        x0, x1 = self.displaced32(x)
        out = [(self.src, x), (self.dst, x), (self.src, x0), (self.dst, x1)]
        for ls, p in ((self.src, x0), (self.dst, x1)):
            eps = f32(ls.h / f32(4))
            for i in range(3):
                for sgn in (1, -1):
                    q = p.copy()
                    q[:, i] = p[:, i] + f32(sgn) * eps
                    out.append((ls, q))
        return out


def touches_absent(ls, keys, x):
    """[n] bool: one of the 2^3 cells of the sample of `ls` (block origins `keys`) at x lies in a block that is not stored"""
    x = np.asarray(x, f32)
    base = np.floor((x - ls.origin) / ls.h).astype(np.int64)
    stored = {tuple(k) for k in np.asarray(keys, np.int64).tolist()}
    bad = np.zeros(x.shape[0], bool)
    for o in np.ndindex(2, 2, 2):
        blk = (base + np.array(o)) // 8 * 8
        bad |= ~np.fromiter((tuple(k) in stored for k in blk.tolist()), bool, x.shape[0])
    return bad


# ------------------------------------------------------------------------------------------------ the test case of the issue
VOXEL = 1.0 / 64
RADIUS, BAND = 0.2, 6 * VOXEL
CENTRE0 = np.array([0.5, 0.47, 0.53])
DIRECTION = np.array([0.6, -0.48, 0.64])          # unit length, no axis
SHIFT = 1.5 * VOXEL * DIRECTION                    # src centre -> dst centre
STEP_DT = 0.01
ALPHAS = (0.0, 0.25, 0.5, 0.96875)
NPOINTS = 4096


def sphere_cells(centre, vel=None, lo=(0.1, 0.1, 0.1), hi=(0.9, 0.9, 0.9), voxel=VOXEL, radius=RADIUS, band=BAND):
    """(keys, cells, origin float32) of the sphere's distance sampled on the lattice lo + voxel * (i, j, k), background = band; vel: a
    uniform material velocity [3] or None"""
    from zpc_amd.levelset import select_blocks
    lo = np.asarray(lo, np.float64)
    n = [int(np.ceil((h - l) / voxel)) + 1 for l, h in zip(lo, hi)]
    x = lo + voxel * np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), axis=-1)
    sdf = (np.linalg.norm(x - centre, axis=-1) - radius).astype(f32)
    v = None if vel is None else np.broadcast_to(np.asarray(vel, f32), sdf.shape + (3,))
    keys, cells = select_blocks(sdf, band, band, v)
    return keys, cells, lo.astype(f32)


def keyframes(vel_src=True, vel_dst=True):
    """the two keyframes: [(keys, cells, origin)] of spheres at CENTRE0 and CENTRE0 + SHIFT with the uniform "v" = SHIFT / STEP_DT"""
    v = SHIFT / STEP_DT
    return [sphere_cells(CENTRE0, v if vel_src else None), sphere_cells(CENTRE0 + SHIFT, v if vel_dst else None)]


def reference(frames, alpha, step_dt=STEP_DT):
    (k0, c0, o0), (k1, c1, o1) = frames
    return Transition64(LevelSet64(k0, c0, o0, VOXEL, BAND), LevelSet64(k1, c1, o1, VOXEL, BAND), step_dt, alpha)


def material_points(alpha, seed=0, n=NPOINTS):
    """n float64 points of material space within 2 voxels of the sphere around the interpolated centre CENTRE0 + alpha SHIFT"""
    g = np.random.default_rng(1000 + seed)
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = RADIUS + (g.random(n) * 4 - 2) * VOXEL
    return CENTRE0 + alpha * SHIFT + d * r[:, None]
