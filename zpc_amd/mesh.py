"""Triangle meshes as colliders: TriMesh owns a device mesh object of the library (LBvh over the triangle boxes, face normals, vertex and
edge pseudonormals) and answers closest-point and signed-distance queries and the proximity pairs of the mesh with itself (vertex-triangle and edge-edge within a
contact distance), the IPC barrier potential with its gradient and Hessian-vector product on those pairs, the largest step along a
direction that keeps them apart (max_step, step_candidates) and the mesh's own membrane and bending energy against a rest shape
(set_rest_shape, elastic, elastic_hessian_product); SparseLevelSet.from_mesh (zpc_amd/levelset.py) turns one
into a sparse level set, MeshSystem (zpc_amd/mesh_solve.py) puts the three Hessian products behind one linear system and solves it.  Set-up code: torch for the plumbing; every query runs in the library's HIP kernels."""
import ctypes as C

import numpy as np

from ._lib import lib, MeshView

FEATURES = ("vertex a", "vertex b", "vertex c", "edge ab", "edge bc", "edge ca", "face")
# ee_category = uCate * 3 + vCate of the closest points a0 + s (a1 - a0), b0 + t (b1 - b0) of two edges
EE_CATEGORIES = ("a0 - b0", "a0 - b1", "a0 - edge b", "a1 - b0", "a1 - b1", "a1 - edge b", "edge a - b0", "edge a - b1", "edge a - edge b")
STAT_NAMES = ("boundary_edges", "nonmanifold_edges", "inconsistent_edges", "zero_area_triangles", "bad_indices")
FLT_MAX = float(np.finfo(np.float32).max)


def default_origin(box_lo, voxel, band):
    """origin of from_mesh: the mesh's total box minus band, snapped down to a multiple of voxel (host logic, no device needed)"""
    lo = np.asarray(box_lo, np.float64) - float(band)
    return tuple(float(v) for v in np.floor(lo / float(voxel)) * float(voxel))


def candidate_capacity(pairs, box_lo, box_hi, origin, voxel, band):
    """upper bound for the candidate blocks of from_mesh: the (triangle, block) pairs, or the blocks under the mesh's total box dilated by
    band and one cell, whichever is smaller (host logic)"""
    lo = np.floor((np.asarray(box_lo, np.float64) - np.asarray(origin, np.float64) - band) / voxel) - 2
    hi = np.ceil((np.asarray(box_hi, np.float64) - np.asarray(origin, np.float64) + band) / voxel) + 2
    nb = np.floor(hi / 8) - np.floor(lo / 8) + 1
    return int(max(1, min(float(pairs), float(np.prod(nb)))))


def proximity_grey(r, box_lo, box_hi):
    """upper bound for the grey zone of the float32 proximity test at radius r on a mesh inside the box: a pair is listed when its float32
    distance is below r, and that distance is off by at most 64 u (S + M), u = 2^-24, S = distance + the lengths of two edges (at most
    the box diagonal each), M = the largest coordinate (the derivation is with the distance code; 64 is the edge-edge constant, the
    point-triangle one is 32).  Host logic."""
    lo, hi = np.asarray(box_lo, np.float64), np.asarray(box_hi, np.float64)
    diag = float(np.linalg.norm(hi - lo)) if lo.size else 0.0
    big = float(max(np.abs(lo).max(), np.abs(hi).max())) if lo.size else 0.0
    return 2.0 ** -18 * (float(r) + 2.0 * diag + big) + 1e-37


def candidate_radius(max_norm, t_max, margin, box_lo, box_hi):
    """radius of TriMesh.step_candidates: 2 t_max max|direction| + margin plus the grey zone of the proximity test at that radius, as a
    float32 number rounded up.  max_norm is the largest float32 row norm (4 roundings below the exact one at most: raised by 8 u).  With
    margin=None the margin is the grey zone once more.  Host logic, float64."""
    reach = 2.0 * float(t_max) * float(max_norm) * (1.0 + 2.0 ** -21)
    # the grey zone g at the radius it leads to: g = c (reach + margin + g + ..), c = 2^-18, so at most 1 / (1 - 2 c) of the zone without it
    grey = proximity_grey(reach + (0.0 if margin is None else float(margin)), box_lo, box_hi) * (1.0 + 2.0 ** -16)
    r = reach + (grey if margin is None else float(margin)) + grey
    r32 = np.float32(r)
    if float(r32) < r:
        r32 = np.nextafter(r32, np.float32(np.inf))
    return float(r32)


def _dev_f32(a, cols):
    import torch
    t = a if hasattr(a, "detach") else torch.from_numpy(np.ascontiguousarray(a, np.float32))
    t = t.to(device="cuda", dtype=torch.float32).contiguous()
    if t.ndim != 2 or t.shape[1] != cols:
        raise ValueError("expected an [n, %d] array" % cols)
    return t


def _ptr(t):
    return None if t is None else t.data_ptr()


def _positive_f32(who, name, x):
    """x as a float: finite, positive and still both as a float32"""
    x = float(x)
    if not (np.isfinite(x) and x > 0 and np.float32(x) > 0 and np.isfinite(np.float32(x))):
        raise ValueError("TriMesh.%s: %s must be finite and positive" % (who, name))
    return x


def _pair_lists(prox):
    """the contiguous PT and EE lists of a Proximity (None for a side it does not have) and their counts"""
    pt = None if prox.pt_pairs is None else prox.pt_pairs.contiguous()
    ee = None if prox.ee_pairs is None else prox.ee_pairs.contiguous()
    return pt, ee, (0 if pt is None else len(pt)), (0 if ee is None else len(ee))


class _ProximityState:
    """room on a Proximity for what the library keeps with it (the incidence of TriMesh.barrier), next to its public fields"""


class Proximity(_ProximityState):
    """result of TriMesh.proximity: device tensors, None for a side that was not asked for.  pt_pairs [n, 2] (vertex, triangle), pt_dist2 [n],
    pt_feature [n] (FEATURES), pt_bary [n, 3]; ee_pairs [m, 2] (edge i < edge j, rows of TriMesh.edges()), ee_dist2 [m], ee_category [m]
    (EE_CATEGORIES), ee_st [m, 2] (the parameters of the closest points on edge i and edge j)"""
    __slots__ = ("pt_pairs", "pt_dist2", "pt_feature", "pt_bary", "ee_pairs", "ee_dist2", "ee_category", "ee_st")

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)
        self._incidence = None      # (starts, entries, scratch size) of TriMesh.barrier, built by its first gradient call


class Barrier:
    """result of TriMesh.barrier: energy (float64 device scalar: PT then EE, summed in a fixed order), pt_energy [npt], ee_energy [nee]
    (None for a side the Proximity does not have), grad [nv, 3] or None, zero_distance = (PT, EE) pairs at zero distance (their energy is
    +inf and they add nothing to the gradient)"""
    __slots__ = ("energy", "pt_energy", "ee_energy", "grad", "zero_distance")


class BarrierHessianProduct:
    """result of TriMesh.barrier_hessian_product: hx [nv, 3] float32 = H x, pair_terms [npt + nee, 4, 3] float32 (the contributions
    (H_pair x) on each pair's four corners, PT pairs first: the scratch of the call), zero_distance = (PT, EE) pairs that contribute
    nothing because their distance is zero"""
    __slots__ = ("hx", "pair_terms", "zero_distance")


class FrictionLag:
    """result of TriMesh.friction_lag: record [npt + nee, 8] float32 on the device, PT pairs first, one row per pair of prox; normal
    [.., 3] (the unit vector between the closest points), lam [..] (the size of the contact force, m (-b') 2 d) and weights [.., 4] (of
    the relative displacement; they sum to zero) are views of it.  An inactive pair has an all-zero row.  zero_distance = (PT, EE)
    pairs at zero distance (or with a lam beyond the float range): their row is zero as well.  prox is the Proximity the rows belong to;
    its incidence is shared with the barrier calls."""
    __slots__ = ("record", "zero_distance", "prox", "npt", "nee")

    @property
    def normal(self):
        return self.record[:, 0:3]

    @property
    def lam(self):
        return self.record[:, 3]

    @property
    def weights(self):
        return self.record[:, 4:8]


class Friction:
    """result of TriMesh.friction: energy (float64 device scalar: PT then EE, summed in a fixed order), pt_energy [npt], ee_energy [nee]
    (None for a side the Proximity does not have), grad [nv, 3] or None, overflow = (PT, EE) pairs whose tangential displacement or result
    leaves the float range (they contribute exactly zero)"""
    __slots__ = ("energy", "pt_energy", "ee_energy", "grad", "overflow")


class FrictionHessianProduct:
    """result of TriMesh.friction_hessian_product: hx [nv, 3] float32 = H x, pair_terms [npt + nee, 4, 3] float32 (the contributions
    (H_pair x) on each pair's four corners, PT pairs first: the scratch of the call), overflow as for Friction"""
    __slots__ = ("hx", "pair_terms", "overflow")


class _ElementTerms:
    """the scratch of an elastic call, elem_terms [9 nt + 12 nh] float32, as its two parts"""
    __slots__ = ()

    @property
    def tri_terms(self):
        return None if self.elem_terms is None else self.elem_terms[:9 * self.nt].view(self.nt, 3, 3)

    @property
    def hinge_terms(self):
        return None if self.elem_terms is None else self.elem_terms[9 * self.nt:].view((self.elem_terms.numel() - 9 * self.nt) // 12, 4, 3)


class Elastic(_ElementTerms):
    """result of TriMesh.elastic: energy (float64 device scalar: triangles then hinges, summed in a fixed order), tri_energy [nt],
    hinge_energy [nh], grad [nv, 3] or None, elem_terms (the scratch of a gradient call: the gradient terms on each triangle's three
    corners, then on each hinge's four; tri_terms [nt, 3, 3] and hinge_terms [nh, 4, 3] are views of it; None without the gradient),
    overflow = (triangles, hinges) whose energy or gradient leaves the float range (they contribute exactly zero)"""
    __slots__ = ("energy", "tri_energy", "hinge_energy", "grad", "elem_terms", "overflow", "nt")


class ElasticHessianProduct(_ElementTerms):
    """result of TriMesh.elastic_hessian_product: hx [nv, 3] float32 = H x, elem_terms [9 nt + 12 nh] float32 (the scratch of the call: the
    contributions (H_element x) on each triangle's three corners, then on each hinge's four; tri_terms [nt, 3, 3] and hinge_terms
    [nh, 4, 3] are views of it), overflow as for Elastic"""
    __slots__ = ("hx", "elem_terms", "overflow", "nt")


class StepBound:
    """result of TriMesh.max_step: t (float32 device scalar: the largest step every pair allows, at most t_max), pt_toi [npt], ee_toi [nee]
    (the per-pair bounds, None for a side the Proximity does not have), zero_distance = (PT, EE) pairs that start at zero distance (their
    bound is 0), capped = (PT, EE) pairs stopped by max_iter (their bound is valid, not tight)"""
    __slots__ = ("t", "pt_toi", "ee_toi", "zero_distance", "capped")


class TriMesh:
    """TriMesh(pol, verts [nv, 3] f32, tris [nt, 3] i32, vel=None [nv, 3] f32): arrays on the host or the device; the object keeps copies."""

    def __init__(self, pol, verts, tris, vel=None):
        import torch
        self.pol = pol
        v = _dev_f32(verts, 3)
        t = tris if hasattr(tris, "detach") else torch.from_numpy(np.ascontiguousarray(tris, np.int32).reshape(-1, 3))
        t = t.to(device="cuda", dtype=torch.int32).contiguous()
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("tris: [nt, 3]")
        w = None if vel is None else _dev_f32(vel, 3)
        if w is not None and w.shape != v.shape:
            raise ValueError("vel: [nv, 3]")
        self.nv, self.nt = int(v.shape[0]), int(t.shape[0])
        self.has_velocity = w is not None
        self._h = lib().zs_rocm_mesh_create(pol.handle, v.data_ptr(), self.nv, t.data_ptr(), self.nt, None if w is None else w.data_ptr())
        if not self._h:
            raise ValueError("TriMesh: triangles without vertices, or too many of either")
        pol.syncCtx()   # the inputs are copied by now
        if self.stats()["bad_indices"]:
            raise ValueError("TriMesh: vertex indices outside [0, %d)" % self.nv)

    def __del__(self):
        try:
            lib().zs_rocm_mesh_destroy(self._h)
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def view(self):
        v = MeshView()
        lib().zs_rocm_mesh_get_view(self._h, C.byref(v))
        return v

    def stats(self):
        out = (C.c_int * 8)()
        lib().zs_rocm_mesh_stats(self.pol.handle, self._h, out)
        return {k: int(out[i]) for i, k in enumerate(STAT_NAMES)}

    def is_closed(self):
        """closed and consistently oriented: what the pseudonormal sign needs"""
        s = self.stats()
        return self.nt > 0 and not (s["boundary_edges"] or s["nonmanifold_edges"] or s["inconsistent_edges"])

    def total_box(self):
        box = (C.c_float * 6)()
        if lib().zs_rocm_mesh_total_box(self.pol.handle, self._h, box) != 0:
            raise ValueError("TriMesh.total_box: a mesh without triangles")
        return np.array(box[:3], np.float32), np.array(box[3:], np.float32)

    def refit(self, verts, vel=None):
        """new vertex positions (and velocities) on the same topology: refits the tree and recomputes the normals"""
        v = _dev_f32(verts, 3)
        w = None if vel is None else _dev_f32(vel, 3)
        if v.shape[0] != self.nv or (w is not None and w.shape[0] != self.nv):
            raise ValueError("TriMesh.refit: the topology is kept, so the vertex count must not change")
        if lib().zs_rocm_mesh_refit(self.pol.handle, self._h, v.data_ptr(), None if w is None else w.data_ptr()) != 0:
            raise RuntimeError("zs_rocm_mesh_refit failed")
        self.pol.syncCtx()
        self.has_velocity = self.has_velocity or w is not None

    @property
    def num_edges(self):
        return int(lib().zs_rocm_mesh_num_edges(self._h))

    def edges(self):
        """the unique edges [ne, 2] int32 on the device, e[0] < e[1], in lexicographic order"""
        import torch
        e = torch.empty(self.num_edges, 2, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_edges(self.pol.handle, self._h, e.data_ptr()) != 0:
            raise RuntimeError("zs_rocm_mesh_edges failed")
        self.pol.syncCtx()
        return e

    def _pairs(self, n, count, fill, dhat, widths):
        """count -> exclusive scan -> one read-back of the total -> fill; returns (pairs, dist2, int tag, float coordinates)"""
        import torch
        from .primitives import exclusive_scan
        counts = torch.zeros(n + 1, dtype=torch.int32, device="cuda")   # one more: its offset is the total
        if count(self.pol.handle, self._h, dhat, counts.data_ptr()) != 0:
            raise RuntimeError("the proximity count pass failed")
        offsets = torch.empty_like(counts)
        exclusive_scan(self.pol, counts, offsets)
        self.pol.syncCtx()
        total = int(offsets[n].item())
        pairs = torch.empty(total, 2, dtype=torch.int32, device="cuda")
        dist2 = torch.empty(total, dtype=torch.float32, device="cuda")
        tag = torch.empty(total, dtype=torch.int32, device="cuda")
        coord = torch.empty(total, widths, dtype=torch.float32, device="cuda")
        if total and fill(self.pol.handle, self._h, dhat, offsets.data_ptr(), pairs.data_ptr(), dist2.data_ptr(), tag.data_ptr(),
                          coord.data_ptr()) != 0:
            raise RuntimeError("the proximity fill pass failed")
        self.pol.syncCtx()
        return pairs, dist2, tag, coord

    def proximity(self, dhat, pt=True, ee=True):
        """the vertex-triangle and edge-edge pairs of the mesh with itself closer than dhat, without topological neighbours (a triangle
        that contains the vertex, edges that share a vertex): a Proximity.  The lists are in a fixed order: two calls give the same bytes."""
        dhat = _positive_f32("proximity", "dhat", dhat)
        r = Proximity()
        L = lib()
        if pt:
            r.pt_pairs, r.pt_dist2, r.pt_feature, r.pt_bary = self._pairs(self.nv, L.zs_rocm_mesh_proximity_pt_count,
                                                                          L.zs_rocm_mesh_proximity_pt_fill, dhat, 3)
        if ee:
            r.ee_pairs, r.ee_dist2, r.ee_category, r.ee_st = self._pairs(self.num_edges, L.zs_rocm_mesh_proximity_ee_count,
                                                                         L.zs_rocm_mesh_proximity_ee_fill, dhat, 2)
        return r

    def set_rest(self, verts=None):
        """stores the squared rest length of every unique edge (the threshold of the edge-edge mollifier) from verts [nv, 3], or from the
        mesh's current vertices"""
        v = self._trial("set_rest", verts)
        if lib().zs_rocm_mesh_set_rest(self.pol.handle, self._h, _ptr(v)) != 0:
            raise RuntimeError("zs_rocm_mesh_set_rest failed")
        self.pol.syncCtx()
        self.has_rest = True

    def rest(self):
        """the squared rest lengths [ne] float32 on the device, rows as TriMesh.edges()"""
        import torch
        r = torch.empty(self.num_edges, dtype=torch.float32, device="cuda")
        if lib().zs_rocm_mesh_rest(self.pol.handle, self._h, r.data_ptr()) != 0:
            raise ValueError("TriMesh.rest: call set_rest first")
        self.pol.syncCtx()
        return r

    def _incidence(self, prox, pt, ee):
        """(starts, entries, scratch size) of the lists of prox, built once and kept on prox"""
        import torch
        if getattr(prox, "_incidence", None) is None:
            npt, nee = (0 if pt is None else len(pt)), (0 if ee is None else len(ee))
            sizes = (C.c_size_t * 3)()
            if lib().zs_rocm_mesh_barrier_sizes(self._h, npt, nee, sizes) != 0:
                raise ValueError("TriMesh.barrier: too many pairs")
            starts = torch.empty(sizes[0], dtype=torch.int32, device="cuda")
            entries = torch.empty(sizes[1], dtype=torch.int32, device="cuda")
            if lib().zs_rocm_mesh_barrier_incidence(self.pol.handle, self._h, _ptr(pt), npt, _ptr(ee), nee, starts.data_ptr(),
                                                    entries.data_ptr()) != 0:
                raise RuntimeError("zs_rocm_mesh_barrier_incidence failed")
            self.pol.syncCtx()
            prox._incidence = (starts, entries, int(sizes[2]))
        return prox._incidence

    def _barrier_args(self, who, prox, dhat, kappa, verts, mollify):
        """what barrier and barrier_hessian_product (who, for the messages) share: the arguments checked; returns the trial positions or None,
        the contiguous lists, their counts and the head of the C call up to mollify"""
        dhat, kappa = _positive_f32(who, "dhat", dhat), _positive_f32(who, "kappa", kappa)
        if mollify and not getattr(self, "has_rest", False):
            raise ValueError("TriMesh.%s: mollify=True needs the rest lengths, call set_rest first" % who)
        if not isinstance(prox, Proximity):
            raise ValueError("TriMesh.%s: prox is the result of TriMesh.proximity" % who)
        v = self._trial(who, verts)
        pt, ee, npt, nee = _pair_lists(prox)
        return v, pt, ee, npt, nee, (self.pol.handle, self._h, _ptr(v), _ptr(pt), npt, _ptr(ee), nee, dhat, kappa, 1 if mollify else 0)

    def _trial(self, who, verts):
        """trial positions on the device, or None"""
        v = None if verts is None else _dev_f32(verts, 3)
        if v is not None and v.shape[0] != self.nv:
            raise ValueError("TriMesh.%s: verts are [nv, 3] positions on the same topology" % who)
        return v

    def _direction(self, who, direction, name="direction", kind="array"):
        d = _dev_f32(direction, 3)
        if d.shape[0] != self.nv:
            raise ValueError("TriMesh.%s: %s is an [nv, 3] %s" % (who, name, kind))
        return d

    def _counts(self, status):
        """waits for the call and returns the counts it left in its status words"""
        self.pol.syncCtx()
        return tuple(int(z) for z in status.tolist())

    def _evaluate(self, r, what, head, sides, terms=None):
        """energy and optional gradient of one term (what: barrier, friction, elastic) into the result r: allocates r.energy, the two
        per-element energies sides = ((field, count or None for a side that is skipped), ..) and, for a gradient, r.grad; terms = (the
        incidence tensors that follow head in the C call.., the size of the scratch array), None: energy only.  Returns the two counts of
        the status word and the scratch array"""
        import torch
        f32 = dict(dtype=torch.float32, device="cuda")
        r.energy = torch.empty((), dtype=torch.float64, device="cuda")
        for field, n in sides:
            setattr(r, field, None if n is None else torch.empty(n, **f32))
        tail = tuple(_ptr(getattr(r, field)) for field, _ in sides) + (r.energy.data_ptr(),)
        status = torch.empty(2, dtype=torch.int32, device="cuda")
        r.grad = scratch = None
        if terms is None:
            rc = getattr(lib(), "zs_rocm_mesh_%s_energy" % what)(*head, *tail, status.data_ptr())
        else:
            scratch, r.grad = torch.empty(terms[-1], **f32), torch.empty(self.nv, 3, **f32)
            rc = getattr(lib(), "zs_rocm_mesh_%s_gradient" % what)(*head, *(t.data_ptr() for t in terms[:-1]), scratch.data_ptr(), *tail,
                                                                   r.grad.data_ptr(), status.data_ptr())
        if rc != 0:
            raise RuntimeError("the %s call failed" % what)
        return self._counts(status), scratch

    def barrier(self, prox, dhat, kappa, verts=None, mollify=True, gradient=True):
        """the IPC barrier potential -kappa (d2 - dhat^2)^2 log(d2 / dhat^2) summed over the pairs of prox (a Proximity of this mesh; a side
        that is None is skipped), and its gradient: a Barrier.  verts [nv, 3]: trial positions on the same topology instead of the mesh's
        own; distances are recomputed there, the lists stay as they are.  mollify: edge-edge pairs are multiplied by the mollifier of
        nearly parallel edges, which needs set_rest.  Two calls give the same bytes."""
        v, pt, ee, npt, nee, head = self._barrier_args("barrier", prox, dhat, kappa, verts, mollify)
        r = Barrier()
        sides = (("pt_energy", None if pt is None else npt), ("ee_energy", None if ee is None else nee))
        r.zero_distance, _ = self._evaluate(r, "barrier", head, sides, self._incidence(prox, pt, ee) if gradient else None)
        return r

    def barrier_hessian_product(self, prox, dhat, kappa, x, verts=None, mollify=True, psd=False):
        """H x for a direction x [nv, 3], H the second derivative of the potential of TriMesh.barrier over the pairs of prox, matrix-free:
        a BarrierHessianProduct.  verts and mollify as for barrier.  psd: the positive semi-definite H+ (every indefinite term discarded
        analytically; a majorant of H without the mollifier, not the eigenvalue projection of the per-pair blocks), the operator a
        conjugate-gradient solve can use.  Two calls give the same bytes."""
        import torch
        v, pt, ee, npt, nee, head = self._barrier_args("barrier_hessian_product", prox, dhat, kappa, verts, mollify)
        d = self._direction("barrier_hessian_product", x, "x", "direction")
        starts, entries, nscratch = self._incidence(prox, pt, ee)
        r = BarrierHessianProduct()
        r.pair_terms = torch.empty(nscratch // 12, 4, 3, dtype=torch.float32, device="cuda")
        r.hx = torch.empty(self.nv, 3, dtype=torch.float32, device="cuda")
        status = torch.empty(2, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_barrier_hessian_product(*head, 1 if psd else 0, d.data_ptr(), starts.data_ptr(), entries.data_ptr(),
                                                      r.pair_terms.data_ptr(), r.hx.data_ptr(), status.data_ptr()) != 0:
            raise RuntimeError("the barrier Hessian product call failed")
        r.zero_distance = self._counts(status)
        return r

    def friction_lag(self, prox, dhat, kappa, verts=None, mollify=True):
        """the lag step of IPC friction: freezes the contact normal, the size of the contact force and the weights of the relative
        displacement of every pair of prox at verts [nv, 3] (None: the mesh's own positions): a FrictionLag.  dhat, kappa, mollify as for
        barrier: the contact force is the barrier's.  Two calls give the same bytes."""
        import torch
        v, pt, ee, npt, nee, head = self._barrier_args("friction_lag", prox, dhat, kappa, verts, mollify)
        sizes = (C.c_size_t * 3)()
        if lib().zs_rocm_mesh_barrier_sizes(self._h, npt, nee, sizes) != 0:
            raise ValueError("TriMesh.friction_lag: too many pairs")
        r = FrictionLag()
        r.prox, r.npt, r.nee = prox, npt, nee
        r.record = torch.empty(npt + nee, 8, dtype=torch.float32, device="cuda")
        status = torch.empty(2, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_friction_lag(*head, r.record.data_ptr(), status.data_ptr()) != 0:
            raise RuntimeError("the friction lag call failed")
        r.zero_distance = self._counts(status)
        return r

    def _friction_args(self, who, lag, u, mu, eps_v):
        """what friction and friction_hessian_product (who, for the messages) share: the arguments checked; returns the displacement, the
        contiguous lists and the head of the C call up to the pair lists"""
        mu, eps_v = float(mu), _positive_f32(who, "eps_v", eps_v)
        if not (0 <= mu <= FLT_MAX):
            raise ValueError("TriMesh.%s: mu must be finite and not negative" % who)
        if not isinstance(lag, FrictionLag):
            raise ValueError("TriMesh.%s: lag is the result of TriMesh.friction_lag" % who)
        d = self._direction(who, u, "u", "displacement")
        pt, ee, npt, nee = _pair_lists(lag.prox)
        rec = lag.record
        if (npt, nee) != (lag.npt, lag.nee) or tuple(rec.shape) != (npt + nee, 8) or rec.dtype != d.dtype or not rec.is_contiguous():
            raise ValueError("TriMesh.%s: the lists of lag.prox have changed since friction_lag" % who)
        return d, pt, ee, npt, nee, mu, eps_v

    def friction(self, lag, u, mu, eps_v, gradient=True):
        """lagged IPC friction at the displacement u [nv, 3] (positions minus the positions at the start of the step): the energy
        mu lam f0(|ut|) summed over the pairs of lag (a FrictionLag of this mesh), ut the tangential part of the pair's relative
        displacement, and its gradient: a Friction.  eps_v: the static-friction threshold in displacement units (the velocity threshold
        times the time step); below it f0 is the smooth cubic, above it |ut|.  Two calls give the same bytes."""
        d, pt, ee, npt, nee, mu, eps_v = self._friction_args("friction", lag, u, mu, eps_v)
        r = Friction()
        head = (self.pol.handle, self._h, d.data_ptr(), _ptr(pt), npt, _ptr(ee), nee, lag.record.data_ptr(), mu, eps_v)
        sides = (("pt_energy", None if pt is None else npt), ("ee_energy", None if ee is None else nee))
        r.overflow, _ = self._evaluate(r, "friction", head, sides, self._incidence(lag.prox, pt, ee) if gradient else None)
        return r

    def friction_hessian_product(self, lag, u, mu, eps_v, x):
        """H x for a direction x [nv, 3], H the second derivative of the energy of TriMesh.friction at u, matrix-free: a
        FrictionHessianProduct.  H is positive semi-definite by construction, so a conjugate-gradient solve can use it as it is.  Two
        calls give the same bytes."""
        import torch
        d, pt, ee, npt, nee, mu, eps_v = self._friction_args("friction_hessian_product", lag, u, mu, eps_v)
        xd = self._direction("friction_hessian_product", x, "x", "direction")
        starts, entries, nscratch = self._incidence(lag.prox, pt, ee)
        r = FrictionHessianProduct()
        r.pair_terms = torch.empty(nscratch // 12, 4, 3, dtype=torch.float32, device="cuda")
        r.hx = torch.empty(self.nv, 3, dtype=torch.float32, device="cuda")
        status = torch.empty(2, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_friction_hessian_product(self.pol.handle, self._h, d.data_ptr(), xd.data_ptr(), _ptr(pt), npt, _ptr(ee), nee,
                                                       lag.record.data_ptr(), mu, eps_v, starts.data_ptr(), entries.data_ptr(),
                                                       r.pair_terms.data_ptr(), r.hx.data_ptr(), status.data_ptr()) != 0:
            raise RuntimeError("the friction Hessian product call failed")
        r.overflow = self._counts(status)
        return r

    def set_rest_shape(self, verts=None):
        """stores the rest shape of the mesh's internal energy from verts [nv, 3], or from the mesh's current vertices: the membrane record
        of every triangle, the hinges (unique edges with exactly two triangles) with their bending records and the vertex areas.  Returns
        the counts (degenerate triangles, degenerate hinges, non-manifold edges): those elements contribute nothing (a non-manifold edge
        makes no hinge).  A second call recomputes the records on the same hinges.  Leaves set_rest and the contact terms alone."""
        v = self._trial("set_rest_shape", verts)
        if lib().zs_rocm_mesh_set_rest_shape(self.pol.handle, self._h, _ptr(v)) != 0:
            raise RuntimeError("zs_rocm_mesh_set_rest_shape failed")
        self.pol.syncCtx()
        sizes = (C.c_size_t * 7)()
        if lib().zs_rocm_mesh_rest_shape_sizes(self._h, sizes) != 0:
            raise RuntimeError("zs_rocm_mesh_rest_shape_sizes failed")
        self.num_hinges, self._elastic_scratch = int(sizes[1]), int(sizes[3])
        self.has_rest_shape = True
        return int(sizes[4]), int(sizes[5]), int(sizes[6])

    def rest_shape(self):
        """(tri_record [nt, 4] float32 (B00, B01, B11, A), hinges [nh, 4] int32, hinge_record [nh, 4] float32, vertex_area [nv] float32) on
        the device.  A hinge row is (v0, v1, v2, v3): v0 < v1 the edge, as in a row of TriMesh.edges(), v2 opposite in the incident triangle
        with the smaller index, v3 in the other; hinges are in edge order.  Lumped masses are density * vertex_area."""
        import torch
        if not getattr(self, "has_rest_shape", False):
            raise ValueError("TriMesh.rest_shape: call set_rest_shape first")
        f32, nh = dict(dtype=torch.float32, device="cuda"), self.num_hinges
        rec, hinges = torch.empty(self.nt, 4, **f32), torch.empty(nh, 4, dtype=torch.int32, device="cuda")
        hrec, area = torch.empty(nh, 4, **f32), torch.empty(self.nv, **f32)
        if lib().zs_rocm_mesh_rest_shape(self.pol.handle, self._h, rec.data_ptr(), hinges.data_ptr(), hrec.data_ptr(), area.data_ptr()) != 0:
            raise RuntimeError("zs_rocm_mesh_rest_shape failed")
        self.pol.syncCtx()
        return rec, hinges, hrec, area

    def _elastic_args(self, who, mu, lam, kb, verts):
        """what elastic and elastic_hessian_product (who, for the messages) share: the arguments checked; returns the trial positions or
        None and the head of the C call up to kb"""
        mu, lam, kb = float(mu), float(lam), float(kb)
        for name, x in (("mu", mu), ("lam", lam), ("kb", kb)):
            if not (0 <= x <= FLT_MAX):
                raise ValueError("TriMesh.%s: %s must be finite and not negative" % (who, name))
        if not getattr(self, "has_rest_shape", False):
            raise ValueError("TriMesh.%s: needs the rest shape, call set_rest_shape first" % who)
        v = self._trial(who, verts)
        return v, (self.pol.handle, self._h, _ptr(v), mu, lam, kb)

    def elastic(self, mu, lam, kb, verts=None, gradient=True):
        """the internal energy of the mesh against the rest shape of set_rest_shape, and its gradient: an Elastic.  Membrane: St.
        Venant-Kirchhoff, A (mu |E|^2 + lam / 2 tr(E)^2) per triangle, E the Green strain of the 3 x 2 deformation gradient, mu and lam
        per-area stiffnesses (the thickness multiplied in).  Bending: the quadratic (isometric) energy of Bergou et al. 2006, kb / 2 |sum_i
        k_i x_i|^2 per hinge.  Its domain is cloth: it is zero at rest only where the rest shape is flat across the hinge, and on a curved
        rest shape it penalises the rest curvature too.  verts [nv, 3]: trial positions instead of the mesh's own.  A zero mu and lam (or
        kb) skips the membrane (or bending) kernels.  Two calls give the same bytes."""
        v, head = self._elastic_args("elastic", mu, lam, kb, verts)
        r = Elastic()
        r.nt = self.nt
        sides = (("tri_energy", self.nt), ("hinge_energy", self.num_hinges))
        r.overflow, r.elem_terms = self._evaluate(r, "elastic", head, sides, (self._elastic_scratch,) if gradient else None)
        return r

    def elastic_hessian_product(self, mu, lam, kb, x, verts=None, psd=False):
        """H x for a direction x [nv, 3], H the second derivative of the energy of TriMesh.elastic, matrix-free: an ElasticHessianProduct.
        psd: the positive semi-definite H+, the membrane stress replaced by its closed-form projection onto the positive semi-definite
        matrices where it multiplies the direction's deformation gradient; H+ majorises H and equals it wherever no triangle is
        compressed, and is the operator a conjugate-gradient solve can use.  The bending part is positive semi-definite as it stands.  Two
        calls give the same bytes."""
        import torch
        v, head = self._elastic_args("elastic_hessian_product", mu, lam, kb, verts)
        d = self._direction("elastic_hessian_product", x, "x", "direction")
        r = ElasticHessianProduct()
        r.nt = self.nt
        r.elem_terms = torch.empty(self._elastic_scratch, dtype=torch.float32, device="cuda")
        r.hx = torch.empty(self.nv, 3, dtype=torch.float32, device="cuda")
        status = torch.empty(2, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_elastic_hessian_product(*head, 1 if psd else 0, d.data_ptr(), r.elem_terms.data_ptr(), r.hx.data_ptr(),
                                                      status.data_ptr()) != 0:
            raise RuntimeError("the elastic Hessian product call failed")
        r.overflow = self._counts(status)
        return r

    def max_step(self, prox, direction, verts=None, slack=0.1, t_max=1.0, max_iter=256):
        """a conservative bound on the step t <= t_max for which verts + t direction (verts=None: the mesh's own positions) keeps every
        pair of prox (a Proximity of this mesh; a side that is None is skipped) free of contact, by additive CCD: a StepBound.  Each pair
        keeps its distance above slack x its distance at t = 0; max_iter caps the distance evaluations of one pair.  Only the pairs of
        prox are looked at: step_candidates gives a list that is complete for a direction.  Two calls give the same bytes."""
        import torch
        slack, t_max = float(slack), _positive_f32("max_step", "t_max", t_max)
        if not (0.0 < slack < 1.0 and 0.0 < float(np.float32(slack)) < 1.0):
            raise ValueError("TriMesh.max_step: slack must be inside (0, 1)")
        if int(max_iter) != max_iter or max_iter < 1 or max_iter > 2 ** 31 - 1:
            raise ValueError("TriMesh.max_step: max_iter is an integer of at least 1")
        if not isinstance(prox, Proximity):
            raise ValueError("TriMesh.max_step: prox is the result of TriMesh.proximity or TriMesh.step_candidates")
        d = self._direction("max_step", direction)
        v = self._trial("max_step", verts)
        pt, ee, npt, nee = _pair_lists(prox)
        r = StepBound()
        r.t = torch.empty((), dtype=torch.float32, device="cuda")
        r.pt_toi = None if pt is None else torch.empty(npt, dtype=torch.float32, device="cuda")
        r.ee_toi = None if ee is None else torch.empty(nee, dtype=torch.float32, device="cuda")
        status = torch.empty(4, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_ccd(self.pol.handle, self._h, _ptr(v), d.data_ptr(), _ptr(pt), npt, _ptr(ee), nee, slack, t_max, int(max_iter),
                                  _ptr(r.pt_toi), _ptr(r.ee_toi), r.t.data_ptr(), status.data_ptr()) != 0:
            raise RuntimeError("the CCD call failed")
        s = self._counts(status)
        r.zero_distance, r.capped = s[:2], s[2:]
        return r

    def step_candidates(self, direction, t_max=1.0, margin=None):
        """the pairs max_step has to look at for steps up to t_max along direction [nv, 3], from the mesh's own positions: self.proximity(r)
        with r = 2 t_max max|direction| + margin + the grey zone of the proximity test, rounded up (candidate_radius).  Complete: over a
        step t <= t_max no vertex moves further than t_max max|direction|, so the distance of a pair falls by at most 2 t_max
        max|direction|; a pair that is not listed has a float32 distance of at least r, a true one of at least r minus the grey zone, and
        keeps at least margin over the whole step.  margin=None: the grey zone once more.  As in every proximity list, topological
        neighbours (a triangle that contains the vertex, edges that share a vertex) are not listed: their distance is zero by
        construction and stays so.  An all-zero direction (or a mesh without triangles) gives an empty Proximity."""
        import torch
        d = self._direction("step_candidates", direction)
        t_max = float(t_max)
        if not (np.isfinite(t_max) and t_max > 0):
            raise ValueError("TriMesh.step_candidates: t_max must be finite and positive")
        if margin is not None and not (np.isfinite(margin) and margin >= 0):
            raise ValueError("TriMesh.step_candidates: margin must be finite and not negative")
        top = float(torch.linalg.vector_norm(d, dim=1).max().item()) if self.nv else 0.0
        if not np.isfinite(top):
            raise ValueError("TriMesh.step_candidates: direction must be finite")
        if top == 0.0 or self.nt == 0:
            r = Proximity()
            i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
            r.pt_pairs, r.pt_dist2, r.pt_feature, r.pt_bary = torch.empty(0, 2, **i32), torch.empty(0, **f32), torch.empty(0, **i32), torch.empty(0, 3, **f32)
            r.ee_pairs, r.ee_dist2, r.ee_category, r.ee_st = torch.empty(0, 2, **i32), torch.empty(0, **f32), torch.empty(0, **i32), torch.empty(0, 2, **f32)
            return r
        lo, hi = self.total_box()
        radius = candidate_radius(top, t_max, margin, lo, hi)
        if not np.isfinite(radius):
            raise ValueError("TriMesh.step_candidates: 2 t_max max|direction| + margin leaves the float range")
        return self.proximity(radius)

    @staticmethod
    def _cap(cap):
        return FLT_MAX if cap is None or not np.isfinite(cap) else float(cap)

    def closest_point(self, points, cap=float("inf")):
        """(dist [n], tri [n], feature [n], bary [n, 3]) as torch tensors on the device; no triangle nearer than cap: dist = cap (the
        largest float for cap = inf), tri = feature = -1"""
        import torch
        p = _dev_f32(points, 3)
        n = int(p.shape[0])
        dist = torch.empty(n, dtype=torch.float32, device="cuda")
        tri = torch.empty(n, dtype=torch.int32, device="cuda")
        feat = torch.empty(n, dtype=torch.int32, device="cuda")
        bary = torch.empty(n, 3, dtype=torch.float32, device="cuda")
        if lib().zs_rocm_mesh_closest_point(self.pol.handle, self._h, p.data_ptr(), n, self._cap(cap), dist.data_ptr(), tri.data_ptr(),
                                            feat.data_ptr(), bary.data_ptr()) != 0:
            raise RuntimeError("zs_rocm_mesh_closest_point failed")
        self.pol.syncCtx()
        return dist, tri, feat, bary

    def signed_distance(self, points, cap=float("inf"), signed=True, allow_open=False):
        """(sdf [n], vel [n, 3] or None); signed=True needs a closed, consistently oriented mesh unless allow_open"""
        import torch
        if signed and not allow_open and not self.is_closed():
            raise ValueError("TriMesh.signed_distance: the mesh is not closed and consistently oriented (%r); pass allow_open=True to take "
                             "the pseudonormal sign anyway" % (self.stats(),))
        p = _dev_f32(points, 3)
        n = int(p.shape[0])
        sdf = torch.empty(n, dtype=torch.float32, device="cuda")
        vel = torch.empty(n, 3, dtype=torch.float32, device="cuda") if self.has_velocity else None
        if lib().zs_rocm_mesh_signed_distance(self.pol.handle, self._h, p.data_ptr(), n, self._cap(cap), sdf.data_ptr(),
                                              None if vel is None else vel.data_ptr()) != 0:
            raise RuntimeError("zs_rocm_mesh_signed_distance failed")
        self.pol.syncCtx()
        return (sdf if signed else sdf.abs()), vel

    def normals(self):
        """(face [nt, 3], vertex [nv, 3], edge [nt, 3, 3]) copied to the host (tests)"""
        v = self.view()
        hip = C.CDLL("libamdhip64.so")

        def fetch(ptr, shape):
            a = np.empty(shape, np.float32)
            if a.size:
                hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.nbytes), 2)
            return a
        self.pol.syncCtx()
        return fetch(v.faceNormals, (self.nt, 3)), fetch(v.vertNormals, (self.nv, 3)), fetch(v.edgeNormals, (self.nt, 3, 3))
