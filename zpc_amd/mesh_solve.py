"""The linear system of one Newton iteration of an implicit cloth / shell step on a TriMesh: MeshSystem puts the mass and the
positive semi-definite Hessians of the mesh's elastic, barrier and friction terms (TriMesh.elastic_hessian_product,
barrier_hessian_product, friction_hessian_product) behind one operator, computes its per-vertex 3 x 3 diagonal blocks and solves with a
block-Jacobi preconditioned conjugate-gradient whose scalars stay on the device.  Set-up code: torch for the plumbing; blocks, operator
and solve run in the library's HIP kernels (zpc_amd/csrc/mesh_solve.hip)."""
import ctypes as C

import numpy as np

from ._lib import lib, MeshSystemDesc
from .mesh import FLT_MAX, FrictionLag, Proximity, _dev_f32, _pair_lists, _positive_f32, _ptr

FLAGS = ("running", "converged", "max_iters", "breakdown", "not_finite")


class SystemCounts:
    """result of MeshSystem.linearize: elastic_overflow = (triangles, hinges), barrier_zero_distance = (PT, EE), friction_overflow =
    (PT, EE) -- elements that contribute nothing to their term's blocks, as in the product calls -- inverse_fallbacks (vertices whose
    combined block could not be inverted in closed form and got the scalar Jacobi) and fixed_masses (vertices whose mass is not finite
    and positive: they are treated as fixed)"""
    __slots__ = ("elastic_overflow", "barrier_zero_distance", "friction_overflow", "inverse_fallbacks", "fixed_masses")


class SystemBlocks:
    """result of MeshSystem.blocks: elastic, barrier, friction [nv, 6] float32 (the diagonal blocks of the terms as (xx, xy, xz, yy, yz,
    zz); zeros for a term the system does not have), combined [nv, 6] = scale ((elastic + barrier) + friction) plus the mass on the
    diagonal, inverse [nv, 6] (its inverse, the scalar Jacobi where the closed form fails, zero at a fixed vertex)"""
    __slots__ = ("elastic", "barrier", "friction", "combined", "inverse")


class SystemSolve:
    """result of MeshSystem.solve: x [nv, 3] float32, iters, residuals [iters + 1] float32 on the host (sqrt(r . z) at the start and
    after every iteration), flag (one of FLAGS but the first: converged, max_iters, breakdown -- p . A p not positive --, not_finite)"""
    __slots__ = ("x", "iters", "residuals", "flag")


def _term(who, name, value, keys, defaults=()):
    """a term given as a dict or as a tuple in the order of keys, as a dict with the defaults filled in"""
    if isinstance(value, dict):
        d = dict(defaults, **value)
    else:
        value = tuple(value)
        d = dict(defaults, **dict(zip(keys, value)))
        if len(value) > len(keys):
            raise ValueError("MeshSystem: %s has at most the fields %s" % (name, ", ".join(keys)))
    if set(d) - set(keys) or not set(keys) - {k for k, _ in defaults} <= set(d):
        raise ValueError("MeshSystem: %s needs the fields %s" % (name, ", ".join(keys)))
    return d


class MeshSystem:
    """MeshSystem(mesh, mass, scale, elastic=None, barrier=None, friction=None, fixed=None): the system A = diag(mass) + scale (H+_elastic
    + H+_barrier + H_friction) on [nv, 3] float32 vectors; scale = h^2 for backward Euler.  mass [nv] float32; a vertex whose mass is not
    finite and positive is treated as fixed.  fixed [nv] (bool or bytes): Dirichlet vertices; their rows of A x are zero and the solve
    leaves them where x0 has them.  Each term is optional: elastic = (mu, lam, kb) as for TriMesh.elastic_hessian_product (needs
    set_rest_shape); barrier = (prox, dhat, kappa[, mollify=True]) as for TriMesh.barrier_hessian_product; friction = (lag, mu, eps_v)
    as for TriMesh.friction_hessian_product, lag a FrictionLag whose lists may differ from the barrier's; dicts with those keys work too.
    The terms are those products with psd=True (friction as it stands), value for value.  Call linearize before blocks, multiply or solve."""

    def __init__(self, mesh, mass, scale, elastic=None, barrier=None, friction=None, fixed=None):
        import torch
        self.mesh, self.pol, self.nv = mesh, mesh.pol, mesh.nv
        m = mass if hasattr(mass, "detach") else torch.from_numpy(np.ascontiguousarray(mass, np.float32))
        self.mass = m.to(device="cuda", dtype=torch.float32).contiguous()
        if tuple(self.mass.shape) != (self.nv,):
            raise ValueError("MeshSystem: mass is an [nv] array")
        self.scale = float(scale)
        if not abs(np.float32(self.scale)) <= FLT_MAX:
            raise ValueError("MeshSystem: scale must be finite")
        self.fixed = None
        if fixed is not None:
            f = fixed if hasattr(fixed, "detach") else torch.from_numpy(np.ascontiguousarray(fixed))
            if tuple(f.shape) != (self.nv,):
                raise ValueError("MeshSystem: fixed is an [nv] array")
            self.fixed = (f.to(device="cuda") != 0).to(torch.uint8).contiguous()
        d = MeshSystemDesc()
        d.mass, d.fixed, d.scale = self.mass.data_ptr(), _ptr(self.fixed), self.scale
        self._keep = []
        if elastic is not None:
            e = _term("MeshSystem", "elastic", elastic, ("mu", "lam", "kb"))
            _, head = mesh._elastic_args("MeshSystem", e["mu"], e["lam"], e["kb"], None)
            d.elastic, (d.mu, d.lam, d.kb) = 1, head[3:]
        if barrier is not None:
            b = _term("MeshSystem", "barrier", barrier, ("prox", "dhat", "kappa", "mollify"), (("mollify", True),))
            _, pt, ee, npt, nee, head = mesh._barrier_args("MeshSystem", b["prox"], b["dhat"], b["kappa"], None, b["mollify"])
            starts, entries, _ = mesh._incidence(b["prox"], pt, ee)
            d.barrier, d.ptPairs, d.npt, d.eePairs, d.nee = 1, _ptr(pt), npt, _ptr(ee), nee
            d.starts, d.entries, (d.dHat, d.kappa, d.mollify) = starts.data_ptr(), entries.data_ptr(), head[7:]
            self._barrier = (b["prox"], npt, nee)
            self._keep += [pt, ee, starts, entries]
        if friction is not None:
            f = _term("MeshSystem", "friction", friction, ("lag", "mu", "eps_v"))
            lag, mu, eps_v = f["lag"], float(f["mu"]), _positive_f32("MeshSystem", "eps_v", f["eps_v"])
            if not (0 <= mu <= FLT_MAX):
                raise ValueError("MeshSystem: the friction coefficient must be finite and not negative")
            if not isinstance(lag, FrictionLag):
                raise ValueError("MeshSystem: friction's lag is the result of TriMesh.friction_lag")
            pt, ee, npt, nee = _pair_lists(lag.prox)
            self._friction_lists_unchanged(lag, npt, nee)
            starts, entries, _ = mesh._incidence(lag.prox, pt, ee)
            d.friction, d.fPtPairs, d.fNpt, d.fEePairs, d.fNee = 1, _ptr(pt), npt, _ptr(ee), nee
            d.fStarts, d.fEntries, d.record, d.fmu, d.epsv = starts.data_ptr(), entries.data_ptr(), lag.record.data_ptr(), mu, eps_v
            self._lag = lag
            self._keep += [pt, ee, starts, entries]
        self._desc = d
        sizes = (C.c_size_t * 3)()
        if lib().zs_rocm_mesh_system_sizes(mesh.handle, C.byref(d), sizes) != 0:
            raise ValueError("MeshSystem: too many pairs")
        self._scratch = torch.empty(max(int(sizes[0]), int(sizes[1])), dtype=torch.float32, device="cuda")
        self._blocks = self._verts = self._u = None

    @staticmethod
    def _friction_lists_unchanged(lag, npt, nee):
        rec = lag.record
        if (npt, nee) != (lag.npt, lag.nee) or tuple(rec.shape) != (npt + nee, 8) or not rec.is_contiguous():
            raise ValueError("MeshSystem: the lists of lag.prox have changed since friction_lag")

    def _check_lists(self):
        """the lists behind the incidences are the ones the system was built on"""
        if self._desc.barrier:
            prox, npt, nee = self._barrier
            if not isinstance(prox, Proximity) or _pair_lists(prox)[2:] != (npt, nee):
                raise ValueError("MeshSystem: the lists of the barrier's prox have changed since the system was built")
        if self._desc.friction:
            self._friction_lists_unchanged(self._lag, *_pair_lists(self._lag.prox)[2:])
            if _pair_lists(self._lag.prox)[2:] != (self._desc.fNpt, self._desc.fNee):
                raise ValueError("MeshSystem: the lists of lag.prox have changed since the system was built")

    def _vector(self, who, x, name):
        v = _dev_f32(x, 3)
        if v.shape[0] != self.nv:
            raise ValueError("MeshSystem.%s: %s is an [nv, 3] array" % (who, name))
        return v

    def linearize(self, verts=None, u=None):
        """fixes the point the Hessians are taken at -- verts [nv, 3]: trial positions for the elastic and the barrier term (None: the
        mesh's own), u [nv, 3]: the displacement since the start of the step for the friction term (required with friction) -- and
        computes the diagonal blocks and their inverses there: a SystemCounts.  Two calls give the same bytes."""
        import torch
        self._check_lists()
        self._verts = self.mesh._trial("MeshSystem.linearize", verts)
        if self._desc.friction:
            if u is None:
                raise ValueError("MeshSystem.linearize: the friction term needs the displacement u")
            self._u = self._vector("linearize", u, "u")
        self._desc.verts, self._desc.u = _ptr(self._verts), _ptr(self._u)
        b = SystemBlocks()
        for k in SystemBlocks.__slots__:
            setattr(b, k, torch.empty(self.nv, 6, dtype=torch.float32, device="cuda"))
        status = torch.empty(8, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_system_blocks(self.pol.handle, self.mesh.handle, C.byref(self._desc), self._scratch.data_ptr(), b.elastic.data_ptr(),
                                            b.barrier.data_ptr(), b.friction.data_ptr(), b.combined.data_ptr(), b.inverse.data_ptr(),
                                            status.data_ptr()) != 0:
            raise RuntimeError("the system blocks call failed")
        self.pol.syncCtx()
        s = [int(z) for z in status.tolist()]
        self._blocks = b
        r = SystemCounts()
        r.elastic_overflow, r.barrier_zero_distance, r.friction_overflow = (s[0], s[1]), (s[2], s[3]), (s[4], s[5])
        r.inverse_fallbacks, r.fixed_masses = s[6], s[7]
        return r

    def _linearized(self, who):
        if self._blocks is None:
            raise ValueError("MeshSystem.%s: call linearize first" % who)
        self._check_lists()

    def blocks(self):
        """the diagonal blocks at the point of linearize: a SystemBlocks.  Entry (i, j) of a term's block at vertex v is component i at v
        of that term's Hessian product with the unit direction e_{v,j}, value for value."""
        self._linearized("blocks")
        return self._blocks

    def multiply(self, x):
        """A x for x [nv, 3]: [nv, 3] float32 on the device.  The element kernels of the three products, then one gather per vertex over
        the elastic triangle run, the elastic hinge run, the barrier run and the friction run; zero rows at fixed vertices.  Two calls
        give the same bytes."""
        import torch
        self._linearized("multiply")
        xd = self._vector("multiply", x, "x")
        q = torch.empty(self.nv, 3, dtype=torch.float32, device="cuda")
        if lib().zs_rocm_mesh_system_multiply(self.pol.handle, self.mesh.handle, C.byref(self._desc), self._scratch.data_ptr(), xd.data_ptr(),
                                              q.data_ptr()) != 0:
            raise RuntimeError("the system multiply call failed")
        self.pol.syncCtx()
        return q

    def solve(self, b, x0=None, max_iters=100, tol=FLT_MAX, rel_tol=1e-3, check_every=8):
        """solves A x = b [nv, 3] from x0 (None: zero) with the conjugate-gradient method preconditioned by the inverse diagonal blocks:
        a SystemSolve.  It stops once res = sqrt(r . z) <= min(rel_tol res0, tol) or after max_iters iterations.  Dot products are
        summed in float64 in a fixed order and the scalars stay on the device; the host reads one flag back every check_every iterations,
        and neither check_every nor a repetition changes a byte of the result."""
        import torch
        self._linearized("solve")
        max_iters, check_every = int(max_iters), int(check_every)
        if max_iters < 0 or check_every < 1:
            raise ValueError("MeshSystem.solve: max_iters >= 0 and check_every >= 1")
        if not (0 <= float(tol) and 0 <= float(rel_tol)):
            raise ValueError("MeshSystem.solve: tol and rel_tol must not be negative")
        bd = self._vector("solve", b, "b")
        x = torch.zeros(self.nv, 3, dtype=torch.float32, device="cuda") if x0 is None else self._vector("solve", x0, "x0").clone()
        record = torch.empty(3 + max_iters, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_system_solve(self.pol.handle, self.mesh.handle, C.byref(self._desc), self._scratch.data_ptr(),
                                           self._blocks.inverse.data_ptr(), bd.data_ptr(), x.data_ptr(), max_iters, min(float(tol), FLT_MAX),
                                           min(float(rel_tol), FLT_MAX), check_every, record.data_ptr()) != 0:
            raise RuntimeError("the system solve call failed")
        self.pol.syncCtx()
        rec = record.cpu().numpy()
        r = SystemSolve()
        r.x, r.iters, r.flag = x, int(rec[0]), FLAGS[int(rec[1])]
        r.residuals = rec[2:3 + r.iters].view(np.float32).copy()
        return r
