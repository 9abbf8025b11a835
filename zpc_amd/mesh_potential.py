"""The incremental potential of an implicit cloth / shell step on a TriMesh, the function MeshSystem (zpc_amd/mesh_solve.py) linearises:

    E(x) = 1/2 (x - target)^T M (x - target) + scale (Psi_elastic(x) + B(x) + D(x - start))

MeshPotential evaluates it with its gradient in one fused pass and walks down it with a backtracking line search whose decisions stay on
the device.  Set-up code: torch for the plumbing; evaluation and search run in the library's HIP kernels (zpc_amd/csrc/mesh_potential.hip).

Known limitation: the per-element energies are float32, so close to convergence the decrease the Armijo test asks for falls below the
rounding of the elements' energies and the search can end with the flag max_trials although the direction descends.  The flag says so;
nothing papers over it."""
import ctypes as C

import numpy as np

from ._lib import lib, MeshSystemDesc
from .mesh import _dev_f32, _ptr
from .mesh_solve import MeshSystem

FLAGS = ("running", "accepted", "max_trials", "not_descent", "not_finite")


class PotentialValue:
    """result of MeshPotential.evaluate: energy (0-dim float64 device tensor), parts [4] float64 on the device (inertia, elastic, barrier,
    friction: energy = parts[0] + scale ((parts[1] + parts[2]) + parts[3])), grad [nv, 3] float32 or None, and the counts elastic_overflow
    = (triangles, hinges), barrier_zero_distance = (PT, EE), friction_overflow = (PT, EE) as in SystemCounts"""
    __slots__ = ("energy", "parts", "grad", "elastic_overflow", "barrier_zero_distance", "friction_overflow")


class LineSearchResult:
    """result of MeshPotential.line_search: x [nv, 3] float32 (the accepted trial, or a copy of verts when none was accepted), t (the
    accepted step, 0.0 when none was), energy (float64: of the accepted trial, else E0), slope (float64: grad . direction), trials,
    energies (the float64 history on the host: E0, then one entry per trial), flag (one of FLAGS but the first: accepted, max_trials,
    not_descent -- the slope is not negative --, not_finite -- E0, the slope or t_max is not finite, or t_max <= 0)"""
    __slots__ = ("x", "t", "energy", "slope", "trials", "energies", "flag")


class MeshPotential:
    """MeshPotential(mesh, mass, scale, target, start=None, elastic=None, barrier=None, friction=None, fixed=None).  mass, scale, fixed and
    the three terms are MeshSystem's, argument for argument (a vertex whose mass is not finite and positive is fixed).  target [nv, 3]
    float32: the inertia target (x + h v + h^2 g for backward Euler).  start [nv, 3] float32: the positions at the start of the step; the
    friction term is taken at u = x - start, so start is required with friction.  A fixed vertex has no inertia energy, a zero gradient
    row, and stays where it is in a line search.

    The barrier's prox may be any Proximity of the mesh with a radius of at least dhat: the barrier is exactly zero from dhat on, so pairs
    beyond dhat add exactly nothing to energy or gradient.  A list from mesh.step_candidates(direction, t_max, margin=dhat) therefore holds
    every pair that can come within dhat over steps up to t_max and is valid for every trial of a line search up to t_max."""

    def __init__(self, mesh, mass, scale, target, start=None, elastic=None, barrier=None, friction=None, fixed=None):
        import torch
        # the system's descriptor, checks and incidences
        self._system = S = MeshSystem(mesh, mass, scale, elastic=elastic, barrier=barrier, friction=friction, fixed=fixed)
        self.mesh, self.pol, self.nv = mesh, mesh.pol, mesh.nv
        self.mass, self.fixed, self.scale = S.mass, S.fixed, S.scale
        self.target = self._vector("__init__", target, "target")
        if start is None and S._desc.friction:
            raise ValueError("MeshPotential: the friction term needs start, the positions at the start of the step")
        self.start = None if start is None else self._vector("__init__", start, "start")
        self._desc = d = MeshSystemDesc()
        C.memmove(C.byref(d), C.byref(S._desc), C.sizeof(d))
        sizes = (C.c_size_t * 3)()
        if lib().zs_rocm_mesh_potential_sizes(mesh.handle, C.byref(d), sizes) != 0:
            raise ValueError("MeshPotential: too many pairs")
        self._scratch = S._scratch      # (the system's own: it holds the operator's terms, laid out as the gradient's are)
        assert self._scratch.numel() >= int(sizes[0])
        self._energies = torch.empty(int(sizes[1]), dtype=torch.float32, device="cuda")

    def _vector(self, who, x, name):
        v = _dev_f32(x, 3)
        if v.shape[0] != self.nv:
            raise ValueError("MeshPotential.%s: %s is an [nv, 3] array" % (who, name))
        return v

    def _head(self, verts):
        return (self.pol.handle, self.mesh.handle, C.byref(self._desc), self.target.data_ptr(), _ptr(self.start), verts.data_ptr())

    def evaluate(self, verts, gradient=True):
        """E and its gradient at verts [nv, 3]: a PotentialValue.  The element kernels of the three terms write their energies and gradient
        terms once, one gather per vertex sums the four runs and adds the inertia term, and each part is totalled in float64 in the order
        of the public calls, so parts[1:] equal the .energy of TriMesh.elastic / barrier / friction at the same point bit for bit.
        gradient=False: the energy operations and no gather; the energies are the same.  Two calls give the same bytes."""
        import torch
        S = self._system
        S._check_lists()
        x = self._vector("evaluate", verts, "verts")
        r = PotentialValue()
        out = torch.empty(5, dtype=torch.float64, device="cuda")
        r.grad = torch.empty(self.nv, 3, dtype=torch.float32, device="cuda") if gradient else None
        status = torch.empty(6, dtype=torch.int32, device="cuda")
        if lib().zs_rocm_mesh_potential_evaluate(*self._head(x), self._scratch.data_ptr(), self._energies.data_ptr(), out.data_ptr(), _ptr(r.grad),
                                                 status.data_ptr()) != 0:
            raise RuntimeError("the potential evaluate call failed")
        self.pol.syncCtx()
        s = [int(z) for z in status.tolist()]
        r.parts, r.energy = out[:4], out[4]
        r.elastic_overflow, r.barrier_zero_distance, r.friction_overflow = (s[0], s[1]), (s[2], s[3]), (s[4], s[5])
        return r

    def line_search(self, verts, direction, t_max, c1=1e-4, shrink=0.5, max_trials=30, check_every=4):
        """backtracking from verts along direction [nv, 3]: trial k is x_k = verts + t_k direction with t_0 = t_max, t_{k+1} = shrink t_k,
        accepted iff E(x_k) is finite and E(x_k) <= E(verts) + c1 t_k slope, slope = grad . direction (float64): a LineSearchResult.  t_max
        is a Python float or a 0-dim float32 device tensor (StepBound.t goes straight in, without a read-back).  The energies, the slope
        and the decisions stay on the device; the host reads one flag back every check_every trials, and neither check_every nor a
        repetition changes a byte of the result.

        The call makes no collision check of its own: a trial that crosses a pair has a finite barrier energy on the far side, so t_max
        must come from TriMesh.max_step over a list that is complete for the direction (TriMesh.step_candidates)."""
        import torch
        S = self._system
        S._check_lists()
        c1, shrink, max_trials, check_every = float(c1), float(shrink), int(max_trials), int(check_every)
        if not (0 <= c1 and np.isfinite(np.float32(c1))):
            raise ValueError("MeshPotential.line_search: c1 must be finite and not negative")
        if not (0 < np.float32(shrink) < 1):
            raise ValueError("MeshPotential.line_search: shrink must be inside (0, 1)")
        if max_trials < 1 or check_every < 1:
            raise ValueError("MeshPotential.line_search: max_trials >= 1 and check_every >= 1")
        x = self._vector("line_search", verts, "verts")
        p = self._vector("line_search", direction, "direction")
        if hasattr(t_max, "detach"):
            if t_max.numel() != 1 or t_max.dtype != torch.float32 or not t_max.is_cuda:
                raise ValueError("MeshPotential.line_search: t_max is a float or a 0-dim float32 device tensor")
            t_host, t_dev = 0.0, t_max
        else:
            t_host, t_dev = float(np.float32(t_max)), None
        r = LineSearchResult()
        r.x = torch.empty(self.nv, 3, dtype=torch.float32, device="cuda")
        record = torch.empty(4 + max_trials + 1, dtype=torch.float64, device="cuda")
        if lib().zs_rocm_mesh_potential_line_search(*self._head(x), p.data_ptr(), t_host, _ptr(t_dev), c1, shrink, max_trials, check_every,
                                                    self._scratch.data_ptr(), self._energies.data_ptr(), r.x.data_ptr(), record.data_ptr()) != 0:
            raise RuntimeError("the potential line search call failed")
        self.pol.syncCtx()
        rec = record.cpu().numpy()
        head = rec[:2].view(np.int32)
        r.trials, r.flag, r.t = int(head[0]), FLAGS[int(head[1])], float(rec[:2].view(np.float32)[2])
        r.energy, r.slope = float(rec[2]), float(rec[3])
        r.energies = rec[4:5 + r.trials].copy()
        return r
