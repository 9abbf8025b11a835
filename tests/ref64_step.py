"""The constitutive update that runs INSIDE a step (stress inside P2G, the fused G2P2G steps), checked from what the step leaves behind.

After such a step the particle storage holds the unprojected F' = (I + dt C) F as float32 bits and the new logJp (and, where the step
stores it, stress_pack of the P F^T vol it scattered); the logJp before the step is in the download taken before it.  So the exact
inputs of the constitutive update (stored F', previous logJp) and its outputs are all observable and nothing is replayed: a second
instantiation of the same update, the `entry` (on the GPU the test entry zs_rocm_mpm_stress, which tests/test_stress_ref64_gpu.py holds
to float64; on the CPU util.oracle_stress_all, with the oracle's step standing in for the kernel), is run on copies of those bits and

    logJp          stored logJp against the entry's, within LOGJP_TOL
    stored stress  the six stored components against stress_pack of the entry's nine, within util.stress_tol
    force          ref64.p2g64(..., PF = the entry's, ePF = util.stress_tol) node by node on all 7 channels; `gap/ePF` is the multiple of
                   ePF the worst node needs once the rounding part of its bound is used up (tests/test_c2_ref64_gpu.py)
    link           the entry's P F^T vol, projected F and logJp on these very states are, sample by sample, no further from the float64
                   reference (ref64_stress.evaluate) than the CPU oracle on the same bits plus LINK_TOL of the scale (the rule of
                   ref64_stress.ORACLE_OWN_ERROR).  Samples within MARGIN_FACTOR propagated S errors of a branch boundary are left out;
                   their share is asserted <= EXCLUDED_CAP.  The S error the margins are built from is that of the `benign` family
                   (F = I + 0.2 N): the states here are I + O(0.01 ... 0.1), between `near_identity` and `benign`, and the larger error
                   gives the wider margin.
    store paths    particles by what the step did with them: stayed in the cell (base node) they were in, moved to another cell of
                   the same 4^3 bin, left the bin -- the three store paths of the fused kernels (register accumulation; queued in
                   LDS, re-reading the packed stress; the exact path)

numpy only; shared by tests/test_mpm_ref64_gpu.py and tests/test_step_stress_ref64_cpu.py."""
import numpy as np

import ref64
import ref64_stress as rs
from util import OracleMpm, oracle_stress_all, stress_tol

LOGJP_TOL = 1e-4        # the project's figure for logJp, kernel against kernel (test_c2_ref64_gpu.py, test_stress_ref64_gpu.ORACLE_TOL)
LINK_TOL = 1e-4         # of the scale: what the entry may be further from float64 than the oracle is
S_ERR = rs.MEASURED_SVD["benign"][0]
PATHS = ("cell", "bin", "left")
PLASTIC = (1, 2, 3)


DX = 1.0 / 64
VOL = DX ** 3 / 8
G = (0.0, -9.8, 0.0)
# the steps that compute their own stress, as tests/test_mpm_ref64_gpu.py runs them and tests/test_step_stress_ref64_cpu.py proves them
# on the oracle first: (cloud, model) of the compact fused steps (3 steps) and of the slotted steps (6 steps), dt = 1e-3
FUSED_CLOUDS, FUSED_STEPS = ("lattice", "edge_moving"), 3
SLOTTED_CASES = [("drifting", 8, 1), ("drifting", 8, 0), ("drifting", 4, 0), ("edge_moving", 8, 0), ("edge_moving", 4, 1), ("uneven", 8, 1),
                 ("uneven", 4, 0), ("drifting", 8, 2), ("drifting", 8, 3), ("edge_moving", 4, 3), ("uneven", 4, 2)]
SLOTTED_STEPS = 6
MOVING = ("edge_moving", "drifting", "uneven")


def cloud(name):
    """mass, pos, vel, C, F of the named cloud (dx = 1 / 64); identity-tagged masses"""
    from util import make_cloud, make_mixed_cloud, make_edge_cloud, make_drifting_cloud, make_uneven_cloud, tag_masses
    if name == "lattice":
        m, x, v, Cm, F = make_cloud(6, DX, 2, seed=3)
    elif name == "mixed":
        m, x, v, Cm, F = make_mixed_cloud(6, DX)
    elif name == "edge":
        m, x, v, Cm, F = make_edge_cloud(DX)
    elif name == "edge_moving":   # straddles 0 and drifts ~0.1 cell per step (dt 1e-3) across block faces at negative keys
        m, x, v, Cm, F = make_edge_cloud(DX, drift=(-1.6, 1.5, -1.4), vel_scale=0.1)
    elif name == "drifting":
        m, x, v, Cm, F = make_drifting_cloud()
    else:
        m, x, v, Cm, F, _ = make_uneven_cloud(2024, ncell=8)
    return tag_masses(m) if name in ("lattice", "mixed", "edge", "edge_moving") else m, x, v, Cm, F


def state(model, F, n):
    """(F or the fluid's J [n, 1], logJp [n]) that the step tests upload"""
    from util import rng
    if model == 4:
        J = (1.0 + 0.01 * rng(11).standard_normal(n)).astype(np.float32)
        return J[:, None], (0.01 * rng(33).standard_normal(n)).astype(np.float32)
    return F, (0.01 * rng(33).standard_normal(n)).astype(np.float32)


def model_kw(model):
    """the material of the step tests: von Mises yields at |F - I| ~ 0.01, NACC with beta 0.5; everything else the defaults"""
    return dict(yield_stress=200.0) if model == 2 else dict(beta=0.5) if model == 3 else {}


def pset(model, volume, **kw):
    """ref64_stress parameter set of an MpmTransfer / OracleMpm built with the keywords kw (their defaults otherwise)"""
    return dict(dict(rs._BASE, yield_stress=240e6, model=model, volume=volume), **kw)


def stress_pack(PF):
    """stress_pack (mpm_math.hpp) in float32: {xx, (xy + yx) / 2, (xz + zx) / 2, yy, (yz + zy) / 2, zz}"""
    PF = np.asarray(PF, np.float32)
    h = np.float32(0.5)
    return np.stack([PF[:, 0], h * (PF[:, 1] + PF[:, 3]), h * (PF[:, 2] + PF[:, 6]), PF[:, 4], h * (PF[:, 5] + PF[:, 7]), PF[:, 8]], 1)


def stress_unpack(S6):
    return np.asarray(S6)[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]


def store_paths(x_before, x_after, dx, side):
    """(path [n] in 0 = stayed in its cell, 1 = moved within its 4^3 bin, 2 = left the bin; left_block [n] bool) from the float32 base
    nodes of the positions before and after the step (ref64.arena32: the cell the kernels bin by); blocks are side^3 cells at
    multiples of side, as the partition keys say"""
    c0, c1 = ref64.arena32(x_before, dx)[0], ref64.arena32(x_after, dx)[0]
    cell = (c0 != c1).any(1)
    left = (c0 // 4 != c1 // 4).any(1)
    return np.where(left, 2, np.where(cell, 1, 0)), (c0 // side != c1 // side).any(1)


def force_gap(ref, world):
    """the multiple of ePF that the worst force value needs: what of its error the rounding part of the bound does not cover, over the
    share of ePF in the bound (ref.ein of channels 4-6 holds nothing else)"""
    gc, gv = world
    k = ref64.node_key(gc)
    o = np.argsort(k)
    at = o[np.minimum(np.searchsorted(k[o], ref.keys), len(k) - 1)]
    e = ref.ein[:, 4:7]
    over = np.abs(gv[at, 4:7] - ref.val[:, 4:7]) - (ref.bound()[:, 4:7] - e)
    return float(np.clip(over[e > 0] / e[e > 0], 0.0, None).max()) if (e > 0).any() else 0.0


def oracle_steps(oracle, cloud_name, model, nsteps, dt=1e-3, side=4):
    """The step sequence of the fused tests on the CPU oracle (solids): a priming P2G (it advances logJp once, as update_stress
    does before the first fused step), then per step grid update, G2P and, on the partition of the new positions, P2G with the stress
    inside.  Yields per step a dict: grid_before (world nodes the G2P read), x0, F0, lj_prev (before the step), m, x, v, C, F, lj (what
    the step leaves) and world (its grid)."""
    mass, x, v, Cm, F = cloud(cloud_name)
    n = len(mass)
    F, lj = state(model, F, n)
    x, v, Cm, F = x.copy(), v.copy(), Cm.copy(), F.copy()
    om = OracleMpm(oracle, model, DX, dt, side, VOL, **model_kw(model))
    om.build_partition(x, n)
    om.p2g(mass, x, v, Cm, F, lj)
    for step in range(nsteps):
        om.grid_update(G)
        before = ref64.world_nodes(om.keys, om.grid, side, side)
        x0, F0 = x.copy(), F.copy()
        om.g2p(x, v, Cm, F)
        lj_prev = lj.copy()
        om.o.orc_bht_destroy(om.table)
        om.build_partition(x, n)
        om.p2g(mass, x, v, Cm, F, lj)
        yield dict(step=step, grid_before=before, x0=x0, F0=F0, lj_prev=lj_prev, m=mass, x=x.copy(), v=v.copy(), C=Cm.copy(), F=F.copy(),
                   lj=lj.copy(), world=ref64.world_nodes(om.keys, om.grid, side, side))


class Result:
    """what StepCheck.constitutive found: PF, ePF, lj, Fp (the entry's), R (the float64 reference), excluded, gap_lj, gap_S6"""


class StepCheck:
    """the checks of the module docstring for one model and material.  entry(F, lj) -> (P F^T vol [n, 9], projected F [n, 9], new
    logJp [n]) works on copies; the default is the CPU oracle's."""

    def __init__(self, oracle, model, dx, dt, volume, entry=None, **kw):
        self.oracle, self.model, self.dx, self.dt = oracle, model, dx, dt
        self.om = OracleMpm(oracle, model, dx, dt, 4, volume, **kw)     # E, nu, volume of stress_tol
        self.pset = pset(model, volume, **kw)
        self.m = rs.material(self.pset)
        self.entry = entry if entry is not None else self.oracle_entry
        self.has_lj = model in (1, 3)

    def oracle_entry(self, F, lj):
        return oracle_stress_all(self.oracle, self.m, F, lj)

    def link64(self, path, F, lj_prev, got):
        """the entry's three outputs on (F, lj_prev) against float64, sample by sample, relative to the oracle's on the same bits"""
        R = rs.evaluate(self.pset, F, lj_prev, S_ERR)
        orc = oracle_stress_all(self.oracle, R.m, F, lj_prev)
        eg, eo = rs.stress_errors(R, *got), rs.stress_errors(R, *orc)
        ref_fin = dict(PF=np.isfinite(R.PF).all(1), F=np.isfinite(R.F).all(1), lj=np.isfinite(R.lj))
        worst = {}
        for o in ("PF", "F", "lj"):
            sel = ~R.near_of[o]
            assert np.array_equal(eg["fin_" + o][sel], ref_fin[o][sel]), "%s: finite pattern of the entry's %s differs from float64 at %s" % (
                path, o, np.flatnonzero(sel & (eg["fin_" + o] != ref_fin[o]))[:5])
            sel = sel & ref_fin[o] & eo["fin_" + o]
            d = np.where(sel, eg[o] - eo[o], -np.inf)
            worst[o] = (float(eg[o][sel].max()), float(eo[o][sel].max())) if sel.any() else (0.0, 0.0)
            i = int(d.argmax())
            assert d[i] <= LINK_TOL, "%s: the entry's %s is %.3g of the scale from float64 at sample %d, the oracle %.3g" % (
                path, o, eg[o][i], i, eo[o][i])
        excluded = float(R.near.mean())
        assert excluded <= rs.EXCLUDED_CAP, "%s: %.1f %% of the samples are near a branch boundary" % (path, 100 * excluded)
        return R, excluded, worst

    def constitutive(self, path, F, lj_prev, lj_now=None, S6=None, paths=None):
        """the entry on copies of (stored F, previous logJp); stored logJp and stored stress against it; the link to float64"""
        n = len(F)
        F = np.ascontiguousarray(F, np.float32)
        lj_prev = np.zeros(n, np.float32) if lj_prev is None or not self.has_lj else np.ascontiguousarray(lj_prev, np.float32)
        PF, Fp, lj = self.entry(F.copy(), lj_prev.copy())
        res = Result()
        res.PF, res.Fp, res.lj = PF, Fp, lj
        res.ePF = stress_tol(self.om, PF, F)
        assert np.isfinite(PF).all() and np.isfinite(Fp).all() and np.isfinite(lj).all(), path + ": the entry's result is not finite"
        res.gap_lj = [0.0, 0.0, 0.0]
        line = ""
        if self.has_lj:
            assert lj_now is not None
            d = np.abs(np.asarray(lj_now, np.float64) - lj)
            if paths is not None:
                res.gap_lj = [float(d[paths == k].max()) if (paths == k).any() else 0.0 for k in range(3)]
                line += " logJp gap cell %.2e bin %.2e left %.2e" % tuple(res.gap_lj)
            else:
                line += " logJp gap %.2e" % d.max()
            assert d.max() <= LOGJP_TOL, "%s: logJp of particle %d is %g from the stress entry's" % (path, int(d.argmax()), d.max())
        res.gap_S6 = 0.0
        if S6 is not None:
            d = np.abs(np.asarray(S6, np.float64) - stress_pack(PF))
            tol = res.ePF[:, :6]
            res.gap_S6 = float((d / (tol / 1e-4)).max())
            line += " stored stress gap %.2e of the scale" % res.gap_S6
            assert (d <= tol).all(), "%s: the stored stress of particle %d is %.3g of the scale from the entry's" % (
                path, int((d / tol).max(1).argmax()), res.gap_S6)
        if self.model < 4:
            res.R, res.excluded, worst = self.link64(path, F, lj_prev, (PF, Fp, lj))
            line += " | float64: entry PF %.2e F %.2e logJp %.2e (oracle %.2e %.2e %.2e) excl %.2f %%" % (
                worst["PF"][0], worst["F"][0], worst["lj"][0], worst["PF"][1], worst["F"][1], worst["lj"][1], 100 * res.excluded)
        print("REF64 step %s%s" % (path, line))
        return res

    def force(self, path, world, m, x, v, Cm, PF, ePF, ev=None, eC=None, channels=range(7), what="force"):
        """all of `channels` node by node from the reference with this stress and its tolerance; returns (ref, err / bound, gap/ePF)"""
        ref = ref64.p2g64(m, x, v, Cm, self.dx, self.dt, PF=PF, ev=ev, eC=eC, ePF=ePF)
        ratio = ref64.check_grid(ref, world, channels, path + " " + what)
        gap = force_gap(ref, world)
        print("REF64 step %s %s %s gap/ePF %.3f" % (path, what, " ".join("nan" if np.isnan(r) else "%.3f" % r for r in ratio), gap))
        return ref, ratio, gap
