"""The gather-style transfers of zpc_amd/csrc/mpm_c2.hip (c2_octant_kernel, c2_particle_kernel, p2c2g_cell8_kernel, p2c2g_node_kernel,
g2c2p_cell_kernel, g2c2p_particle_kernel, the Pre / Post kernels) against the float64 reference of tests/ref64_c2.py, node by node and
particle by particle, on the scenes of util.c2_scene.  Every check is fed with what the GPU itself holds: its uploaded particles read
back, its active_keys(), its grid before G2C2P.  The bound of every value is its own ((N + c) u T + e_in, derived in ref64_c2 and
validated on the CPU oracle by tests/test_c2_ref64_cpu.py), so a particle missing from one cell, a light particle's mass or a node
missing from one cell's v_c cannot hide under a channel maximum.  The channel-max checks of tests/test_c2_gpu.py stay as the coarser
second check.

Force: where a stress enters (kinds 0, 2), PF of models 0-3 is the GPU's own test entry zs_rocm_mpm_stress on the uploaded F, logJp
(held to float64 by tests/test_stress_ref64_gpu.py) with e_in = util.stress_tol (1e-4 of the row scale: another instantiation computed
it); the fluid's is ref64.eos_pf64 (viscosity 0), to rounding.  Every line prints the gap between the kernel's force and the reference in
units of that e_in (`gap/ePF`: the multiple of ePF the worst node needs once the rest of its bound is used up), so that it can be
tightened from a recorded number.  No node and no particle is excluded from any check
(`excl 0` in every line; check_grid itself fails on a touched node that is not in the partition).

Prints one `REF64 c2 <path> <worst err/bound per channel>` line per check.

Record of the MI355X run of this file (records, not thresholds; worst err / bound over all scenes, sides and models):
  P2C2G, cleared grid     m 0.067   mv 0.052 0.042 0.038 (kind 1 and the fluid; with a stress tolerance in the bound: 0.000)
  P2C2G, pre-filled grid  m 0.972   mv 0.901 0.937 0.978 (the one rounding of prefill + value, against u |prefill| + u T)
  G2C2P fused = 3 calls   v 0.172   B 0.096   x 0.500   F / J 0.706;  accumulate entry  v 0.252   B 0.074
  worst gap/ePF           0.002 (the fluid, to rounding); 0.000 for models 0-3 on every scene: the kernels' force passes with the rounding
                          part of the bound alone, the stress inside c2_particle_kernel and the test entry's agree that closely here
  nodes / particles excluded  0 in all 627 checks
  run time                8 s for the 124 tests, the slowest 0.35 s"""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref64_c2 as r2
from util import c2_scene, c2_lone_pos, C2_SCENES, OracleMpm, stress_tol, rng

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DX, DT, G = 1.0 / 64, 1e-4, (0.0, -9.8, 0.0)
VOL = DX ** 3 / 8
LOGJP_TOL = 1e-4    # ORACLE_TOL of test_stress_ref64_gpu.py: kernel against kernel (test_c2_ref64_cpu.py, control g)


def _kw(model):
    return dict(yield_stress=200.0) if model == 2 else dict(beta=0.5) if model == 3 else {}


def _report(path, r, extra=""):
    r = np.atleast_1d(np.asarray(r, np.float64))
    print("REF64 c2 %s %s excl 0%s" % (path, " ".join("nan" if np.isnan(x) else "%.3f" % x for x in r), extra))


class Run:
    """an MpmTransfer with a scene uploaded, its partition and buckets built"""

    def __init__(self, pol, scene, side, model, buckets="hashed"):
        from zpc_amd.mpm import MpmTransfer
        s = c2_scene(scene, DX)
        if s["block"] is not None:
            s["pos"] = c2_lone_pos(s["block"], side, DX)
        self.pol, self.s, self.model, self.side, self.origin = pol, s, model, side, s["key_is_origin"]
        self.n = n = len(s["mass"])
        self.mt = mt = MpmTransfer(pol, n, DX, DT, model=model, side=side, volume=VOL, key_is_origin=self.origin, viscosity=0.0, **_kw(model))
        self.upload()
        if s["block"] is not None:
            self.keys_dev = torch.tensor(s["block"], dtype=torch.int32).mul(side if self.origin else 1).cuda()
            mt.adopt_partition(self.keys_dev.data_ptr(), 1)
        else:
            mt.build_partition(n)
        self.build_buckets = lambda: mt.build_buckets(displacement=0.5 if buckets == "foreign" else 0.0, dense=buckets == "dense")
        self.build_buckets()
        self.path = "%s s%d m%d%s" % (scene, side, model, "" if buckets == "hashed" else " " + buckets)

    def upload(self):
        s, m = self.s, self.model
        self.mt.upload(s["mass"], s["pos"], s["vel"], s["B"], s["J"] if m == 4 else s["F"], s["logJp"] if m in (1, 3) else None)

    def stress(self, oracle, before):
        """(PF, ePF, logJp the entry leaves) of the particles the GPU holds"""
        mt = self.mt
        if self.model == 4:
            assert mt.params.viscosity == 0
            return ref64.eos_pf64(before["J"][:, 0], mt.params.bulk, mt.params.volume) + (None,)
        from zpc_amd import lib
        Fd = torch.from_numpy(np.ascontiguousarray(before["F"])).cuda()
        ljd = torch.from_numpy(np.ascontiguousarray(before.get("logJp", np.zeros(self.n, np.float32)))).cuda()
        PF = torch.empty(self.n, 9, device="cuda")
        lib().zs_rocm_mpm_stress(self.pol.handle, C.byref(mt.params), Fd.data_ptr(), ljd.data_ptr(), self.n, PF.data_ptr())
        self.pol.syncCtx()
        PF = PF.cpu().numpy()
        om = OracleMpm(oracle, self.model, DX, DT, self.side, VOL, **_kw(self.model))   # (E, nu, volume of stress_tol)
        return PF, stress_tol(om, PF, before["F"]), ljd.cpu().numpy()

    def p2c2g_checked(self, oracle, kind, prefill=None, what="", reuse=None):
        """one P2C2G on the (pre-filled) grid, checked against the reference built from the GPU's own particles and keys; returns the
        worst err / bound of channels 0-3 and the gap in units of ePF.  reuse: a dict that keeps the reference of a kind between two
        runs on the same uploaded particles (asserted)."""
        mt, pol = self.mt, self.pol
        before = mt.download()
        keys = mt.active_keys()
        if reuse is not None and kind in reuse:
            b0, ePF, lj_entry, ref = reuse[kind]
            assert all(np.array_equal(before[k], b0[k]) for k in before)
        else:
            PF, ePF, lj_entry = self.stress(oracle, before) if kind != 1 else (None, None, None)
            ref = r2.p2c2g64(kind, keys, self.side, before["m"], before["x"], before["v"], before["C"], DX, DT, PF=PF, ePF=ePF,
                             key_is_origin=self.origin)
            if reuse is not None:
                reuse[kind] = (before, ePF, lj_entry, ref)
        if prefill is None:
            mt.clear_grid()
            pol.syncCtx()
            pre = np.zeros(mt.grid.numel(), np.float32)
        else:
            pol.syncCtx()
            mt.grid.copy_(torch.from_numpy(prefill).cuda())
            torch.cuda.synchronize()
            pre = prefill
        mt.p2c2g(kind)
        pol.syncCtx()
        coords, got = ref64.to_world_nodes(mt)
        _, pw = ref64.world_nodes(keys, pre, self.side, self.side // mt.kstride)
        diff = got - pw                                                        # exact in float64
        path = "p2c2g[%s k%d%s%s]" % (self.path, kind, " prefilled" if prefill is not None else "", what)
        k = ref64.node_key(coords)
        o = np.argsort(k)
        at_ref = o[np.minimum(np.searchsorted(k[o], ref.keys), len(k) - 1)]    # (check_grid asserts that every touched node exists)
        bound = ref.bound() + ref64.U * np.abs(pw[at_ref])
        ratio = ref64.check_grid(ref, (coords, diff), range(4), path, bound=bound)
        assert (diff[:, 4:] == 0).all(), path + ": channels 4-6 were written"
        if kind == 2:
            assert (diff[:, 0] == 0).all(), path + ": the force transfer wrote mass"
        gap = 0.0
        if ePF is not None:   # the multiple of ePF this run needs: what of the error the rest of the bound does not cover, over ePF's share
            e = ref.e_pf[:, 1:4]
            over = np.abs(diff[at_ref, 1:4] - ref.val[:, 1:4]) - (bound[:, 1:4] - e)
            gap = float(np.clip(over[e > 0] / e[e > 0], 0.0, None).max()) if (e > 0).any() else 0.0
        after = mt.download()
        if "logJp" in after:
            if kind == 1:
                assert np.array_equal(after["logJp"], before["logJp"]), path + ": the momentum transfer changed logJp"
            else:
                d = np.abs(after["logJp"] - lj_entry).max()
                assert d <= LOGJP_TOL, "%s: logJp is %g from the stress entry's" % (path, d)
        _report(path, ratio[:4], " gap/ePF %.3f" % gap)
        return ratio[:4], gap


@pytest.mark.parametrize("scene", C2_SCENES)
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
def test_p2c2g_vs_ref64(pol, oracle, model, side, scene):
    """kinds 0, 1, 2 on this model's particle storage: channels 0-3 node by node, channels 4-6 untouched, no mass from kind 2, logJp
    advanced once (kinds 0, 2) or not at all (kind 1); then the same into a pre-filled grid (the transfer ADDS)"""
    run = Run(pol, scene, side, model)
    pre = (1e-3 * rng(900 + side).standard_normal(run.mt.grid.numel())).astype(np.float32)
    refs = {}
    for kind in (1, 0, 2):
        for prefill in (None, pre):
            run.upload()
            run.p2c2g_checked(oracle, kind, prefill, reuse=refs)


@pytest.mark.parametrize("buckets", ["hashed", "dense", "foreign"])
def test_p2c2g_bucket_kinds_vs_ref64(pol, oracle, buckets):
    """hashed IndexBuckets, buckets over the partition (dense) and buckets that are not this grid's cells (displacement 0.5: no octant
    order, every bucket walked whole), on the cloud that straddles 0"""
    Run(pol, "edge", 8, 0, buckets).p2c2g_checked(oracle, 0)


def _g2c2p_ref(run, world, before, v0=None, B0=None):
    m = run.model
    return r2.g2c2p64(run.mt.active_keys(), run.side, (world[0], world[1][:, 1:4]), before["x"], DX, DT, v0=v0, B0=B0,
                      F=before["F"] if m != 4 and v0 is None else None, J=before["J"][:, 0] if m == 4 and v0 is None else None,
                      key_is_origin=run.origin)


def _check_particles(path, r, after, model, post=True):
    out = [ref64.check_particles(after["v"], r["v"], r["b_v"], path + " v"), ref64.check_particles(after["C"], r["B"], r["b_B"], path + " B")]
    if post:
        out.append(ref64.check_particles(after["x"], r["x"], r["b_x"], path + " x"))
        out.append(ref64.check_particles(after["J"][:, 0], r["J"], r["b_J"], path + " J") if model == 4 else
                   ref64.check_particles(after["F"], r["F"], r["b_F"], path + " F"))
    _report(path, out)
    return out


@pytest.mark.parametrize("scene", C2_SCENES)
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 4])
def test_g2c2p_vs_ref64(pol, oracle, model, side, scene):
    """after the GPU's own P2C2G and grid update: v, B, x and F / J per particle from the fused step call, from the three-call form, and
    v, B from the bare accumulate entry on the uploaded (non-zero) v, B, without Pre"""
    from zpc_amd import lib
    run = Run(pol, scene, side, model)
    mt = run.mt
    mt.clear_grid()
    mt.p2c2g(0)
    mt.grid_update(G)
    pol.syncCtx()
    world = ref64.to_world_nodes(mt)
    before = mt.download()
    buf0 = mt.buf.clone()
    torch.cuda.synchronize()
    r = _g2c2p_ref(run, world, before)
    for fused in (True, False):
        mt.buf.copy_(buf0)
        torch.cuda.synchronize()
        mt.g2c2p(fused=fused)
        pol.syncCtx()
        _check_particles("g2c2p[%s %s]" % (run.path, "fused" if fused else "three calls"), r, mt.download(), model)
    mt.buf.copy_(buf0)
    torch.cuda.synchronize()
    assert np.abs(before["v"]).max() > 0 and np.abs(before["C"]).max() > 0
    assert lib().zs_rocm_mpm_g2c2p(pol.handle, C.byref(mt.params), mt.particles(), None, mt.table.handle, mt.grid.data_ptr(), mt.nblocks) == 0
    pol.syncCtx()
    after = mt.download()
    _check_particles("g2c2p[%s accumulate]" % run.path, _g2c2p_ref(run, world, before, v0=before["v"], B0=before["C"]), after, model, post=False)
    assert np.array_equal(after["x"], before["x"]) and np.array_equal(after["J" if model == 4 else "F"], before["J" if model == 4 else "F"])


@pytest.mark.parametrize("scene", ["lattice", "edge"])
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1])
def test_c2_time_loop_vs_ref64(pol, oracle, model, side, scene):
    """three sub-steps (buckets -> P2C2G -> grid update -> G2C2P), each checked from the state downloaded before it"""
    run = Run(pol, scene, side, model)
    mt = run.mt
    for step in range(3):
        run.build_buckets()
        run.p2c2g_checked(oracle, 0, what=" step %d" % step)
        mt.grid_update(G)
        pol.syncCtx()
        world = ref64.to_world_nodes(mt)
        before = mt.download()
        mt.g2c2p()
        pol.syncCtx()
        _check_particles("g2c2p[%s step %d]" % (run.path, step), _g2c2p_ref(run, world, before), mt.download(), model)


def test_light_particle_mass_change_is_rejected_on_device_data(pol):
    """GPU-side negative control: against a real GPU grid (mixed-mass cloud, kind 1), a reference built with one particle of the 1e-3 m
    slab 1 % heavier is rejected, while the true reference passes"""
    run = Run(pol, "mixed", 4, 0)
    mt = run.mt
    mt.clear_grid()
    mt.p2c2g(1)
    pol.syncCtx()
    world = ref64.to_world_nodes(mt)
    d = mt.download()
    mass, pos = d["m"], d["x"]
    ref = lambda m: r2.p2c2g64(1, mt.active_keys(), 4, m, pos, d["v"], d["C"], DX, DT)
    ref64.check_grid(ref(mass), world, range(4))
    light = np.nonzero((mass < 2e-3 * mass.max()) & (mass > 2e-4 * mass.max()))[0]
    j = light[np.argmin(np.abs(pos[light] - np.median(pos[light], 0)).sum(1))]
    m2 = mass.copy()
    m2[j] *= np.float32(1.01)
    with pytest.raises(AssertionError):
        ref64.check_grid(ref(m2), world, range(4))
