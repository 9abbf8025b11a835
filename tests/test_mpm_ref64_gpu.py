"""Every particle <-> grid transfer path of the C ABI against the float64 reference of tests/ref64.py, node by node and particle by
particle, each fed with inputs the GPU itself produced (its grid before a step, its stored particle state after it).  The bound of every
value is its own ((N + c) u T + e_in, see ref64), so a free-surface node, a node where momentum cancels or a lost low-weight term cannot
hide under the channel maximum.  The channel-max checks of the other modules stay as a second, coarser check.

Force channels: where the kernel read the cached P F^T vol, the test reads the same 6 components back (mt.off["PF"]) and the force is
checked to rounding.  Where the step computed the stress itself (stress inside P2G, the compact and slotted fused steps, step_slotted),
the constitutive update is checked from what the step leaves behind (tests/ref64_step.py, proven on the CPU oracle by
tests/test_step_stress_ref64_cpu.py): every solid's stored F is the unprojected (I + dt C) F and is held to ref64.g2p64's bound; the
GPU's own test entry zs_rocm_mpm_stress runs on copies of (stored F, the logJp downloaded before the step), and for models 0-3 alike
  - the stored logJp is within LOGJP_TOL = 1e-4 of the entry's (models 1, 3), reported per store path (stayed in its cell / moved within
    the 4^3 bin / left the bin; each path is taken in every plastic case on a moving cloud, asserted);
  - with write_all the six stored stress components are within util.stress_tol (1e-4 of the row scale) of stress_pack of the entry's nine;
  - the force is checked on channels 4-6 of every step and mode, the product instantiation and step_slotted included, with the entry's
    stress and e_in = util.stress_tol, and with write_all once more from the six stored components (the same e_in, there only for the
    symmetrisation); FixedCorotated keeps its earlier check against the oracle's stress of the stored F as well;
  - on these very states the entry's P F^T vol, projected F and logJp are, sample by sample, no further from float64
    (ref64_stress.evaluate) than the CPU oracle on the same bits plus 1e-4 of the scale; samples within MARGIN_FACTOR propagated S
    errors of a branch boundary are left out, their share asserted <= 5 % per step.
The fluid's force is checked to rounding from its closed-form stress of the stored J.  Every force line prints `gap/ePF`, the multiple
of e_in the worst node needs once the rounding part of its bound is used up, so that e_in can be tightened from a recorded number.
Prints `REF64 <path> <worst err/bound per value>` and `REF64 step <path> ...` lines.

Record of the MI355X run of this file (2026-10-20; records, not thresholds; worst over all cases and steps):
  P2G half of the steps     m 0.296   mv 0.214 0.223 0.256   force, with the stress tolerance in its bound: 0.001 (the fluid, to
                            rounding: 0.153 0.187 0.184)
  G2P half                  x 0.491   v 0.163   C 0.100   F 0.706 (all solids)   J 0.462
  worst gap/ePF             entry's stress 0.000 on models 0-3 in every mode (unfused, compact, slotted, step_slotted): the kernels'
                            force passes with the rounding part of the bound alone; from the six stored components 0.003 (model 0,
                            the symmetrisation); FixedCorotated with the oracle's stress 0.004; the fluid 0.122 (of its rounding bound)
  stored stress (write_all) 0 of the scale from stress_pack of the entry's, models 0-3
  logJp gap to the entry    sand 0 on all three paths in every mode; NACC 1.19e-7 (compact) and 5.96e-8 (slotted) on the in-cell path,
                            0 on the in-bin and left-the-bin paths, 0 after the unfused P2G
  entry against float64     PF 4.1e-5 / 1.7e-5 / 7.9e-6 / 9.3e-6, projected F - / 1.2e-4 / 1.2e-4 / 5.4e-5, logJp - / 9.4e-7 / - / 1.1e-6
                            of the scale for models 0 / 1 / 2 / 3 (the oracle: 4.1e-5 / 1.7e-5 / 7.6e-6 / 9.5e-6 on PF)
  excluded share            <= 1.22 % sand (the uploaded state), 0.02 % von Mises, 4.03 % NACC (drifting, side 8)
  run time                  26 s for the 173 tests, the slowest 0.92 s"""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref64_step as st
from ref64_step import cloud as _cloud, state as _state, model_kw as _kw
from util import make_mixed_cloud, make_full_cell_cloud, move_after_binning, OracleMpm, oracle_stress, stress_tol as _stress_tol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DX = 1.0 / 64
G = (0.0, -9.8, 0.0)


def _report(path, r):
    r = np.atleast_1d(np.asarray(r, np.float64))
    print("REF64 %s %s" % (path, " ".join("nan" if np.isnan(x) else "%.3f" % x for x in r)))


def _read_all(mt):
    """[n, nchn] of the stored particles (slotted: the occupied slots), all channels (PF included)"""
    buf = mt.buf
    if mt.slotted:
        buf, cnt = mt._compact_copy()
        assert cnt == mt.n
    aos = torch.empty(mt.n, mt.nchn, dtype=torch.float32, device="cuda")
    __import__("zpc_amd").lib().zs_rocm_tv_to_aos_f32(mt.pol.handle, buf.data_ptr(), mt.n, mt.nchn, mt.L, aos.data_ptr())
    mt.pol.syncCtx()
    return aos.cpu().numpy()


def _fields(a, mt):
    nF = mt.nF
    out = dict(m=a[:, 0], x=a[:, 1:4], v=a[:, 4:7], C=a[:, 7:16], F=a[:, 16:16 + nF])
    if mt.model in (1, 3):
        out["logJp"] = a[:, mt.off["logJp"]]
    if "PF" in mt.off:
        S = a[:, mt.off["PF"]:mt.off["PF"] + 6]
        out["S6"] = S
        out["PF"] = S[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
    return out


def _checker(pol, oracle, mt, dt):
    """ref64_step.StepCheck of an MpmTransfer's material whose entry is the GPU's own zs_rocm_mpm_stress on copies of (F, logJp)"""
    from zpc_amd import lib

    def entry(F, lj):
        n = len(F)
        Fd, ljd = torch.from_numpy(np.ascontiguousarray(F, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(lj, np.float32)).cuda()
        PF = torch.empty(n, 9, device="cuda")
        lib().zs_rocm_mpm_stress(pol.handle, C.byref(mt.params), Fd.data_ptr(), ljd.data_ptr(), n, PF.data_ptr())
        pol.syncCtx()
        return PF.cpu().numpy(), Fd.cpu().numpy(), ljd.cpu().numpy()
    return st.StepCheck(oracle, mt.model, DX, dt, mt.params.volume, entry=entry if mt.model < 4 else None, **_kw(mt.model))


def _by_mass(f):
    o = np.argsort(f["m"], kind="stable")
    return {k: v[o] for k, v in f.items()}


def _grid_update_checked(mt, path, dt):
    """grid_update + CFL max from 0: node v from the GPU's own pre-update sums, max_vel = max of the GPU's own |v|^2"""
    pre = ref64.to_world_nodes(mt)
    mx = torch.zeros(1, dtype=torch.float32, device="cuda")
    mt.grid_update(G, mx)
    mt.pol.syncCtx()
    post = ref64.to_world_nodes(mt)
    has = pre[1][:, 0] != 0
    v, bv = ref64.grid_update64(pre[1][has, 0], pre[1][has, 1:4], dt, G)
    _report(path + " grid_update v", ref64.check_particles(post[1][has, 1:4], v, bv, path + " grid update"))
    assert (post[1][~has] == 0).all()
    vsq = (post[1][has, 1:4] ** 2).sum(1).max()
    assert abs(float(mx.item()) - vsq) <= 4 * ref64.U * vsq
    return post, has


def _g2p_checked(path, grid, has, before, after, dt, model):
    """the G2P half: x, v, C (when stored), F (every solid: the stored F is the unprojected (I + dt C) F) / J (the fluid) of `after`
    from `before`'s x, F and the node velocities `grid`"""
    r = ref64.g2p64((grid[0], grid[1][:, 1:4]), before["x"], DX, dt, F=before["F"] if model != 4 else None,
                    J=before["F"][:, 0] if model == 4 else None)
    out = [ref64.check_particles(after["x"], r["x"], r["b_x"], path + " x")]
    if "v" in after:
        out += [ref64.check_particles(after["v"], r["v"], r["b_v"], path + " v"), ref64.check_particles(after["C"], r["C"], r["b_C"], path + " C")]
    if model != 4:
        out.append(ref64.check_particles(after["F"], r["F"], r["b_F"], path + " F"))
    if model == 4:
        out.append(ref64.check_particles(after["F"][:, 0], r["J"], r["b_J"], path + " J"))
    _report(path + " g2p", out)
    return r


# ------------------------------------------------------------------------------------------------ P2G, grid update, G2P
@pytest.mark.parametrize("cloud", ["lattice", "mixed", "edge"])
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("binned", [False, True])
def test_unfused_transfers_vs_ref64(pol, oracle, binned, model, side, cloud):
    """mt.p2g() with the stress computed inside P2G (particle order / reference-order binned kernels): all 7 channels node-local, the
    force of models 0-3 from the test entry's stress of the uploaded state (the fluid: channels 0-3), logJp after P2G against the
    entry's and F untouched; grid update and CFL max; mt.g2p(): x, v, C and F / J per particle"""
    _unfused(pol, binned, model, side, cloud, oracle)


@pytest.mark.parametrize("side,binned", [(8, True), (4, True), (8, False)])
def test_unfused_transfers_block_origin_keys_vs_ref64(pol, oracle, side, binned):
    """the same with the SparseGrid key convention (partition keys are block origins, key_is_origin=True), on the cloud that straddles 0"""
    _unfused(pol, binned, 0, side, "edge", oracle, key_is_origin=True)


def _unfused(pol, binned, model, side, cloud, oracle, key_is_origin=False):
    from zpc_amd.mpm import MpmTransfer
    dt = 1e-4
    mass, pos, vel, Cm, F = _cloud(cloud)
    n = pos.shape[0]
    F, lj = _state(model, F, n)
    mt = MpmTransfer(pol, n, DX, dt, model=model, side=side, volume=DX ** 3 / 8, key_is_origin=key_is_origin, **_kw(model))
    mt.upload(mass, pos, vel, Cm, F, lj if model in (1, 3) else None)
    mt.build_partition(n)
    if key_is_origin:
        assert (mt.active_keys() % side == 0).all()
    if binned:
        mt.rebin()
    before = _fields(_read_all(mt), mt)
    mt.clear_grid()
    mt.p2g()
    pol.syncCtx()
    path = "p2g[%s m%d s%d %s%s]" % ("binned" if binned else "particle", model, side, cloud, " origin-keys" if key_is_origin else "")
    if model == 4:
        ref = ref64.p2g64(before["m"], before["x"], before["v"], before["C"], DX, dt)
        _report(path, ref64.check_grid(ref, ref64.to_world_nodes(mt), range(4), path))
    else:   # the stress of the uploaded state: P2G stores the new logJp and nothing else
        stored = _fields(_read_all(mt), mt)
        assert all(np.array_equal(stored[k], before[k]) for k in ("m", "x", "v", "C", "F")), path + ": P2G changed more than logJp"
        sc = _checker(pol, oracle, mt, dt)
        res = sc.constitutive(path, before["F"], before.get("logJp"), stored.get("logJp"))
        sc.force(path, ref64.to_world_nodes(mt), before["m"], before["x"], before["v"], before["C"], res.PF, res.ePF)
    grid, has = _grid_update_checked(mt, path, dt)
    mt.g2p()
    pol.syncCtx()
    _g2p_checked(path, grid, has, before, _fields(_read_all(mt), mt), dt, model)


@pytest.mark.parametrize("cloud", ["lattice", "mixed", "edge"])
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("variant", ["tile_merged", "tile_separate_bases", "wide_32_lanes"])
@pytest.mark.parametrize("model", [0, 1])
def test_cached_stress_p2g_vs_ref64(pol, model, variant, side, cloud):
    """The three cached-stress P2G kernels behind zs_rocm_mpm_p2g: all 7 channels, the force from the P F^T vol read back from the
    particles (the 6 components the kernel reads), on a cloud a sixth of whose inner particles moved after it was binned (in-bin movers:
    the LDS post-pass; out-of-bin movers: the exact path)"""
    from zpc_amd.mpm import MpmTransfer, Particles
    dt = 1e-4
    mass, pos, vel, Cm, F = _cloud(cloud)
    n = pos.shape[0]
    F, lj = _state(model, F, n)
    mt = MpmTransfer(pol, n, DX, dt, model=model, side=side, volume=DX ** 3 / 8, cache_stress=True,
                     lane_width=32 if variant == "wide_32_lanes" else 64)
    mt.upload(mass, pos, vel, Cm, F, lj if model == 1 else None)
    mt.build_partition(n)
    mt.rebin()
    mt.update_stress()
    _, moved = move_after_binning(mt, pos)
    assert moved.any()
    parts = mt.particles()
    if variant == "tile_separate_bases":
        other = mt.buf.clone()
        parts = Particles(mt._port("m", other), parts.pos, parts.vel, parts.C, parts.F, parts.logJp, parts.stress, parts.n)
    before = _fields(_read_all(mt), mt)
    mt.clear_grid()
    __import__("zpc_amd").lib().zs_rocm_mpm_p2g(pol.handle, C.byref(mt.params), parts, mt.table.handle, mt.grid.data_ptr(), mt.nblocks,
                                                mt.bin_start.data_ptr(), mt.cell_count.data_ptr(), mt.nbr.data_ptr())
    pol.syncCtx()
    path = "p2g[%s m%d s%d %s]" % (variant, model, side, cloud)
    ref = ref64.p2g64(before["m"], before["x"], before["v"], before["C"], DX, dt, PF=before["PF"])
    _report(path, ref64.check_grid(ref, ref64.to_world_nodes(mt), range(7), path))


def test_light_particle_mass_change_is_rejected_on_device_data(pol):
    """GPU-side negative control: against a real GPU grid (mixed-mass cloud, binned P2G), a reference built with one particle of the
    1e-3 m slab 1 % heavier is rejected, while the true reference passes"""
    from zpc_amd.mpm import MpmTransfer
    dt = 1e-4
    mass, pos, vel, Cm, F = make_mixed_cloud(6, DX)
    n = pos.shape[0]
    mt = MpmTransfer(pol, n, DX, dt, model=0, side=4, volume=DX ** 3 / 8)
    mt.upload(mass, pos, vel, Cm, F)
    mt.build_partition(n)
    mt.clear_grid()
    mt.p2g()
    pol.syncCtx()
    world = ref64.to_world_nodes(mt)
    ref64.check_grid(ref64.p2g64(mass, pos, vel, Cm, DX, dt), world, range(4))
    light = np.nonzero((mass < 2e-3 * mass.max()) & (mass > 2e-4 * mass.max()))[0]
    j = light[np.argmin(np.abs(pos[light] - np.median(pos[light], 0)).sum(1))]
    m2 = mass.copy()
    m2[j] *= np.float32(1.01)
    with pytest.raises(AssertionError):
        ref64.check_grid(ref64.p2g64(m2, pos, vel, Cm, DX, dt), world, range(4))


# ------------------------------------------------------------------------------------------------ fused steps
def _step_stress(path, sc, mt, lj_before, after, write_all, paths):
    """(PF, ePF) for the force of a step that computed the stress itself, from the stored state `after` and the logJp before the step.
    The fluid: the closed form from the stored J (to rounding: ref64.eos_pf64).  Models 0-3: the test entry's stress of (stored F,
    previous logJp) with the stress tolerance (ref64_step.StepCheck.constitutive: the stored logJp against the entry's, per store path;
    the entry against float64 on these states).  With write_all the stored (packed) stress is the one the scatter used, up to the
    symmetrisation of stress_pack: asserted against the fluid's closed form / stress_pack of the entry's within the same tolerance."""
    if sc.model == 4:
        assert mt.params.viscosity == 0
        PF, ePF = ref64.eos_pf64(after["F"][:, 0], mt.params.bulk, mt.params.volume)
        if write_all:
            assert (np.abs(after["PF"] - PF) <= ePF).all(), np.abs(after["PF"] - PF).max()
        return PF, ePF
    res = sc.constitutive(path, after["F"], lj_before, after.get("logJp"), S6=after["S6"] if write_all else None, paths=paths)
    return res.PF, res.ePF


def _fc_oracle_stress(om, after, write_all):
    """(PF, ePF) of FixedCorotated from the oracle's stress of the stored F with the stress tolerance; with write_all the stored
    (packed) stress is the one the scatter used, up to the symmetrisation of stress_pack"""
    PF = oracle_stress(om.o, om, None, after["F"])
    ePF = _stress_tol(om, PF, after["F"])
    if write_all:
        assert (np.abs(after["PF"] - PF) <= ePF).all(), np.abs(after["PF"] - PF).max()
    return PF, ePF


def _p2g_half(path, sc, mt, om, before, after, r, write_all, dt, taken, channels=range(7)):
    """the P2G half of a fused step: mass from the stored x; momentum from the stored v, C (write_all) or from g2p64's with their bounds;
    force from _step_stress on `channels`, and with write_all once more from the six stored components (to rounding but for the
    symmetrisation: the same tolerance, its gap reported on its own).  FixedCorotated keeps its earlier check against the oracle's
    stress of the stored F as well.  taken [4]: counts the particles per store path, and those of the last path
    that also left their side^3 block."""
    if write_all:
        v, Cm, ev, eC = after["v"], after["C"], None, None
    else:
        v, Cm, ev, eC = r["v"], r["C"], r["b_v"], r["b_C"]
    paths, left_block = st.store_paths(before["x"], after["x"], DX, mt.side)
    taken[:3] += np.bincount(paths, minlength=3)
    taken[3] += int(left_block.sum())
    PF, ePF = _step_stress(path, sc, mt, before.get("logJp"), after, write_all, paths)
    world = ref64.to_world_nodes(mt)
    ref, _, _ = sc.force(path, world, after["m"], after["x"], v, Cm, PF, ePF, ev=ev, eC=eC, channels=channels, what="p2g")
    if sc.model == 0:
        PFo, ePFo = _fc_oracle_stress(om, after, write_all)
        sc.force(path, world, after["m"], after["x"], v, Cm, PFo, ePFo, ev=ev, eC=eC, channels=channels, what="p2g (oracle's stress)")
    if write_all and sc.model != 4:
        sc.force(path, world, after["m"], after["x"], v, Cm, after["PF"], ePF, channels=[4, 5, 6], what="force from the stored stress")
    return ref


@pytest.mark.parametrize("cloud", ["lattice", "edge_moving"])
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["write_all", "product", "reorder"])
def test_fused_compact_steps_vs_ref64(pol, oracle, mode, model, side, cloud):
    """zs_rocm_mpm_g2p2g on compact binned storage (write_all on and off) and the re-ordering step: three steps, each one's G2P half
    from the grid and particles downloaded before it, its P2G half (all 7 channels), logJp and stored stress from what it stored"""
    from zpc_amd.mpm import MpmTransfer
    dt = 1e-3
    mass, pos, vel, Cm, F = _cloud(cloud)
    n = pos.shape[0]
    F, lj = _state(model, F, n)
    om = OracleMpm(oracle, model, DX, dt, side, DX ** 3 / 8, **_kw(model))
    mt = MpmTransfer(pol, n, DX, dt, model=model, side=side, volume=DX ** 3 / 8, cache_stress=True, **_kw(model))
    mt.upload(mass, pos, vel, Cm, F, lj if model in (1, 3) else None)
    mt.build_partition(n, margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    sc = _checker(pol, oracle, mt, dt)
    taken = np.zeros(4, int)
    for step in range(st.FUSED_STEPS):
        grid, has = _grid_update_checked(mt, "fused[%s m%d s%d %s] step %d" % (mode, model, side, cloud, step), dt)
        before = _by_mass(_fields(_read_all(mt), mt))
        wa = mode == "write_all"
        mt.g2p2g(write_all=wa, reorder=mode == "reorder")
        pol.syncCtx()
        after = _by_mass(_fields(_read_all(mt), mt))
        assert np.array_equal(after["m"], before["m"])
        if not wa:
            del after["v"], after["C"]
        path = "fused[%s m%d s%d %s] step %d" % (mode, model, side, cloud, step)
        r = _g2p_checked(path, grid, has, before, after, dt, model)
        _p2g_half(path, sc, mt, om, before, after, r, wa, dt, taken)
    _paths_taken("fused[%s m%d s%d %s]" % (mode, model, side, cloud), taken, cloud, model)


def _paths_taken(path, taken, cloud, model):
    """on a moving cloud every plastic case has particles on each of the three store paths"""
    print("REF64 step %s store paths %s" % (path, dict(zip(st.PATHS + ("of them left the block",), taken.tolist()))))
    if cloud in st.MOVING and model in st.PLASTIC:
        assert (taken[:3] > 0).all(), taken


@pytest.mark.parametrize("cloud,side,model", st.SLOTTED_CASES)
def test_slotted_steps_vs_ref64(pol, oracle, cloud, side, model):
    """Slotted storage: g2p2g_slotblk_kernel (side 8, per 8^3 block) and g2p2g_slot_kernel (side 4, per bin), write_all off (the product
    instantiation) and on in turn over four steps of a moving cloud, then two whole steps behind zs_rocm_mpm_step_slotted, whose grid
    comes back updated: its mass and force channels against the P2G reference, its velocities against grid_update64 with the P2G bounds
    propagated.  Every step: logJp and (write_all) the stored stress against the test entry's, per store path.  Particles are matched by
    their identity-tagged mass."""
    from zpc_amd.mpm import MpmTransfer
    dt = 1e-3
    mass, pos, vel, Cm, F = _cloud(cloud)
    n = pos.shape[0]
    F, lj = _state(model, F, n)
    om = OracleMpm(oracle, model, DX, dt, side, DX ** 3 / 8, **_kw(model))
    mt = MpmTransfer(pol, n, DX, dt, model=model, side=side, volume=DX ** 3 / 8, cache_stress=True, **_kw(model))
    mt.upload(mass, pos, vel, Cm, F, lj if model in (1, 3) else None)
    mt.build_partition(n, margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update(G)
    mt.slot(K=32, outbox_cap=512)
    sc = _checker(pol, oracle, mt, dt)
    taken = np.zeros(4, int)
    moved = 0
    for step in range(st.SLOTTED_STEPS):
        path = "slotted[%s s%d m%d] step %d" % (cloud, side, model, step)
        grid = ref64.to_world_nodes(mt)
        has = grid[1][:, 0] != 0
        before = _by_mass(_fields(_read_all(mt), mt))
        wa = step % 2 == 1
        if step < 4:
            mt.g2p2g(write_all=wa)
        else:
            mt.step_slotted(G, write_all=wa)
        pol.syncCtx()
        mt.check_slots()
        after = _by_mass(_fields(_read_all(mt), mt))
        assert np.array_equal(after["m"], before["m"])
        moved += int((ref64.arena32(after["x"], DX)[0] != ref64.arena32(before["x"], DX)[0]).any(1).sum())
        if not wa:
            del after["v"], after["C"]
        r = _g2p_checked(path, grid, has, before, after, dt, model)
        if step < 4:
            _p2g_half(path, sc, mt, om, before, after, r, wa, dt, taken)
            mt.grid_update(G)
            continue
        # step_slotted: the grid is updated in the same call (channels 1-3 become velocities; mass and force stay)
        ref = _p2g_half(path, sc, mt, om, before, after, r, wa, dt, taken, channels=[0, 4, 5, 6])
        world = ref64.to_world_nodes(mt)
        vg, bv = ref64.grid_update64(ref.val[:, 0], ref.val[:, 1:4], dt, G, ref.bound()[:, 0], ref.bound()[:, 1:4])
        rows = ref.lookup(world[0])
        sel = rows >= 0
        sel[sel] = ref.val[rows[sel], 0] > 0
        _report(path + " step v", ref64.check_particles(world[1][sel, 1:4], vg[rows[sel]], bv[rows[sel]], path + " v"))
    assert moved > n // 4, moved
    _paths_taken("slotted[%s s%d m%d]" % (cloud, side, model), taken, cloud, model)


@pytest.mark.parametrize("write_all", [False, True])
def test_slotted_full_destination_cell_keeps_movers_contributions(pol, oracle, write_all):
    """The same-block full-destination case of test_slot_block_movers_gpu.py: the four movers keep their old slots, but the step's grid
    holds their contributions from their NEW positions, node by node (write_all off: the product instantiation)"""
    from zpc_amd.mpm import MpmTransfer
    dt, side, K = 1e-3, 8, 8
    mass, pos, vel, Cm, F = make_full_cell_cloud(DX, K)
    n = pos.shape[0]
    om = OracleMpm(oracle, 0, DX, dt, side, DX ** 3 / 8)
    mt = MpmTransfer(pol, n, DX, dt, model=0, side=side, volume=DX ** 3 / 8, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, None)
    mt.build_partition(n, margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update(G)
    mt.slot(K=K, outbox_cap=64)
    grid = ref64.to_world_nodes(mt)
    has = grid[1][:, 0] != 0
    before = _by_mass(_fields(_read_all(mt), mt))
    mt.g2p2g(write_all=write_all)
    pol.syncCtx()
    status = mt.check_slots(strict=False)
    assert status[1], "the destination cell was not full: the test does not test"
    after = _by_mass(_fields(_read_all(mt), mt))
    assert (ref64.arena32(after["x"], DX)[0][:, 0] == 36).all()
    if not write_all:
        del after["v"], after["C"]
    path = "full_cell[write_all %d]" % write_all
    r = _g2p_checked(path, grid, has, before, after, dt, 0)
    _p2g_half(path, _checker(pol, oracle, mt, dt), mt, om, before, after, r, write_all, dt, np.zeros(4, int))
