"""Every particle <-> grid transfer path of the C ABI against the float64 reference of tests/ref64.py, node by node and particle by
particle, each fed with inputs the GPU itself produced (its grid before a step, its stored particle state after it).  The bound of every
value is its own ((N + c) u T + e_in, see ref64), so a free-surface node, a node where momentum cancels or a lost low-weight term cannot
hide under the channel maximum.  The channel-max checks of the other modules stay as a second, coarser check.

Force channels: where the kernel read the cached P F^T vol, the test reads the same 6 components back (mt.off["PF"]) and the force is
checked to rounding.  Where the step computed the stress itself (stress inside P2G, the fused steps), the force is checked against the
oracle's stress of the stored state with the stress tolerance of test_svd_and_stress_blocks (1e-4 of the row scale) as e_in, and only
for FixedCorotated, whose F is stored unprojected.  That tolerance is kernel against oracle, the same algorithm in the same precision; how
far both are from the float64 stress (up to 1e-2 of the scale away from F = I), and the kernels' own stress sample by sample on every
model and branch, is the subject of tests/ref64_stress.py and tests/test_stress_ref64_gpu.py.  With write_all the stored stress is stress_pack of the 9-component PF the scatter
used; its symmetric part is compared with the oracle's under the same tolerance (the off-diagonal pairs differ by the SVD's rounding,
not by a multiple of u).  Prints one `REF64 <path> <worst err/bound per channel>` line per check."""
import ctypes as C

import numpy as np
import pytest

import ref64
from util import rng, make_cloud, make_mixed_cloud, make_edge_cloud, make_drifting_cloud, make_uneven_cloud, make_full_cell_cloud, \
    move_after_binning, tag_masses, OracleMpm, oracle_stress, stress_tol as _stress_tol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DX = 1.0 / 64
G = (0.0, -9.8, 0.0)


def _kw(model):
    return dict(yield_stress=200.0) if model == 2 else dict(beta=0.5) if model == 3 else {}


def _cloud(name):
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


def _state(model, F, n):
    if model == 4:
        J = (1.0 + 0.01 * rng(11).standard_normal(n)).astype(np.float32)
        return J[:, None], (0.01 * rng(33).standard_normal(n)).astype(np.float32)
    return F, (0.01 * rng(33).standard_normal(n)).astype(np.float32)


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
    if "PF" in mt.off:
        S = a[:, mt.off["PF"]:mt.off["PF"] + 6]
        out["PF"] = S[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
    return out


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
    """the G2P half: x, v, C (when stored), F / J (models 0, 4) of `after` from `before`'s x, F and the node velocities `grid`"""
    r = ref64.g2p64((grid[0], grid[1][:, 1:4]), before["x"], DX, dt, F=before["F"] if model == 0 else None,
                    J=before["F"][:, 0] if model == 4 else None)
    out = [ref64.check_particles(after["x"], r["x"], r["b_x"], path + " x")]
    if "v" in after:
        out += [ref64.check_particles(after["v"], r["v"], r["b_v"], path + " v"), ref64.check_particles(after["C"], r["C"], r["b_C"], path + " C")]
    if model == 0:
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
def test_unfused_transfers_vs_ref64(pol, binned, model, side, cloud):
    """mt.p2g() with the stress computed inside P2G (particle order / reference-order binned kernels): channels 0-3 node-local (4-6 stay
    with the oracle checks of test_mpm_gpu.py); grid update and CFL max; mt.g2p(): x, v, C and F / J (models 0, 4) per particle"""
    _unfused(pol, binned, model, side, cloud)


@pytest.mark.parametrize("side,binned", [(8, True), (4, True), (8, False)])
def test_unfused_transfers_block_origin_keys_vs_ref64(pol, side, binned):
    """the same with the SparseGrid key convention (partition keys are block origins, key_is_origin=True), on the cloud that straddles 0"""
    _unfused(pol, binned, 0, side, "edge", key_is_origin=True)


def _unfused(pol, binned, model, side, cloud, key_is_origin=False):
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
    ref = ref64.p2g64(before["m"], before["x"], before["v"], before["C"], DX, dt)
    _report(path, ref64.check_grid(ref, ref64.to_world_nodes(mt), range(4), path))
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
def _step_stress(mt, om, after, Cm, model, write_all):
    """(PF, ePF, channels) for the force of a step that computed the stress itself: the fluid's closed form from the stored J (to
    rounding: ref64.eos_pf64); FixedCorotated's from the oracle's stress of the stored F with the stress tolerance; no force check for
    the plastic models (their stored F is the unprojected one)"""
    if model == 4:
        assert mt.params.viscosity == 0
        PF, ePF = ref64.eos_pf64(after["F"][:, 0], mt.params.bulk, mt.params.volume)
    elif model == 0:
        PF = oracle_stress(om.o, om, Cm, after["F"])
        ePF = _stress_tol(om, PF, after["F"])
    else:
        return None, None, range(4)
    if write_all:   # the stored (packed) stress is the one the scatter used, up to the symmetrisation of stress_pack
        assert (np.abs(after["PF"] - PF) <= ePF).all(), np.abs(after["PF"] - PF).max()
    return PF, ePF, range(7)


def _p2g_half(path, mt, om, after, r, write_all, model, dt):
    """the P2G half of a fused step: mass from the stored x; momentum from the stored v, C (write_all) or from g2p64's with their bounds;
    force from _step_stress"""
    if write_all:
        v, Cm, ev, eC = after["v"], after["C"], None, None
    else:
        v, Cm, ev, eC = r["v"], r["C"], r["b_v"], r["b_C"]
    PF, ePF, ch = _step_stress(mt, om, after, Cm, model, write_all)
    ref = ref64.p2g64(after["m"], after["x"], v, Cm, DX, dt, PF=PF, ev=ev, eC=eC, ePF=ePF)
    _report(path + " p2g", ref64.check_grid(ref, ref64.to_world_nodes(mt), ch, path))
    return ref


@pytest.mark.parametrize("cloud", ["lattice", "edge_moving"])
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 4])
@pytest.mark.parametrize("mode", ["write_all", "product", "reorder"])
def test_fused_compact_steps_vs_ref64(pol, oracle, mode, model, side, cloud):
    """zs_rocm_mpm_g2p2g on compact binned storage (write_all on and off) and the re-ordering step: three steps, each one's G2P half
    from the grid and particles downloaded before it, its P2G half from the positions it stored"""
    from zpc_amd.mpm import MpmTransfer
    dt = 1e-3
    mass, pos, vel, Cm, F = _cloud(cloud)
    n = pos.shape[0]
    F, lj = _state(model, F, n)
    om = OracleMpm(oracle, model, DX, dt, side, DX ** 3 / 8)
    mt = MpmTransfer(pol, n, DX, dt, model=model, side=side, volume=DX ** 3 / 8, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, lj if model == 1 else None)
    mt.build_partition(n, margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    for step in range(3):
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
        _p2g_half(path, mt, om, after, r, wa, model, dt)


@pytest.mark.parametrize("cloud,side,model", [("drifting", 8, 1), ("drifting", 8, 0), ("drifting", 4, 0), ("edge_moving", 8, 0),
                                              ("edge_moving", 4, 1), ("uneven", 8, 1), ("uneven", 4, 0)])
def test_slotted_steps_vs_ref64(pol, oracle, cloud, side, model):
    """Slotted storage: g2p2g_slotblk_kernel (side 8, per 8^3 block) and g2p2g_slot_kernel (side 4, per bin), write_all off (the product
    instantiation) and on in turn over four steps of a moving cloud, then two whole steps behind zs_rocm_mpm_step_slotted, whose grid
    comes back updated: its mass channel (and for FixedCorotated its force channels) against the P2G reference, its velocities against
    grid_update64 with the P2G bounds propagated.  Particles are matched by their identity-tagged mass."""
    from zpc_amd.mpm import MpmTransfer
    dt = 1e-3
    mass, pos, vel, Cm, F = _cloud(cloud)
    n = pos.shape[0]
    F, lj = _state(model, F, n)
    om = OracleMpm(oracle, model, DX, dt, side, DX ** 3 / 8)
    mt = MpmTransfer(pol, n, DX, dt, model=model, side=side, volume=DX ** 3 / 8, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, lj if model == 1 else None)
    mt.build_partition(n, margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update(G)
    mt.slot(K=32, outbox_cap=512)
    moved = 0
    for step in range(6):
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
            _p2g_half(path, mt, om, after, r, wa, model, dt)
            mt.grid_update(G)
            continue
        # step_slotted: the grid is updated in the same call (channels 1-3 become velocities; mass and force stay)
        v, Cm_, ev, eC = (after["v"], after["C"], None, None) if wa else (r["v"], r["C"], r["b_v"], r["b_C"])
        PF, ePF, ch = _step_stress(mt, om, after, Cm_, model, wa)
        ref = ref64.p2g64(after["m"], after["x"], v, Cm_, DX, dt, PF=PF, ev=ev, eC=eC, ePF=ePF)
        world = ref64.to_world_nodes(mt)
        _report(path + " step m, force", ref64.check_grid(ref, world, [c for c in ch if c == 0 or c >= 4], path))
        vg, bv = ref64.grid_update64(ref.val[:, 0], ref.val[:, 1:4], dt, G, ref.bound()[:, 0], ref.bound()[:, 1:4])
        rows = ref.lookup(world[0])
        sel = rows >= 0
        sel[sel] = ref.val[rows[sel], 0] > 0
        _report(path + " step v", ref64.check_particles(world[1][sel, 1:4], vg[rows[sel]], bv[rows[sel]], path + " v"))
    assert moved > n // 4, moved


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
    st = mt.check_slots(strict=False)
    assert st[1], "the destination cell was not full: the test does not test"
    after = _by_mass(_fields(_read_all(mt), mt))
    assert (ref64.arena32(after["x"], DX)[0][:, 0] == 36).all()
    if not write_all:
        del after["v"], after["C"]
    path = "full_cell[write_all %d]" % write_all
    r = _g2p_checked(path, grid, has, before, after, dt, 0)
    _p2g_half(path, mt, om, after, r, write_all, 0, dt)
