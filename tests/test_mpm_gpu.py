"""GPU parity for the MPM transfer path vs the CPU oracle (restated reference functors).

Tolerances (stated per north_star): the SVD/stress building blocks agree to 2e-5 relative to the stress
scale (2*mu + lambda)*vol (float rounding of sigma-1 near F = I is amplified by mu); P2G grid sums to
rel 2e-4 of the per-channel magnitude (float atomics: order-dependent sums); G2P to rel 2e-5."""
import ctypes as C

import numpy as np
import pytest

from util import rng, make_cloud, make_uneven_cloud, move_after_binning, OracleMpm, ptr, YIELD_SURFACE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_svd_and_stress_blocks(pol, oracle):
    import zpc_amd as zs
    from zpc_amd import MpmParams
    g = rng(30)
    n = 20000
    F = (np.eye(3).reshape(1, 9) + 0.2 * g.standard_normal((n, 9))).astype(np.float32)
    dF = torch.from_numpy(F).cuda()
    U, S, V = (torch.empty(n, 9, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, 9, device="cuda"))
    zs.lib().zs_rocm_svd3(pol.handle, dF.data_ptr(), n, U.data_ptr(), S.data_ptr(), V.data_ptr())
    Uh, Sh, Vh = U.cpu().numpy(), S.cpu().numpy(), V.cpu().numpy()
    Sref = np.zeros((n, 3), np.float32)
    Uref, Vref = np.zeros((n, 9), np.float32), np.zeros((n, 9), np.float32)
    for i in range(n):
        oracle.orc_svd3(ptr(F[i]), ptr(Uref[i]), ptr(Sref[i]), ptr(Vref[i]))
    assert np.abs(Sh - Sref).max() < 2e-5 * max(1.0, np.abs(Sref).max())
    Um, Vm = Uh.reshape(n, 3, 3).transpose(0, 2, 1), Vh.reshape(n, 3, 3).transpose(0, 2, 1)
    assert np.abs(np.einsum("nij,nkj->nik", Um, Um) - np.eye(3)).max() < 1e-5   # U orthonormal
    assert np.abs(np.einsum("nij,nkj->nik", Vm, Vm) - np.eye(3)).max() < 1e-5
    assert (np.linalg.det(Um) > 0).all() and (np.linalg.det(Vm) > 0).all()     # rotations (math::svd convention)
    # U diag(S) V^T = F and |S0| >= |S1| >= |S2| against float64 (ref64_stress): the reconstruction within twice the oracle's own error
    # on this input (the 4-sweep truncation error, 2.5e-3 of ||F||_2 here: far above rounding), the order up to each sample's S error
    import ref64_stress
    eg, eo = ref64_stress.svd_errors(F, Uh, Sh, Vh), ref64_stress.svd_errors(F, Uref, Sref, Vref)
    assert eg["recon"].max() <= 2 * eo["recon"].max(), (eg["recon"].max(), eo["recon"].max())
    assert (eg["order"] <= 2 * eg["S"] + 4 * ref64_stress.U32).all(), eg["order"].max()
    # stress: fixed corotated + sand
    mu, lam = 0.5 * 5e4 / 1.4, 5e4 * 0.4 / (1.4 * 0.2)
    oracle.orc_nacc_bulk.restype = C.c_float
    oracle.orc_nacc_msqr.restype = C.c_float
    bm, msqr = oracle.orc_nacc_bulk(C.c_float(5e4), C.c_float(0.4)), oracle.orc_nacc_msqr(C.c_float(45.0))
    assert zs.lib().zs_rocm_nacc_msqr(45.0) == msqr
    for model in (0, 1, 2, 3):
        # von Mises: yield stress 500 (part of the cloud yields); NACC: beta 0.5, xi 0.8, hardening on
        p = MpmParams(model, 1 / 64, 1e-4, 2.5e-7, 5e4, 0.4, 0.0, 0.5 if model == 3 else 1.0, YIELD_SURFACE, 1, 4, 0, 500.0, 0.8, msqr, 1)
        Fd = dF.clone()
        lj = torch.from_numpy((0.01 * g.standard_normal(n)).astype(np.float32)).cuda()
        lj0 = lj.cpu().numpy().copy()
        PF = torch.empty(n, 9, device="cuda")
        zs.lib().zs_rocm_mpm_stress(pol.handle, C.byref(p), Fd.data_ptr(), lj.data_ptr(), n, PF.data_ptr())
        PFh = PF.cpu().numpy()
        ref = np.zeros((n, 9), np.float32)
        Fo = F.copy()
        ljo = lj0.copy()
        cf = C.c_float
        for i in range(n):
            if model == 0:
                oracle.orc_stress_fixedcorotated(cf(2.5e-7), cf(mu), cf(lam), ptr(Fo[i]), ptr(ref[i]))
            elif model == 2:  # hostVariant 0 = the CUDA header's arithmetic (sqrtf), which the GPU path follows
                oracle.orc_stress_vonmises(cf(2.5e-7), cf(mu), cf(lam), cf(500.0), 0, ptr(Fo[i]), ptr(ref[i]))
            else:
                l = cf(ljo[i])
                if model == 1:
                    oracle.orc_stress_sand(cf(2.5e-7), cf(mu), cf(lam), cf(0.0), cf(1.0), cf(YIELD_SURFACE), 1, C.byref(l), ptr(Fo[i]), ptr(ref[i]))
                else:
                    oracle.orc_stress_nacc(cf(2.5e-7), cf(mu), cf(lam), cf(bm), cf(0.8), cf(0.5), cf(msqr), 1, 0, C.byref(l), ptr(Fo[i]), ptr(ref[i]))
                ljo[i] = l.value
        scale = (2 * mu + lam) * 2.5e-7
        rowmag = np.maximum(np.abs(ref).max(1, keepdims=True), scale * max(1.0, np.abs(F - np.eye(3).reshape(1, 9)).max()))
        ok = np.isfinite(ref).all(1)  # von Mises: a negative discriminant gives NaN in the CUDA header (sqrtf), on both sides
        assert ok.mean() > 0.5 and np.array_equal(np.isfinite(PFh).all(1), ok), model
        assert (np.abs(PFh - ref)[ok] <= 1e-4 * rowmag[ok]).all(), (model, (np.abs(PFh - ref)[ok] / rowmag[ok]).max())
        if model != 0:
            assert np.abs(Fd.cpu().numpy() - Fo)[ok].max() < 5e-5, model          # projected F returned by the test entry
        if model in (1, 3):
            ljg = lj.cpu().numpy()
            fin = np.isfinite(ljo)  # NACC, inverted F: log of a negative volume ratio -> NaN, on both sides
            assert np.array_equal(np.isfinite(ljg), fin) and np.abs(ljg - ljo)[ok & fin].max() < 2e-5, model
        if model == 2:
            assert 0.05 < (np.abs(Fo - F).max(1) > 1e-6).mean() < 1.0             # some particles yield, in both implementations


def _compare_grids(ga, gb, rtol):
    assert set(ga.keys()) == set(gb.keys())
    A = np.stack([ga[k] for k in sorted(ga)])
    B = np.stack([gb[k] for k in sorted(ga)])
    for ch in range(7):
        s = np.abs(B[:, ch]).max() + 1e-30
        assert np.abs(A[:, ch] - B[:, ch]).max() <= rtol * s, (ch, np.abs(A[:, ch] - B[:, ch]).max() / s)


@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("binned", [False, True])
def test_p2g_g2p_vs_oracle(pol, oracle, side, model, binned):
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(9, dx, 2, seed=31 + side + model)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    lj0 = (0.01 * rng(33).standard_normal(n)).astype(np.float32)
    om = OracleMpm(oracle, model, dx, dt, side, vol, yield_stress=200.0, beta=0.5 if model == 3 else 1.0)
    nb_o = om.build_partition(pos, n)
    lj_o = om.p2g(mass, pos, vel, Cm, F, lj0.copy())

    mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, lane_width=64, yield_stress=200.0,
                     beta=0.5 if model == 3 else 1.0)
    mt.upload(mass, pos, vel, Cm, F, lj0 if model in (1, 3) else None)
    nb = mt.build_partition(n)
    assert nb == nb_o
    if binned:
        mt.rebin()
        bs = mt.bin_start.cpu().numpy()
        assert bs[0] == 0 and bs[-1] == n and (np.diff(bs) >= 0).all()
        cc = mt.cell_count.cpu().numpy().reshape(-1, 64)
        assert np.array_equal(cc.sum(1), np.diff(bs))
        assert np.array_equal(np.sort(mt.order.cpu().numpy()), np.arange(n))  # a permutation
    mt.clear_grid()
    mt.p2g()
    pol.syncCtx()
    # NACC: the hardening update takes the root of a nearly cancelling discriminant, its stress is the least well conditioned
    grtol = 5e-4 if model == 3 else 2e-4
    _compare_grids(mt.grid_by_key(), om.grid_by_key(), grtol)
    # conservation (size-independent property): total mass and momentum on the grid == particles
    g = np.stack(list(mt.grid_by_key().values()))
    assert abs(g[:, 0].sum() - mass.sum()) < 1e-4 * mass.sum()
    mom_p = (mass[:, None] * vel).sum(0)
    assert np.abs(g[:, 1:4].sum(axis=(0, 2)) - mom_p).max() < 2e-3 * np.abs(mass[:, None] * vel).sum()
    if model in (1, 3):
        d = mt.download()
        inv = mt.order.cpu().numpy() if binned else np.arange(n)
        assert np.abs(d["logJp"] - lj_o[inv]).max() < (2e-3 if model == 3 else 2e-5)
    # grid update + G2P
    mx = torch.zeros(1, dtype=torch.float32, device="cuda")
    mt.grid_update((0.0, -9.8, 0.0), mx)
    mxo = om.grid_update((0.0, -9.8, 0.0))
    assert abs(float(mx.item()) - mxo) <= 1e-4 * mxo
    _compare_grids(mt.grid_by_key(), om.grid_by_key(), grtol)
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    om.g2p(po, vo, Co, Fo)
    mt.g2p()
    pol.syncCtx()
    d = mt.download()
    inv = mt.order.cpu().numpy() if binned else np.arange(n)
    assert np.abs(d["x"] - po[inv]).max() < 1e-6
    assert np.abs(d["v"] - vo[inv]).max() < 2e-4 * np.abs(vo).max()
    assert np.abs(d["C"] - Co[inv]).max() < 2e-4 * np.abs(Co).max()
    assert np.abs(d["F"] - Fo[inv]).max() < 2e-5


def test_stale_bins_fall_back_exactly(pol, oracle):
    """Particles that left their bin since the last re-binning take the exact slow path: results unchanged."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=41)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    mt = MpmTransfer(pol, n, dx, dt, model=0, side=4, volume=vol)
    mt.upload(mass, pos, vel, Cm, F)
    mt.build_partition(n)
    mt.rebin()
    order = mt.order.cpu().numpy()
    # move 10 % of the particles by up to one cell AFTER binning (stay inside the partition's enlarged blocks)
    g = rng(42)
    pos2 = pos[order].copy()
    sel = g.random(n) < 0.1
    pos2[sel] += (g.random((sel.sum(), 3)).astype(np.float32) - 0.5) * dx * 1.2
    mt2 = MpmTransfer(pol, n, dx, dt, model=0, side=4, volume=vol)
    mt2.upload(mass[order], pos2, vel[order], Cm[order], F[order])
    mt2.table, mt2.nblocks, mt2.grid, mt2.nbr = mt.table, mt.nblocks, torch.zeros_like(mt.grid), mt.nbr
    mt2.bin_start, mt2.cell_count, mt2.binned = mt.bin_start, mt.cell_count, True
    mt2.p2g()
    pol.syncCtx()
    binned_grid = mt2.grid.cpu().numpy().copy()
    mt2.grid.zero_()
    mt2.p2g(binned=False)
    pol.syncCtx()
    ref_grid = mt2.grid.cpu().numpy()
    for ch in range(7):
        a = binned_grid.reshape(-1, 7, 64)[:, ch]
        b = ref_grid.reshape(-1, 7, 64)[:, ch]
        assert np.abs(a - b).max() <= 2e-4 * (np.abs(b).max() + 1e-30)


@pytest.mark.parametrize("side,binned", [(8, True), (4, True), (8, False)])
def test_sparsegrid_origin_keys(pol, oracle, side, binned):
    """SparseGrid convention (geometry/SparseGrid.hpp:305-309): partition keys are block ORIGINS (multiples of side)."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(9, dx, 2, seed=71, origin=(-0.05, 0.31, 0.29))  # straddles negative coordinates
    n = pos.shape[0]
    vol = dx ** 3 / 8
    om = OracleMpm(oracle, 0, dx, dt, side, vol)
    om.build_partition(pos, n)
    om.p2g(mass, pos, vel, Cm, F)
    mt = MpmTransfer(pol, n, dx, dt, model=0, side=side, volume=vol, key_is_origin=True)
    mt.upload(mass, pos, vel, Cm, F)
    assert mt.build_partition(n) == om.nblocks
    if binned:
        mt.rebin()
    mt.clear_grid()
    mt.p2g()
    pol.syncCtx()
    ga = {tuple(k // side for k in key): v for key, v in mt.grid_by_key().items()}
    assert all(all(c % side == 0 for c in key) for key in mt.grid_by_key())
    _compare_grids(ga, om.grid_by_key(), 2e-4)
    mt.grid_update((0.0, -9.8, 0.0))
    om.grid_update((0.0, -9.8, 0.0))
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    om.g2p(po, vo, Co, Fo)
    mt.g2p()
    pol.syncCtx()
    d = mt.download()
    inv = mt.order.cpu().numpy() if binned else np.arange(n)
    assert np.abs(d["v"] - vo[inv]).max() < 2e-4 * np.abs(vo).max()
    assert np.abs(d["F"] - Fo[inv]).max() < 2e-5


@pytest.mark.parametrize("binned", [False, True])
def test_aos_particles(pol, oracle, binned):
    """AoS attribute storage (zs::Particles: Vector<vec3>, Vector<vec9>, geometry/Structurefree.hpp:21-237) through the
    same iterator ports (numTileBits = tileMask = 0)."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=72)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    lj0 = (0.01 * rng(73).standard_normal(n)).astype(np.float32)
    om = OracleMpm(oracle, 1, dx, dt, 4, vol)
    om.build_partition(pos, n)
    lj_o = om.p2g(mass, pos, vel, Cm, F, lj0.copy())
    mt = MpmTransfer(pol, n, dx, dt, model=1, side=4, volume=vol, aos=True)
    aos = np.concatenate([mass[:, None], pos, vel, Cm, F, lj0[:, None]], axis=1).astype(np.float32)
    mt.buf.copy_(torch.from_numpy(aos.reshape(-1)).cuda())
    assert mt.build_partition(n) == om.nblocks
    if binned:
        mt.rebin()
    mt.clear_grid()
    mt.p2g()
    pol.syncCtx()
    _compare_grids(mt.grid_by_key(), om.grid_by_key(), 2e-4)
    mt.grid_update((0.0, -9.8, 0.0))
    om.grid_update((0.0, -9.8, 0.0))
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    om.g2p(po, vo, Co, Fo)
    mt.g2p()
    pol.syncCtx()
    out = mt.buf.cpu().numpy().reshape(n, 26)
    inv = mt.order.cpu().numpy() if binned else np.arange(n)
    assert np.abs(out[:, 1:4] - po[inv]).max() < 1e-6
    assert np.abs(out[:, 4:7] - vo[inv]).max() < 2e-4 * np.abs(vo).max()
    assert np.abs(out[:, 16:25] - Fo[inv]).max() < 2e-5
    assert np.abs(out[:, 25] - lj_o[inv]).max() < 2e-5


@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("variant", ["tile_merged", "tile_separate_bases", "wide_32_lanes"])
def test_cached_stress_p2g_kernel_variants_vs_oracle(pol, oracle, variant, side):
    """The stand-alone P2G with cached stress has three kernels behind zs_rocm_mpm_p2g: p2g_tile_kernel with m, x, v, C in 16 adjacent
    channels (4 + 2 tile requests), the same with one base per attribute (8 requests: here the mass port points into a second
    TileVector of the same layout), and p2g_wide_kernel for 32-lane tiles.  All three against the oracle's P2G (P2G.hpp:38-116), on a
    cloud whose particles have moved since it was binned (in-bin movers: LDS post-pass; out-of-bin movers: exact path)."""
    from zpc_amd.mpm import MpmTransfer, Particles
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(9, dx, 2, seed=57 + side)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    mt = MpmTransfer(pol, n, dx, dt, model=0, side=side, volume=vol, cache_stress=True, lane_width=32 if variant == "wide_32_lanes" else 64)
    mt.upload(mass, pos, vel, Cm, F)
    om = OracleMpm(oracle, 0, dx, dt, side, vol)
    assert mt.build_partition(n) == om.build_partition(pos, n)
    mt.rebin()
    mt.update_stress()
    # move a sixth of the cloud's inner particles by up to 1.2 cells AFTER binning (two cells from its faces: they stay inside the partition)
    pos2, moved = move_after_binning(mt, pos)
    assert moved.sum() > 100
    lib = __import__("zpc_amd").lib()
    parts = mt.particles()
    if variant == "tile_separate_bases":
        other = mt.buf.clone()   # same layout, another allocation: the mass port no longer sits 64 floats in front of x
        parts = Particles(mt._port("m", other), parts.pos, parts.vel, parts.C, parts.F, parts.logJp, parts.stress, parts.n)
    mt.clear_grid()
    lib.zs_rocm_mpm_p2g(pol.handle, C.byref(mt.params), parts, mt.table.handle, mt.grid.data_ptr(), mt.nblocks, mt.bin_start.data_ptr(),
                        mt.cell_count.data_ptr(), mt.nbr.data_ptr())
    pol.syncCtx()
    om.p2g(mass, pos2, vel, Cm, F)
    _compare_grids(mt.grid_by_key(), om.grid_by_key(), 2e-4)
    g = np.stack(list(mt.grid_by_key().values()))
    assert abs(g[:, 0].sum() - mass.sum()) < 1e-4 * mass.sum()


@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("side", [4, 8])
def test_cached_stress_matches_recompute_over_steps(pol, oracle, model, side):
    """Fusing the constitutive update into the tail of G2P (particles.stress) gives the same multi-step trajectory as the
    reference order (stress inside P2G), and both follow the CPU oracle over 3 sub-steps."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=81 + model)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    lj0 = (0.01 * rng(83).standard_normal(n)).astype(np.float32)
    om = OracleMpm(oracle, model, dx, dt, side, vol, yield_stress=200.0, beta=0.5 if model == 3 else 1.0)
    om.build_partition(pos, n)
    po, vo, Co, Fo, ljo = pos.copy(), vel.copy(), Cm.copy(), F.copy(), lj0.copy()
    runs = {}
    for cached in (False, True):
        mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=cached, yield_stress=200.0,
                         beta=0.5 if model == 3 else 1.0)
        mt.upload(mass, pos, vel, Cm, F, lj0 if model in (1, 3) else None)
        assert mt.build_partition(n) == om.nblocks
        mt.rebin()
        mt.update_stress()
        runs[cached] = mt
    for step in range(3):
        om.grid[:] = 0
        ljo = om.p2g(mass, po, vo, Co, Fo, ljo)
        om.grid_update((0.0, -9.8, 0.0))
        om.g2p(po, vo, Co, Fo)
        for mt in runs.values():
            mt.clear_grid()
            mt.p2g()
            mt.grid_update((0.0, -9.8, 0.0))
            mt.g2p()
    # the cached run has already evaluated the model for the NEXT P2G (logJp is one evaluation ahead by design): advance the
    # other two by one more constitutive update before comparing logJp
    om.grid[:] = 0
    ljo = om.p2g(mass, po, vo, Co, Fo, ljo)
    runs[False].clear_grid()
    runs[False].p2g()
    pol.syncCtx()

    def original_order(mt):  # binned storage -> original particle numbering (the rank inside a cell is race-ordered)
        d, order = mt.download(), mt.order.cpu().numpy()
        out = {}
        for k, v in d.items():
            o = np.empty_like(v)
            o[order] = v
            out[k] = o
        return out
    da, db = original_order(runs[False]), original_order(runs[True])
    for k, tol in (("x", 2e-6), ("v", 3e-4 * np.abs(vo).max()), ("F", 5e-5), ("C", 5e-4 * np.abs(Co).max())):
        assert np.abs(da[k] - db[k]).max() <= tol, k          # cached == recompute
        ref = {"x": po, "v": vo, "F": Fo, "C": Co}[k]
        assert np.abs(db[k] - ref).max() <= tol * 2, k         # both follow the oracle
    if model in (1, 3):
        assert np.abs(da["logJp"] - db["logJp"]).max() < 5e-5
        assert np.abs(db["logJp"] - ljo).max() < (2e-3 if model == 3 else 1e-4)   # NACC hardening: see test_p2g_g2p_vs_oracle


@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("side", [4, 8])
def test_fused_g2p2g_matches_unfused_steps(pol, oracle, model, side):
    """zs_rocm_mpm_g2p2g (G2P of step n + P2G of step n+1 in one pass, v / C / stress kept on chip) reproduces the unfused
    g2p -> clear -> p2g sequence: same grids after every step, same particle state at the end; with a velocity field that
    pushes particles across cell boundaries so that both exact-path queues are exercised."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-3
    # von Mises: the CUDA header takes sqrtf of a discriminant that turns negative under strong compression (NaN, "Wrong
    # projection"); keep that model's cloud gentle -- the cell-crossing particles are exercised by the other three models
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=91 + model, vel_scale=3.0 if model != 2 else 0.3)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    lj0 = (0.01 * rng(93).standard_normal(n)).astype(np.float32)
    runs = []
    for fused in (False, True):
        mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True, yield_stress=200.0,
                         beta=0.5 if model == 3 else 1.0)
        mt.upload(mass, pos, vel, Cm, F, lj0 if model in (1, 3) else None)
        mt.build_partition(n)
        mt.rebin()
        mt.update_stress()
        mt.clear_grid()
        mt.p2g()
        mt.grid_update((0.0, -9.8, 0.0))
        runs.append(mt)
    a, b = runs
    nsteps = 4
    for step in range(nsteps):
        last = step == nsteps - 1
        a.g2p()
        a.clear_grid()
        a.p2g()
        b.g2p2g(write_all=last)
        pol.syncCtx()
        ga, gb = a.grid_by_key(), b.grid_by_key()
        scale = np.abs(np.stack(list(ga.values()))).max(axis=(0, 2)) + 1e-30
        for k in list(ga.keys())[:: max(1, len(ga) // 300)]:
            assert (np.abs(ga[k] - gb[k]).max(axis=1) <= 3e-4 * scale).all(), (step, k)
        a.grid_update((0.0, -9.8, 0.0))
        b.grid_update((0.0, -9.8, 0.0))
    pol.syncCtx()

    def original_order(mt):
        d, order = mt.download(), mt.order.cpu().numpy()
        out = {}
        for k, v in d.items():
            o = np.empty_like(v)
            o[order] = v
            out[k] = o
        return out
    da, db = original_order(a), original_order(b)
    moved = np.abs(da["x"] - pos).max() / dx
    assert moved > (0.05 if model != 2 else 0.005)  # the cloud really moved (cells were crossed)
    for k, tol in (("x", 3e-6), ("v", 5e-4 * np.abs(da["v"]).max()), ("F", 1e-4), ("C", 1e-3 * np.abs(da["C"]).max())):
        assert np.abs(da[k] - db[k]).max() <= tol, k
    if model in (1, 3):
        assert np.abs(da["logJp"] - db["logJp"]).max() < 1e-4


@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("binned,cached", [(False, False), (True, False), (True, True)])
def test_equation_of_state_fluid_vs_oracle(pol, oracle, side, binned, cached):
    """EquationOfStateConfig (P2G.hpp:60-81, G2P.hpp:70-74): particles carry J instead of F; two sub-steps (P2G, grid update,
    G2P) against the oracle, through the particle-order path, the reference-order binned kernels and the cached-stress path;
    then the fused pass must agree with the unfused sequence."""
    from zpc_amd.mpm import MpmTransfer, EQUATION_OF_STATE
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=57 + side)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    J = (1.0 + 0.02 * rng(58).standard_normal(n)).astype(np.float32)
    om = OracleMpm(oracle, 4, dx, dt, side, vol, bulk=4e4, viscosity=0.05)
    om.build_partition(pos, n)
    Fo = np.zeros((n, 9), np.float32)
    Fo[:, 0] = J
    po, vo, Co = pos.copy(), vel.copy(), Cm.copy()
    mt = MpmTransfer(pol, n, dx, dt, model=EQUATION_OF_STATE, side=side, volume=vol, cache_stress=cached, bulk=4e4, viscosity=0.05)
    mt.upload(mass, pos, vel, Cm, J)
    mt.build_partition(n)
    if binned:
        mt.rebin()
    if cached:
        mt.update_stress()
    for step in range(2):
        om.grid[:] = 0
        om.p2g(mass, po, vo, Co, Fo)
        mt.clear_grid()
        mt.p2g()
        pol.syncCtx()
        _compare_grids(mt.grid_by_key(), om.grid_by_key(), 2e-4)
        om.grid_update((0.0, -9.8, 0.0))
        mt.grid_update((0.0, -9.8, 0.0))
        om.g2p(po, vo, Co, Fo)
        mt.g2p()
        pol.syncCtx()
        d = mt.download()
        inv = mt.order.cpu().numpy() if binned else np.arange(n)
        assert np.abs(d["x"] - po[inv]).max() < 2e-6
        assert np.abs(d["v"] - vo[inv]).max() < 3e-4 * np.abs(vo).max()
        assert np.abs(d["C"] - Co[inv]).max() < 5e-4 * np.abs(Co).max()
        assert np.abs(d["J"][:, 0] - Fo[inv, 0]).max() < 2e-6
    assert np.abs(Fo[:, 0] - J).max() > 1e-4        # J really evolved
    if cached:  # fused pass == p2g of the state above + grid update + g2p
        mt.clear_grid(); mt.p2g(); mt.grid_update((0.0, -9.8, 0.0))
        om.grid[:] = 0; om.p2g(mass, po, vo, Co, Fo); om.grid_update((0.0, -9.8, 0.0)); om.g2p(po, vo, Co, Fo)
        mt.g2p2g(write_all=True)
        pol.syncCtx()
        d = mt.download()
        inv = mt.order.cpu().numpy()
        assert np.abs(d["x"] - po[inv]).max() < 2e-6 and np.abs(d["J"][:, 0] - Fo[inv, 0]).max() < 2e-6
        assert np.abs(d["v"] - vo[inv]).max() < 3e-4 * np.abs(vo).max()
        om.grid[:] = 0; om.p2g(mass, po, vo, Co, Fo)
        _compare_grids(mt.grid_by_key(), om.grid_by_key(), 3e-4)


@pytest.mark.parametrize("model", [0, 1])
def test_inputs_only_rebin_between_fused_steps(pol, oracle, model):
    """rebin(inputs_only=True) moves only m, x, F, logJp (what a fused step reads); a fused run that re-bins this way in the
    middle ends in the same particle state (order-independent channel sums) and on the same grid as one that never re-bins."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=131 + model, vel_scale=3.0)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    lj0 = (0.01 * rng(132).standard_normal(n)).astype(np.float32)
    res = []
    for rebin_at in (None, 3):
        mt = MpmTransfer(pol, n, dx, dt, model=model, side=4, volume=vol, cache_stress=True)
        mt.upload(mass, pos, vel, Cm, F, lj0 if model == 1 else None)
        mt.build_partition(n)
        mt.rebin()
        mt.update_stress()
        mt.clear_grid(); mt.p2g(); mt.grid_update((0.0, -9.8, 0.0))
        for step in range(6):
            mt.g2p2g(write_all=(step == 5))
            mt.grid_update((0.0, -9.8, 0.0))
            if rebin_at == step:
                mt.buf2 = torch.full_like(mt.buf, float("nan"))   # whatever is not carried must not be read afterwards
                mt.rebin(inputs_only=True)
        pol.syncCtx()
        d = mt.download()
        assert mt.exact_path_particles() >= 0
        res.append((d, mt.grid_by_key()))
    (da, ga), (db, gb) = res
    for k in da:
        a, b = da[k].reshape(n, -1).astype(np.float64), db[k].reshape(n, -1).astype(np.float64)
        assert np.isfinite(b).all(), k
        scale = np.sqrt(n * (a ** 2).sum(0)) + 1e-30
        assert (np.abs(a.sum(0) - b.sum(0)) <= 2e-5 * scale).all(), k
        assert (np.abs((a ** 2).sum(0) - (b ** 2).sum(0)) <= 1e-4 * (a ** 2).sum(0) + 1e-30).all(), k
    _compare_grids(ga, gb, 3e-4)


@pytest.mark.parametrize("model,side", [(0, 4), (1, 8), (4, 4)])
def test_reordering_fused_step_matches_in_place_steps(pol, oracle, model, side):
    """g2p2g(reorder=True): every step bins the particles anew and carries them into that order (inputs through the
    permutation from the other buffer).  Six such steps of a fast cloud end in the same particle state (order-independent
    channel sums) and grid as six in-place fused steps, and put nothing on the exact path that started the step mis-binned."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=151 + model, vel_scale=3.0)
    n = pos.shape[0]
    vol = dx ** 3 / 8
    lj0 = (0.01 * rng(152).standard_normal(n)).astype(np.float32)
    state = (1.0 + 0.02 * rng(153).standard_normal(n)).astype(np.float32) if model == 4 else F
    res = []
    for reorder in (False, True):
        mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True, viscosity=0.05)
        mt.upload(mass, pos, vel, Cm, state, lj0 if model == 1 else None)
        mt.build_partition(n)
        mt.rebin()
        mt.update_stress()
        mt.clear_grid(); mt.p2g(); mt.grid_update((0.0, -9.8, 0.0))
        if reorder:
            mt.buf2 = torch.full_like(mt.buf, float("nan"))  # the step must fill everything it later reads
        for step in range(6):
            # the last step materialises v, C, stress for the comparison (a re-ordering step never does)
            mt.g2p2g(write_all=(step == 5), reorder=reorder and step < 5)
            mt.grid_update((0.0, -9.8, 0.0))
        pol.syncCtx()
        res.append((mt.download(), mt.grid_by_key(), mt.exact_path_particles()))
    (da, ga, ea), (db, gb, eb) = res
    assert eb < ea  # in place, the particles that left their bin keep taking the exact path; re-binned every step only the new ones do
    for k in da:
        a, b = da[k].reshape(n, -1).astype(np.float64), db[k].reshape(n, -1).astype(np.float64)
        assert np.isfinite(b).all(), k
        scale = np.sqrt(n * (a ** 2).sum(0)) + 1e-30
        assert (np.abs(a.sum(0) - b.sum(0)) <= 2e-5 * scale).all(), k
        assert (np.abs((a ** 2).sum(0) - (b ** 2).sum(0)) <= 1e-4 * (a ** 2).sum(0) + 1e-30).all(), k
    _compare_grids(ga, gb, 3e-4)


# ------------------------------------------------------------------------------------------------------------------------------
# Whole-function parity against the REFERENCE (tests/golden/p2g_g2p.npz: P2GTransfer / G2PTransfer spelled over the reference's own
# LocalArena, compute_stress_*, matrixMatrixMultiplication3d; tools/gen_golden.py + oracle/ref_shim.cpp).  The fixtures are in
# SequentialExecutionPolicy order; the GPU sums the same terms in another order, so the tolerances are those of an order-dependent
# float sum of ~64 like-signed terms (mass, momentum: 2e-6 of the channel maximum) and, for the force channels, the stress budget
# of the per-particle pin (5e-5 of the elastic force scale of the cloud; von Mises / NACC follow cuda/physics/ConstitutiveModel.hpp
# where it differs from the host header the fixture was made with, see DESIGN.md "Oracle").
def _golden_setup(pol, name, side, cache_stress, binned=True, lane_width=64):
    from util import golden_p2g_g2p
    from zpc_amd.mpm import MpmTransfer
    g = golden_p2g_g2p(name, side)
    kw = dict(g["kw"])
    mt = MpmTransfer(pol, g["pos"].shape[0], g["dx"], g["dt"], model=g["model"], side=side, volume=g["volume"], lane_width=lane_width,
                     cache_stress=cache_stress, **kw)
    mt.upload(g["mass"], g["pos"], g["vel"], g["C"], g["F"][:, :mt.nF], g["logJp"] if g["model"] in (1, 3) else None)
    keys = torch.from_numpy(np.ascontiguousarray(g["keys"])).cuda()
    mt.adopt_partition(keys.data_ptr(), g["keys"].shape[0])     # block i = fixture key i: grids compare index for index
    pol.syncCtx()
    if binned:
        mt.rebin()
    return g, mt


def _grid_err(mt, want, rhs_scale):
    got = mt.grid.cpu().numpy().reshape(want.shape)
    scale = np.abs(want).max(axis=(0, 2))
    scale[4:] = rhs_scale
    return np.abs(got - want).max(axis=(0, 2)) / scale


def _particles_in_input_order(mt, binned):
    d = mt.download()
    if not binned:
        return d
    inv = np.empty(mt.n, np.int64)
    inv[mt.order.cpu().numpy()] = np.arange(mt.n)   # stored row r holds input particle order[r]
    return {k: v[inv] for k, v in d.items()}


GOLDEN_GPU_CASES = [("fixedcorotated", 4), ("fixedcorotated", 8), ("sand", 4), ("sand", 8), ("vonmises", 8), ("nacc", 8), ("eos", 8)]
# force-channel budget per model (fraction of the cloud's elastic force scale).  von Mises / NACC: the fixture was made with the HOST
# header simulation/transfer/P2G.hpp includes (physics/ConstitutiveModel_Vol_dP.hpp); the GPU path follows the header the
# reference's CUDA build uses (cuda/physics/ConstitutiveModel.hpp), which computes something else where the material yields
# (NACC: p0 = bm (1e-5 + sinh(xi max(-logJp, 0))) instead of bm 1e-5 + sin(...); von Mises: sqrtf of a negative discriminant = NaN
# instead of a clamp) -- see DESIGN.md "Oracle".  For those two the force channels and logJp are pinned through the oracle
# (oracle hostVariant=1 == fixture on the CPU, GPU == oracle hostVariant=0 in test_p2g_g2p_vs_oracle); everything that does not go
# through the yield branch (mass, momentum, the whole G2P leg, F) is compared with the fixture here.
RHS_TOL = {"fixedcorotated": 5e-5, "sand": 5e-5, "eos": 5e-5, "vonmises": None, "nacc": None}


def _rhs_ok(err, name):
    return RHS_TOL[name] is None or bool((err[4:] <= RHS_TOL[name]).all())


@pytest.mark.parametrize("binned", [True, False])
@pytest.mark.parametrize("name,side", GOLDEN_GPU_CASES)
def test_p2g_g2p_match_reference_golden(pol, name, side, binned):
    """zs_rocm_mpm_p2g and zs_rocm_mpm_g2p (reference order: constitutive update inside P2G) vs the reference-made fixture."""
    g, mt = _golden_setup(pol, name, side, cache_stress=False, binned=binned)
    mt.clear_grid()
    mt.p2g()
    pol.syncCtx()
    err = _grid_err(mt, g["grid"], g["rhs_scale"])
    assert (err[:4] <= 2e-6).all() and _rhs_ok(err, name), err
    if name == "sand":
        lj = _particles_in_input_order(mt, binned)["logJp"]
        assert np.abs(lj - g["logJp1"]).max() <= 2e-5
    # G2P from the fixture's velocity grid
    mt.grid.copy_(torch.from_numpy(g["gridv"]).reshape(-1))
    mt.g2p()
    pol.syncCtx()
    d = _particles_in_input_order(mt, binned)
    assert np.abs(d["x"] - g["pos1"]).max() <= 1e-7
    assert np.abs(d["v"] - g["vel1"]).max() <= 2e-6 * np.abs(g["vel1"]).max()
    assert np.abs(d["C"] - g["C1"]).max() <= 1e-5 * np.abs(g["C1"]).max()
    if name == "eos":
        assert np.abs(d["J"][:, 0] - g["F1"][:, 0]).max() <= 1e-6
    else:
        assert np.abs(d["F"] - g["F1"]).max() <= 2e-6
    assert __import__("zpc_amd").lib().zs_rocm_last_error(-1) == 0


@pytest.mark.parametrize("name,side", GOLDEN_GPU_CASES)
def test_fused_g2p2g_matches_reference_golden(pol, name, side):
    """The bench's flagship kernel (zs_rocm_mpm_g2p2g: G2P of step n + P2G of step n+1, binned, cached stress; sand / side 8 is the
    headline instantiation) DIRECTLY against the reference-made fixture: particle state after G2P and the next step's grid."""
    g, mt = _golden_setup(pol, name, side, cache_stress=True)
    mt.grid.copy_(torch.from_numpy(g["gridv"]).reshape(-1))
    # the fused pass reads the logJp the previous P2G left behind (reference: P2G.hpp:101 stores it), F unprojected
    if name in ("sand", "nacc"):
        o = mt.order.cpu().numpy()
        lj1 = torch.from_numpy(g["logJp1"][o]).cuda()
        lib = __import__("zpc_amd").lib()
        tmp = torch.empty(mt.n, mt.nchn, device="cuda")
        lib.zs_rocm_tv_to_aos_f32(pol.handle, mt.buf.data_ptr(), mt.n, mt.nchn, mt.L, tmp.data_ptr())
        pol.syncCtx()
        tmp[:, mt.off["logJp"]] = lj1
        lib.zs_rocm_tv_from_aos_f32(pol.handle, tmp.data_ptr(), mt.n, mt.nchn, mt.L, mt.buf.data_ptr())
        pol.syncCtx()
    mt.g2p2g(write_all=True)
    pol.syncCtx()
    d = _particles_in_input_order(mt, True)
    assert np.abs(d["x"] - g["pos1"]).max() <= 1e-7
    assert np.abs(d["v"] - g["vel1"]).max() <= 2e-6 * np.abs(g["vel1"]).max()
    assert np.abs(d["C"] - g["C1"]).max() <= 1e-5 * np.abs(g["C1"]).max()
    if name == "eos":
        assert np.abs(d["J"][:, 0] - g["F1"][:, 0]).max() <= 1e-6
    else:
        assert np.abs(d["F"] - g["F1"]).max() <= 2e-6
    err = _grid_err(mt, g["grid2"], g["rhs_scale"])
    assert (err[:4] <= 5e-6).all() and _rhs_ok(err, name), err
    if name == "sand":
        assert np.abs(d["logJp"] - g["logJp2"]).max() <= 2e-5
    assert not mt.left_partition()
    assert __import__("zpc_amd").lib().zs_rocm_last_error(-1) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# Slotted particle storage (zpc_amd/csrc/mpm_slotted.hip): the fused step that keeps its own storage order while particles move.
def _id_order(m, x):
    """particles carry their identity in their mass (a few fixture masses coincide: the position breaks the tie)"""
    return np.lexsort((x[:, 2], x[:, 1], x[:, 0], m))


def _by_mass(d):
    o = _id_order(d["m"], d["x"])
    return {k: v[o] for k, v in d.items()}


@pytest.mark.parametrize("name,side", [("fixedcorotated", 4), ("fixedcorotated", 8), ("sand", 4), ("sand", 8), ("eos", 8)])
def test_slotted_fused_matches_reference_golden(pol, name, side):
    """zs_rocm_mpm_g2p2g_slotted (main kernel + mover pull) against the reference-made fixture: particle state after G2P and the next
    step's grid, as test_fused_g2p2g_matches_reference_golden; the fixture's particles move (|v| ~ 1, dt 1e-4, dx 1/128: a few change
    cell), so outboxes, pull and re-homing are on the path."""
    g, mt = _golden_setup(pol, name, side, cache_stress=True, binned=False)
    if name == "sand":   # the fused pass reads the logJp the previous P2G left behind
        tmp = torch.empty(mt.n, mt.nchn, device="cuda")
        lib = __import__("zpc_amd").lib()
        lib.zs_rocm_tv_to_aos_f32(pol.handle, mt.buf.data_ptr(), mt.n, mt.nchn, mt.L, tmp.data_ptr())
        pol.syncCtx()
        tmp[:, mt.off["logJp"]] = torch.from_numpy(g["logJp1"]).cuda()
        lib.zs_rocm_tv_from_aos_f32(pol.handle, tmp.data_ptr(), mt.n, mt.nchn, mt.L, mt.buf.data_ptr())
        pol.syncCtx()
    mt.slot(K=16)
    assert int(mt.cell_mask.cpu().numpy().view(np.uint32).astype(np.uint64).sum()) > 0
    mt.grid.copy_(torch.from_numpy(g["gridv"]).reshape(-1))
    mt.g2p2g(write_all=True)
    pol.syncCtx()
    st = mt.check_slots()
    d = _by_mass(mt.download())
    o = _id_order(g["mass"], g["pos1"])
    assert np.array_equal(d["m"], g["mass"][o])                       # every particle is still there, exactly once
    assert np.abs(d["x"] - g["pos1"][o]).max() <= 1e-7
    assert np.abs(d["v"] - g["vel1"][o]).max() <= 2e-6 * np.abs(g["vel1"]).max()
    assert np.abs(d["C"] - g["C1"][o]).max() <= 1e-5 * np.abs(g["C1"]).max()
    if name == "eos":
        assert np.abs(d["J"][:, 0] - g["F1"][o, 0]).max() <= 1e-6
    else:
        assert np.abs(d["F"] - g["F1"][o]).max() <= 2e-6
    err = _grid_err(mt, g["grid2"], g["rhs_scale"])
    assert (err[:4] <= 5e-6).all() and _rhs_ok(err, name), err
    if name == "sand":
        assert np.abs(d["logJp"] - g["logJp2"][o]).max() <= 2e-5
    # the storage invariant: every particle sits under the cell of its base node
    assert st[5] == st[6]


@pytest.mark.parametrize("side,model", [(8, 1), (4, 1), (8, 0)])
def test_slotted_steps_of_a_moving_cloud_vs_oracle(pol, oracle, side, model):
    """six fused steps of a cloud drifting ~0.3 cell per step (most particles change cell, many change bin / block): the slotted
    step (no re-bin anywhere) against the oracle's g2p -> p2g sequence, particle for particle and node for node."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-3
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=77 + side, vel_scale=0.3)
    n = pos.shape[0]
    mass = (mass * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)   # identity tag
    assert len(np.unique(mass)) == n
    vel += np.array([4.0, -5.0, 3.0], np.float32)                      # 0.25-0.32 cell per step
    vol = dx ** 3 / 8
    lj = (0.01 * rng(5).standard_normal(n)).astype(np.float32)
    om = OracleMpm(oracle, model, dx, dt, side, vol)
    mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, lj if model == 1 else None)
    mt.build_partition(n, margin=1)
    keys = mt.active_keys()
    om.adopt_partition(keys)
    # step 0: P2G on both sides (the GPU primes its grid through the binned path), then grid update
    ljo = lj.copy()
    om.p2g(mass, pos, vel, Cm, F, ljo)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    om.grid_update((0.0, -9.8, 0.0))
    mt.grid_update((0.0, -9.8, 0.0))
    mt.slot(K=24, outbox_cap=512)
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    # the binned priming pass re-ordered the particles and evaluated the model once (logJp): continue from that state
    for step in range(6):
        om.g2p(po, vo, Co, Fo)
        om.grid[:] = 0
        om.p2g(mass, po, vo, Co, Fo, ljo)
        mt.g2p2g(write_all=(step == 5))
        pol.syncCtx()
        mt.check_slots()
        ga = mt.grid.cpu().numpy().reshape(om.grid.shape)
        scale = np.abs(om.grid).max(axis=(0, 2)) + 1e-30
        assert (np.abs(ga - om.grid).max(axis=(0, 2)) <= 3e-4 * scale).all(), (step, np.abs(ga - om.grid).max(axis=(0, 2)) / scale)
        om.grid_update((0.0, -9.8, 0.0))
        mt.grid_update((0.0, -9.8, 0.0))
    d = _by_mass(mt.download())
    o = _id_order(mass, po)
    assert np.array_equal(d["m"], mass[o])
    assert np.abs(d["x"] - po[o]).max() <= 2e-6
    assert np.abs(d["v"] - vo[o]).max() <= 2e-4 * np.abs(vo).max()
    assert np.abs(d["F"] - Fo[o]).max() <= 5e-5
    # most particles changed cell at least once
    c0 = np.floor(pos / dx - 0.5).astype(int)
    c1 = np.floor(po / dx - 0.5).astype(int)
    assert (np.abs(c1 - c0).max(axis=1) >= 1).mean() > 0.8


@pytest.mark.parametrize("side", [8, 4])
def test_slotted_uneven_cells_many_sparse_rounds_vs_oracle(pol, oracle, side):
    """A cloud whose density varies by a factor of ~20 from cell to cell (up to 22 particles in a cell next to cells with one): the
    bins have many sparse rounds, which the packed producers walk several to a group and the consumers still take one by one
    (entry table, staged-entry ring, rounds completing in the middle of a chunk).  Four slotted steps with motion against the oracle."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-3
    # a 10^3-cell box; per cell a particle count drawn from a heavy-tailed distribution
    # (a cell needs free rounds for a step's arrivals on top of the particles it holds: K = 32 rounds, up to 22 particles at the start)
    mass, pos, vel, Cm, F, cnt = make_uneven_cloud(2024 + side)   # ~0.2-0.25 cell per step
    n = pos.shape[0]
    assert cnt.max() >= 20 and (cnt == 1).sum() > 50
    lj = np.zeros(n, np.float32)
    vol = dx ** 3 / 8
    om = OracleMpm(oracle, 1, dx, dt, side, vol)
    mt = MpmTransfer(pol, n, dx, dt, model=1, side=side, volume=vol, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, lj)
    mt.build_partition(n, margin=1)
    om.adopt_partition(mt.active_keys())
    ljo = lj.copy()
    om.p2g(mass, pos, vel, Cm, F, ljo)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    om.grid_update((0.0, -9.8, 0.0))
    mt.grid_update((0.0, -9.8, 0.0))
    mt.slot(K=32, outbox_cap=512)
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    for step in range(4):
        om.g2p(po, vo, Co, Fo)
        om.grid[:] = 0
        om.p2g(mass, po, vo, Co, Fo, ljo)
        mt.g2p2g(write_all=(step == 3))
        pol.syncCtx()
        mt.check_slots()
        ga = mt.grid.cpu().numpy().reshape(om.grid.shape)
        scale = np.abs(om.grid).max(axis=(0, 2)) + 1e-30
        assert (np.abs(ga - om.grid).max(axis=(0, 2)) <= 3e-4 * scale).all(), (step, np.abs(ga - om.grid).max(axis=(0, 2)) / scale)
        om.grid_update((0.0, -9.8, 0.0))
        mt.grid_update((0.0, -9.8, 0.0))
    d = _by_mass(mt.download())
    o = _id_order(mass, po)
    assert np.array_equal(d["m"], mass[o])
    assert np.abs(d["x"] - po[o]).max() <= 2e-6
    assert np.abs(d["v"] - vo[o]).max() <= 2e-4 * np.abs(vo).max()
    assert np.abs(d["F"] - Fo[o]).max() <= 5e-5


def _slot_census(mt):
    """(tags, cells): mass tag and the world cell of every occupied slot of the slotted storage, from the occupancy words and the block keys"""
    side, K = mt.side, mt.K
    bpb = (side // 4) ** 3
    masks = mt.cell_mask.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    keys = mt.active_keys() * (1 if mt.key_is_origin else side)      # block origin in cells
    buf = mt.buf.view(mt.nbins * K, mt.nchn, 64).cpu().numpy()
    tags, cells, where = [], [], []
    for c in np.nonzero(masks)[0]:
        b, lane = divmod(int(c), 64)
        blk, sub = divmod(b, bpb)
        o = np.array([((sub >> 2) & 1) * 4, ((sub >> 1) & 1) * 4, (sub & 1) * 4]) if side == 8 else np.zeros(3, int)
        cell = keys[blk] + o + np.array([lane >> 4, (lane >> 2) & 3, lane & 3])
        for r in range(K):
            if (masks[c] >> r) & 1:
                row = buf[b * K + r]
                tags.append(row[0, lane])
                cells.append(cell)
                where.append((b, r, lane, row[1:4, lane].copy()))
    return np.array(tags, np.float32), np.array(cells), where


@pytest.mark.parametrize("side", [8, 4])
def test_slotted_downward_rehome_with_simultaneous_arrivals(pol, oracle, side):
    """The stayer that holds the top round of a cell re-homes into a lower free round IN THE SAME STEP in which other particles arrive in
    that cell from a neighbour cell of the bin (both draw tickets of the cell's counter: mpm_slot.hpp, `lowered`).  Construction: a
    uniform drift of 0.3 cell per step; cell A = cell (1,1,1) of a bin holds leavers (near its +x face) in its low rounds and stayers
    above them; the cell before it holds particles that cross into A one step later.  After step 1 cell A has holes below its top round,
    in step 2 the top stayer is lowered while four particles arrive.  Checked: every particle is stored exactly once under the cell of
    its base node, the occupancy words say so, nobody is lost, and the particle state follows the oracle."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-3
    v0 = np.array([0.3 * dx / dt, 0.0, 0.0], np.float32)
    org = np.array([16, 16, 16]) * 1.0                               # a block corner (cells); base node of x is floor(x/dx - 0.5)
    g = rng(4321 + side)

    def in_cell(cx, lx, k):                                          # k particles with base node (cx, 1, 1) + org, local x in lx
        p = np.empty((k, 3))
        p[:, 0] = org[0] + cx + 0.5 + g.uniform(lx[0], lx[1], k)
        p[:, 1:] = org[1:] + 1 + 0.5 + g.uniform(0.2, 0.8, (k, 2))
        return p
    # cell A = (1,1,1): leaver, stayer, leaver, stayer, leaver, stayer (slot_particles hands out rounds in this order)
    a = np.empty((6, 3))
    a[0::2] = in_cell(1, (0.80, 0.95), 3)                           # cross into (2,1,1) in step 1
    a[1::2] = in_cell(1, (0.05, 0.30), 3)                           # still in A after two steps
    b = in_cell(0, (0.45, 0.65), 4)                                  # cell (0,1,1): in A after step 2, not after step 1
    filler = np.concatenate([in_cell(cx, (0.1, 0.9), 3) for cx in (2, 3, 4, 5)])   # company, so that the grid around A carries mass
    pos = (np.concatenate([a, b, filler]) * dx).astype(np.float32)
    n = pos.shape[0]
    mass = (1000.0 * dx ** 3 / 8 * (1 + 1e-2 * np.arange(1, n + 1) / n)).astype(np.float32)
    vel = np.tile(v0, (n, 1)).astype(np.float32)
    Cm = np.zeros((n, 9), np.float32)
    F = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))
    vol = dx ** 3 / 8
    om = OracleMpm(oracle, 0, dx, dt, side, vol)
    mt = MpmTransfer(pol, n, dx, dt, model=0, side=side, volume=vol, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F)
    mt.build_partition(64, margin=1)
    om.adopt_partition(mt.active_keys())
    om.p2g(mass, pos, vel, Cm, F)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    om.grid_update((0.0, 0.0, 0.0))
    mt.grid_update((0.0, 0.0, 0.0))
    mt.slot(K=24, outbox_cap=64)
    cellA = (org + np.array([1, 1, 1])).astype(int)
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    seen_lowering = False
    for step in range(3):
        tags0, cells0, where0 = _slot_census(mt)
        inA0 = {float(t): w[1] for t, c, w in zip(tags0, cells0, where0) if (c == cellA).all()}   # tag -> round, before the step
        om.g2p(po, vo, Co, Fo)
        om.grid[:] = 0
        om.p2g(mass, po, vo, Co, Fo)
        mt.g2p2g(write_all=(step == 2))
        pol.syncCtx()
        st = mt.check_slots()
        tags, cells, where = _slot_census(mt)
        # every particle once, under the cell of its base node
        assert tags.shape[0] == n and len(set(tags.tolist())) == n and set(tags.tolist()) == set(mass.tolist())
        base = np.floor(np.array([w[3] for w in where]) / dx - 0.5).astype(int)
        assert np.array_equal(base, cells)
        o = {float(t): i for i, t in enumerate(mass)}
        want = np.floor(po[[o[float(t)] for t in tags]] / dx - 0.5).astype(int)
        assert np.array_equal(cells, want)
        inA = {float(t): w[1] for t, c, w in zip(tags, cells, where) if (c == cellA).all()}
        if step == 0:
            # the three leavers are gone, the stayers sit above the holes they left
            assert len(inA) == 3 and max(inA.values()) > 2, inA
        if step == 1:
            arrivals = [t for t in inA if t not in inA0]
            stayers = {t: (inA0[t], inA[t]) for t in inA if t in inA0}
            assert len(arrivals) == 4 and len(stayers) == 3, (inA0, inA)
            top = max(stayers, key=lambda t: stayers[t][0])
            seen_lowering = stayers[top][1] != stayers[top][0]                      # the top stayer changed its round in this step ...
            assert all(stayers[t][0] == stayers[t][1] for t in stayers if t != top)  # ... the others kept theirs
            assert len(set(inA.values())) == 7                                       # seven particles, seven different rounds
        ga = mt.grid.cpu().numpy().reshape(om.grid.shape)
        scale = np.abs(om.grid).max(axis=(0, 2)) + 1e-30
        scale = np.maximum(scale, 1e-2 * scale[1])   # (F = I: the force channels (an impulse, like the momentum) are rounding noise of a zero stress)
        assert (np.abs(ga - om.grid).max(axis=(0, 2)) <= 3e-4 * scale).all(), (step, np.abs(ga - om.grid).max(axis=(0, 2)) / scale)
        om.grid_update((0.0, 0.0, 0.0))
        mt.grid_update((0.0, 0.0, 0.0))
    assert seen_lowering
    d = _by_mass(mt.download())
    oi = _id_order(mass, po)
    assert np.array_equal(d["m"], mass[oi])
    assert np.abs(d["x"] - po[oi]).max() <= 2e-6
    assert np.abs(d["v"] - vo[oi]).max() <= 2e-4 * np.abs(vo).max()


@pytest.mark.parametrize("storage", ["unfused", "compact", "slotted"])
def test_local_position_that_rounds_up_to_one_and_a_half_follows_the_reference(pol, oracle, storage):
    """The reference takes a quadratic arena's weights from localPos - base_node(localPos) although localPos is already relative to the base
    node (math/curve/InterpolationKernel.hpp:108 on simulation/Utils.hpp:59-60).  Next to the coordinate origin X - floor(X - 0.5) can ROUND
    up to exactly 1.5 (or X - 0.5 round up to an integer and leave it just below 0.5); the second base_node is then +-1 and the particle is
    weighted as if one cell away on the unchanged corner: half of its mass lands one node off.  (That is what left 76 particles with |C| ~ 2000 / s at the foot of the 64 Mi column in 3 % of the runs,
    profiles/r03_compact_outliers.md.)  The oracle restates it; every scatter path of the library has to do the same.  dx = 2^-6 and a grid
    at rest make the positions exact: particles sit at X = 0.5 - 2^-25, 0.5 - 2^-24 and -0.5 - 2^-24 on one axis each."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt, side, model = 1.0 / 64, 1e-3, 8, 0
    mass, pos, vel, Cm, F = make_cloud(6, dx, 2, origin=(-3 * dx, -3 * dx, -3 * dx), seed=311, vel_scale=0.0)
    n = pos.shape[0]
    vel[:] = 0
    Cm[:] = 0
    edges = [np.float32(0.5) - np.float32(2.0 ** -25), np.float32(0.5) - np.float32(2.0 ** -24), np.float32(-0.5) - np.float32(2.0 ** -24)]
    g = rng(312)
    picked = g.choice(n, 36, replace=False)
    for j, i in enumerate(picked):
        pos[i, j % 3] = edges[(j // 3) % 3] * np.float32(dx)
    X = pos * np.float32(64.0)
    lpn = X - np.floor(X - np.float32(0.5))
    assert lpn.dtype == np.float32 and int(((lpn[picked] >= np.float32(1.5)) | (lpn[picked] < np.float32(0.5))).any(axis=1).sum()) == 36
    mass = (mass * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    vol = dx ** 3 / 8
    om = OracleMpm(oracle, model, dx, dt, side, vol)
    mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, None)
    mt.build_partition(n, margin=1)
    om.adopt_partition(mt.active_keys())
    om.p2g(mass, pos, vel, Cm, F, None)
    want = om.grid.copy()
    # the folded deposit really differs from the plain one: the same cloud with those coordinates one ulp further out
    pos2 = pos.copy()
    for j, i in enumerate(picked):
        pos2[i, j % 3] = np.nextafter(pos2[i, j % 3], np.float32(-1.0))
    om.grid[:] = 0
    om.p2g(mass, pos2, vel, Cm, F, None)
    assert np.abs(om.grid[:, 0] - want[:, 0]).max() > 0.2 * mass.max()
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    pol.syncCtx()
    scale = np.abs(want).max(axis=(0, 2)) + 1e-30

    def check(tag):
        got = mt.grid.cpu().numpy().reshape(want.shape)
        err = np.abs(got - want).max(axis=(0, 2)) / scale
        assert (err[[0, 4, 5, 6]] <= 3e-4).all() and np.abs(got[:, 1:4]).max() == 0, (tag, err)
    check("p2g")
    if storage == "unfused":
        return
    mt.grid_update((0.0, 0.0, 0.0))   # a grid at rest: the fused step leaves every particle where it is, F unchanged
    if storage == "slotted":
        mt.slot(K=24, outbox_cap=256)
    for step in range(2):
        mt.g2p2g(write_all=(step == 1))
        pol.syncCtx()
        if storage == "slotted":
            mt.check_slots()
        check("fused step %d" % step)
        mt.grid_update((0.0, 0.0, 0.0))
    d = _by_mass(mt.download())
    o = _id_order(mass, pos)
    assert np.array_equal(d["x"], pos[o]) and np.abs(d["v"]).max() == 0


def test_slotted_capacity_overflow_is_reported_and_loses_no_particle(pol, oracle):
    """A tiny outbox (and few spare rounds per cell): the step reports it through the status words, and a mover that found no new home
    stays in its old slot with its new state -- after the failing step the storage still holds every particle (same set of masses),
    so the caller can re-slot with a larger K / outboxCap instead of having lost mass."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt, side = 1.0 / 64, 1e-3, 8
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=401, vel_scale=0.3)
    n = pos.shape[0]
    mass = (mass * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    vel += np.array([4.0, -5.0, 3.0], np.float32)
    vol = dx ** 3 / 8
    lj = np.zeros(n, np.float32)
    mt = MpmTransfer(pol, n, dx, dt, model=1, side=side, volume=vol, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, lj)
    mt.build_partition(n, margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    mt.slot(K=32, outbox_cap=2)     # at 0.3 cell per step a bin sends dozens of movers to its neighbours: two records fit
    reported = False
    for step in range(3):
        mt.g2p2g(write_all=True)
        pol.syncCtx()
        try:
            mt.check_slots()
        except RuntimeError as e:
            reported = True
            assert "full" in str(e) or "not stored under its cell" in str(e), str(e)
        mt.grid_update((0.0, -9.8, 0.0))
    assert reported
    d = mt.download()
    assert d["m"].shape[0] == n and np.array_equal(np.sort(d["m"]), np.sort(mass))


# ------------------------------------------------------------------------------------------------ r04: the slotted step never drops a particle
def _primed_slotted(pol, n, dx, dt, model, side, mass, pos, vel, Cm, F, lj, margin, K, outbox_cap):
    from zpc_amd.mpm import MpmTransfer
    vol = dx ** 3 / 8
    mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True)
    mt.upload(mass, pos, vel, Cm, F, lj if model == 1 else None)
    mt.build_partition(n, margin=margin)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    mt.slot(K=K, outbox_cap=outbox_cap)
    return mt


def _repartition(mt, pol, margin, K, outbox_cap, strict=True):
    """what bench.py::remap does on one rank: the step before stored v, C and the stress of every particle"""
    mt.unslot(strict=strict)
    mt.build_partition(max(mt.n, 64), margin=margin)
    mt.rebin()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    mt.slot(K=K, outbox_cap=outbox_cap)


@pytest.mark.parametrize("side", [8, 4])
def test_slotted_mover_without_a_destination_block_keeps_its_slot(pol, side):
    """A partition without margin and a cloud that runs out of it (0.3 cell per step towards -x, -y: the blocks there are not in the
    table): r03 dropped such movers (the 3000-step soak lost 0.34 % of the column this way).  Now a mover whose destination block is
    missing keeps its old slot with its new state: after every step the storage holds every particle (same multiset of identity
    masses), `sent == re-homed`, status word [2] reports it, the early warning [3] came first, and a re-partition + re-slot recovers
    (the following steps run clean).  Reference semantics: every particle is written back, simulation/transfer/G2P.hpp:67-82."""
    dx, dt = 1.0 / 64, 1e-3
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=431 + side, vel_scale=0.2)
    n = pos.shape[0]
    mass = (mass * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    vel += np.array([-5.0, -4.0, 0.5], np.float32)
    lj = np.zeros(n, np.float32)
    mt = _primed_slotted(pol, n, dx, dt, 1, side, mass, pos, vel, Cm, F, lj, margin=0, K=24, outbox_cap=512)
    warned_at = flagged_at = None
    for step in range(side * 5):
        mt.g2p2g(write_all=True)
        mt.grid_update((0.0, -9.8, 0.0))
        pol.syncCtx()
        w = mt.slot_status[:5].cpu().numpy()
        if w[3] and warned_at is None:
            warned_at = step
        if w[2] and flagged_at is None:
            flagged_at = step
        cnt = int(__import__("zpc_amd").lib().zs_rocm_mpm_slot_list(pol.handle, mt.cell_mask.data_ptr(), mt.nbins, mt.K, None))
        assert cnt == n, (step, cnt, n)
        if flagged_at is not None and step >= flagged_at + 2:
            break
    assert flagged_at is not None, "the cloud never left the partition: the test does not test"
    assert warned_at is not None and warned_at < flagged_at, (warned_at, flagged_at)   # the early warning comes first
    with pytest.raises(RuntimeError, match="outside the partition"):
        mt.check_slots(strict=True)                                      # strict callers are stopped; the record keeps what happened
    rec = mt.slot_record
    assert rec["sent"] == rec["homed"] and rec["sent"] > 0               # every mover that was sent was re-homed
    assert rec["flags"][2] == 1 and rec["log"], rec
    # nobody lost, nobody duplicated; and a re-partition + re-slot takes everybody back into a valid storage
    _repartition(mt, pol, 1, 24, 512, strict=False)
    d = mt.download()
    assert np.array_equal(np.sort(d["m"]), np.sort(mass))
    for step in range(3):
        mt.g2p2g(write_all=True)
        mt.grid_update((0.0, -9.8, 0.0))
        pol.syncCtx()
        mt.check_slots(strict=True)
    assert np.array_equal(np.sort(mt.download()["m"]), np.sort(mass))


def test_slotted_full_destination_cell_in_another_bin_returns_the_mover(pol):
    """One spare round per cell over the fullest cell of the start and a drift of 0.3 cell per step: cells overflow within a few steps,
    inside a bin and across bins.  A record whose destination cell (another bin) has no free round goes BACK into the slot it left (slot_rehome_kernel, r04;
    r03 dropped it); the in-bin case keeps its slot.  Reported in status word [1]; the storage holds every identity after every step."""
    dx, dt, side = 1.0 / 64, 1e-3, 8
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=977, vel_scale=0.6)
    n = pos.shape[0]
    mass = (mass * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    vel += np.array([4.0, -5.0, 3.0], np.float32)
    lj = np.zeros(n, np.float32)
    base = np.floor(pos / np.float32(dx) - np.float32(0.5)).astype(np.int64)
    K = int(np.unique(base, axis=0, return_counts=True)[1].max()) + 1
    mt = _primed_slotted(pol, n, dx, dt, 1, side, mass, pos, vel, Cm, F, lj, margin=2, K=K, outbox_cap=512)
    full = False
    for step in range(8):
        mt.g2p2g(write_all=True)
        mt.grid_update((0.0, -9.8, 0.0))
        pol.syncCtx()
        st = mt.check_slots(strict=False)
        full = full or bool(st[1])
        assert st[5] == st[6], st
        d = mt.download()
        assert np.array_equal(np.sort(d["m"]), np.sort(mass)), step
    assert full, "no cell overflowed: the test does not test"


@pytest.mark.parametrize("inplace", [False, True])
def test_slotted_closed_loop_repartition_vs_oracle(pol, oracle, inplace):
    """(inplace: the partition follows the particles through zs_rocm_mpm_slot_compute_sparsity + zs_rocm_mpm_reslot -- bins move as whole
    tile rows, the velocity grid is carried over, no particle is read -- instead of unslot / partition / re-bin / prime / slot.)
    70 slotted steps of a cloud moving 0.3 cell per step (21 cells of travel through a partition with one block of margin), re-partitioned
    whenever the step's own status word [3] asks for it (poll_repartition: asynchronous copy, one polling interval of lag) -- the
    bench's closed loop.  The oracle's g2p -> p2g sequence runs beside it on the same partitions; after the last step every particle
    agrees, no flag other than the early warning was ever raised, and at least two re-partitions happened."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt, side, model = 1.0 / 64, 1e-3, 8, 0
    mass, pos, vel, Cm, F = make_cloud(8, dx, 2, seed=1311, vel_scale=0.2)
    n = pos.shape[0]
    mass = (mass * (1 + 1e-3 * np.arange(n) / n)).astype(np.float32)
    vel += np.array([4.0, -5.0, 3.0], np.float32)
    vol = dx ** 3 / 8
    mt = _primed_slotted(pol, n, dx, dt, model, side, mass, pos, vel, Cm, F, None, margin=1, K=24, outbox_cap=512)
    om = OracleMpm(oracle, model, dx, dt, side, vol)
    om.adopt_partition(mt.active_keys())
    om.p2g(mass, pos, vel, Cm, F, None)
    om.grid_update((0.0, -9.8, 0.0))
    po, vo, Co, Fo = pos.copy(), vel.copy(), Cm.copy(), F.copy()
    reparts, pending = [], False
    for step in range(70):
        om.g2p(po, vo, Co, Fo)
        om.grid[:] = 0
        om.p2g(mass, po, vo, Co, Fo, None)
        om.grid_update((0.0, -9.8, 0.0))
        mt.g2p2g(write_all=(pending and not inplace) or step == 69)
        mt.grid_update((0.0, -9.8, 0.0))
        if pending:
            if inplace:
                mt.repartition_slotted(margin=1, strict=True)
            else:
                _repartition(mt, pol, 1, 24, 512, strict=True)
            # the oracle moves to the same partition: its grid is a function of the particles it holds
            om.adopt_partition(mt.active_keys())
            om.grid[:] = 0
            om.p2g(mass, po, vo, Co, Fo, None)
            om.grid_update((0.0, -9.8, 0.0))
            reparts.append(step)
            pending = False
        elif step % 2 == 1:
            pending = mt.poll_repartition()
    pol.syncCtx()
    mt.check_slots(strict=True)
    assert len(reparts) >= 2, reparts
    rec = mt.slot_record
    assert rec["sent"] == rec["homed"] and rec["flags"][0] == rec["flags"][1] == rec["flags"][2] == rec["flags"][4] == 0, rec
    d = _by_mass(mt.download())
    o = _id_order(mass, po)
    assert np.array_equal(d["m"], mass[o])
    assert np.abs(d["x"] - po[o]).max() <= 2e-5
    assert np.abs(d["v"] - vo[o]).max() <= 1e-3 * np.abs(vo).max()
    assert np.abs(d["F"] - Fo[o]).max() <= 5e-4


@pytest.mark.parametrize("side", [4, 8])
def test_block_numbering_orders_of_the_partition(pol, oracle, side):
    """build_partition(order=...): every order numbers the same set of blocks; holders_lex (the default) puts the blocks that hold particles
    first in lexicographic key order with the apron blocks behind them; lex sorts every block; the P2G grid is the same by key
    (zs::bht leaves the numbering to the race of the inserting threads, Bht.hpp insert: any numbering is a valid one)."""
    from zpc_amd.mpm import MpmTransfer
    dx, dt = 1.0 / 64, 1e-4
    mass, pos, vel, Cm, F = make_cloud(11, dx, 2, seed=77 + side)
    n = pos.shape[0]
    # the block of each particle's stencil base (ComputeSparsity, SparsityOp.hpp:75-84: offset -2, displacement 0.5), in float32 like the kernel
    base = np.floor(pos.astype(np.float32) * np.float32(1.0 / dx) + np.float32(0.5)).astype(np.int64) - 2
    holders = {tuple(int(c) for c in k) for k in base // side}
    grids, keysets = {}, {}
    for order in ("insertion", None, "holders_lex", "lex", "morton"):
        mt = MpmTransfer(pol, n, dx, dt, model=0, side=side, volume=dx ** 3 / 8, lane_width=64)
        mt.upload(mass, pos, vel, Cm, F)
        nb = mt.build_partition(n, order=order)
        keys = [tuple(int(c) for c in k) for k in mt.active_keys()]
        assert len(set(keys)) == nb
        keysets[order] = set(keys)
        if order in (None, "holders_lex"):
            assert mt.block_order == "holders_lex"
            h = len(holders)
            assert set(keys[:h]) == holders and keys[:h] == sorted(keys[:h])
            assert keys[h:] == sorted(keys[h:])   # ... and the apron blocks behind them in key order too: nothing is left to the race
        if order == "lex":
            assert keys == sorted(keys)
        mt.rebin()
        mt.clear_grid()
        mt.p2g()
        pol.syncCtx()
        grids[order] = mt.grid_by_key()
    assert all(ks == keysets["insertion"] for ks in keysets.values())
    for order in (None, "holders_lex", "lex", "morton"):
        _compare_grids(grids[order], grids["insertion"], 1e-5)
    with pytest.raises(ValueError):
        mt.build_partition(n, order="hilbert")
    # the significance of the key's components: (0, 2, 1) = x, then z, y fastest
    nb = mt.build_partition(n, order="lex", axes=(0, 2, 1))
    keys = [tuple(int(c) for c in k) for k in mt.active_keys()]
    assert set(keys) == keysets["insertion"] and keys == sorted(keys, key=lambda k: (k[0], k[2], k[1]))
    mt.build_partition(n, axes=(2, 0, 1))
    keys = [tuple(int(c) for c in k) for k in mt.active_keys()]
    h = len(holders)
    assert set(keys[:h]) == holders and keys[:h] == sorted(keys[:h], key=lambda k: (k[2], k[0], k[1])) and mt.block_axes == (2, 0, 1)
    assert keys[h:] == sorted(keys[h:], key=lambda k: (k[2], k[0], k[1]))
    with pytest.raises(ValueError):
        mt.build_partition(n, axes=(0, 0, 1))
