"""The SVD and constitutive kernels against the float64 reference of tests/ref64_stress.py: the same families, seeds and checker as
tests/test_stress_ref64_cpu.py.  The kernels are held to the ceilings measured there from the CPU oracle (never from the kernels), and
sample by sample to the oracle within the tolerance of test_svd_and_stress_blocks, 1e-4 of the scale, now on every family and for
P F^T vol, the projected F and logJp alike.  Only sand's P F^T vol on the wide and the rank-deficient families may be further from the
oracle (ref64_stress.ORACLE_OWN_ERROR: the oracle forms it through V and is off by 3.5e-3 there; the kernel's U diag(tau) U^T by
1.9e-5 on rank 2 and 4.5e-7 on rank 1, and by 3.0 ... 3.7e-3 on `wide`, where both carry the truncation error of log s2 and differ by up
to 2.3e-3 on 16 % of the samples), and then no further from float64 than the oracle is, plus 1e-4.  For the projected F the 1e-4 is multiplied by the condition
number of the polar rotation, max(1, 2 ||F|| / (s1 + s2)) from the float64 singular values (ref64_stress.evaluate): at plain 1e-4 von
Mises and NACC on the wide family miss it by up to 4.3e-4 and 1.8e-4 on about 1 % and 0.1 % of the samples, all at s1 + s2 = 0.01 ...
0.02 ||F||, where U V^T multiplies the rounding difference between device and host (rsq against 1 / sqrtf, contraction) by 1e2.  The
last three figures of each line count the samples over the plain 1e-4, the one before them is the worst |F - F oracle| / tolerance.

    zs_rocm_svd3                 S, reconstruction, ordering, orthonormality, determinants
    zs_rocm_mpm_stress           model_stress<MODEL, WRITE_F = true>: P F^T vol, projected F, logJp, finite pattern; the fluid from J
    zs_rocm_mpm_update_stress    model_stress<MODEL, false>, the production instantiation, through an MpmTransfer with cache_stress at
                                 both lane widths: the six packed components and logJp against the reference, and against stress_pack of
                                 the test entry's nine (PROD_GAP)

Prints `REF64 stress gpu ...` lines in the format of the CPU module."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref64_stress as rs
from util import oracle_stress_all, eos_f32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-4     # |kernel - oracle| per sample, of the scale: the tolerance of test_svd_and_stress_blocks, unchanged
# |update_stress - stress_pack(zs_rocm_mpm_stress)| of the scale, worst over the families, per model: measured on the MI355X
# (2026-10-18), asserted at 4 x.  Sand and fixed-corotated share every operation that reaches the stress between the two
# instantiations; von Mises, NACC and the fluid are the same code in both.  A measured 0 is asserted as equality.
PROD_GAP = {0: 0.0, 1: 0.0, 2: 2.72e-10, 3: 0.0, 4: 0.0}
PROD_GAP_LOGJP = {1: 0.0, 3: 1.19e-7}     # logJp, absolute: sand equal; NACC 1 ulp at |logJp| ~ 1 on two families (benign, nearly_repeated)
# Sand's U diag(tau) U^T: component (r, c) sums (U[r][i] tau[i]) U[c][i] over i and (c, r) sums (U[c][i] tau[i]) U[r][i].  Each term
# differs between the two by at most 2 u |tau_i| (two roundings, |U| <= 1), three terms and two additions: 8 u max|tau|, and
# max|tau| = ||PF||_2 <= 3 |PF|max <= 3 scale.
SAND_ASYM = 24 * rs.U32


def _fmt(x):
    return "nan" if np.isnan(x) else "%.2e" % x


@pytest.fixture(scope="module")
def fams():
    return {seed: rs.families(seed) for seed in rs.SEEDS}


def _params(pset, volume=rs.VOLUME):
    from zpc_amd import MpmParams, lib
    k = rs.PSETS[pset] if isinstance(pset, str) else pset
    return MpmParams(k["model"], 1 / 64, 1e-4, volume, k["E"], k["nu"], k["cohesion"], k["beta"], k["yield_surface"], int(k["vol_correction"]),
                     4, 0, k["yield_stress"], k["xi"], lib().zs_rocm_nacc_msqr(k["friction_angle"]), int(k["hardening"]), k["bulk"], k["viscosity"])


def _gpu_stress(pol, pset, F, lj):
    """zs_rocm_mpm_stress on copies -> PF [n, 9], F [n, 9], logJp [n]"""
    from zpc_amd import lib
    n = len(F)
    p = _params(pset)
    Fd, ljd = torch.from_numpy(np.ascontiguousarray(F)).cuda(), torch.from_numpy(np.ascontiguousarray(lj)).cuda()
    PF = torch.empty(n, 9, device="cuda")
    lib().zs_rocm_mpm_stress(pol.handle, C.byref(p), Fd.data_ptr(), ljd.data_ptr(), n, PF.data_ptr())
    pol.syncCtx()
    return PF.cpu().numpy(), Fd.cpu().numpy(), ljd.cpu().numpy()


def _collect(failures, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except AssertionError as err:
        failures.append(str(err).splitlines()[0])
        return None


@pytest.mark.parametrize("seed", rs.SEEDS)
def test_svd3_vs_ref64(pol, fams, seed):
    from zpc_amd import lib
    failures = []
    for family in rs.FAMILIES:
        F = fams[seed][family][0]
        n = len(F)
        dF = torch.from_numpy(F).cuda()
        U, S, V = torch.empty(n, 9, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, 9, device="cuda")
        lib().zs_rocm_svd3(pol.handle, dF.data_ptr(), n, U.data_ptr(), S.data_ptr(), V.data_ptr())
        pol.syncCtx()
        Uh, Sh, Vh = U.cpu().numpy(), S.cpu().numpy(), V.cpu().numpy()
        e = rs.svd_errors(F, Uh, Sh, Vh)
        print("REF64 stress gpu %s svd S %s recon %s order %s ortho %s" % (family, _fmt(e["S"].max()), _fmt(e["recon"].max()),
                                                                            _fmt(max(e["order"].max(), 0)), _fmt(e["ortho"].max())))
        _collect(failures, rs.check_svd, family, F, Uh, Sh, Vh, what="gpu svd")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("seed", rs.SEEDS)
def test_stress_entry_vs_ref64(pol, oracle, fams, seed):
    """zs_rocm_mpm_stress, models 0-3, every family and parameter set"""
    failures = []
    for family in rs.FAMILIES:
        F, lj = fams[seed][family]
        for pset in rs.psets_of(family):
            R = rs.evaluate(pset, F, lj, rs.MEASURED_SVD[family][0])
            orc = oracle_stress_all(oracle, R.m, F, lj, key=(seed, family, pset))
            PF, Fp, ljn = _gpu_stress(pol, pset, F, lj)
            if R.m.model == 0:
                assert np.array_equal(Fp, F)
            e = rs.stress_errors(R, PF, Fp, ljn)
            gaps = rs.per_sample_gaps(R, (PF, Fp, ljn), orc)

            def mx(a, o):
                a = a[~R.near_of[o] & np.isfinite(a)]
                return a.max() if a.size else np.nan
            over = {o: int((gaps[o][~R.near_of[o] & np.isfinite(gaps[o])] > ORACLE_TOL).sum()) for o in gaps}   # at plain 1e-4
            print("REF64 stress gpu %s %s PF %s F %s logJp %s asym %s | vs oracle PF %s F %s logJp %s F/tol %s over %d %d %d" % (
                family, pset, _fmt(mx(e["PF"], "PF")), _fmt(mx(e["F"], "F")), _fmt(mx(e["lj"], "lj")), _fmt(mx(e["asym"], "PF")),
                _fmt(mx(gaps["PF"], "PF")), _fmt(mx(gaps["F"], "F")), _fmt(mx(gaps["lj"], "lj")),
                _fmt(mx(gaps["F"] / (ORACLE_TOL * R.ampF), "F")), over["PF"], over["F"], over["lj"]))
            if R.m.model == 1:      # sand tau is symmetric: to rounding on every finite sample, near a boundary or not
                asym = e["asym"][np.isfinite(e["asym"])]
                if asym.size and asym.max() > SAND_ASYM:
                    failures.append("gpu %s %s: asymmetry of sand's P F^T vol %.3g > %.3g of the scale" % (family, pset, asym.max(), SAND_ASYM))
            _collect(failures, rs.check_stress, family, pset, R, PF, Fp, ljn, what="gpu", per_sample=orc + (ORACLE_TOL,))
    assert not failures, "\n".join(failures)


def test_eos_entry_vs_ref64(pol, fams):
    """the fluid through zs_rocm_mpm_stress with J in place of F: the spread of eos_J (J^7 up to the float32 range) against eos_pf64
    and its rounding bound, and component 0 of every family (negative, zero and tiny J: the same finite pattern as float32 numpy)"""
    seed = rs.SEEDS[0]
    k = dict(rs._BASE, model=4)
    m = rs.material(k)
    J = rs.eos_J(seed)
    F = np.zeros((len(J), 9), np.float32)
    F[:, 0] = J
    PF, Fp, _ = _gpu_stress(pol, k, F, np.zeros(len(J), np.float32))
    want, bound = ref64.eos_pf64(J, m.bulk, m.volume)
    r = np.abs(PF - want)[:, [0, 4, 8]] / bound[:, [0, 4, 8]]
    print("REF64 stress gpu eos err/bound %.3f" % r.max())
    assert np.isfinite(PF).all() and r.max() <= 1.0 and (PF[:, [1, 2, 3, 5, 6, 7]] == 0).all()
    for family in rs.FAMILIES:
        F = fams[seed][family][0]
        PF, _, _ = _gpu_stress(pol, k, F, np.zeros(len(F), np.float32))
        host = eos_f32(F[:, 0], m.bulk, m.volume)
        fin = np.isfinite(host).all(1)
        assert np.array_equal(np.isfinite(PF).all(1), fin), family
        want, bound = ref64.eos_pf64(F[fin, 0], m.bulk, m.volume)
        with np.errstate(all="ignore"):
            ok = np.isfinite(want).all(1) & np.isfinite(bound).all(1)
            r = (np.abs(PF[fin] - want)[:, [0, 4, 8]] / bound[:, [0, 4, 8]])[ok]
        assert r.size == 0 or r.max() <= 1.0, (family, r.max())


@pytest.mark.parametrize("lane_width", [32, 64])
def test_update_stress_vs_ref64(pol, fams, lane_width):
    """the production instantiation model_stress<MODEL, WRITE_F = false> (update_stress_kernel): an MpmTransfer with cache_stress holds
    the family's F and logJp at arbitrary positions, update_stress() writes the six packed components and logJp"""
    from zpc_amd import lib
    from zpc_amd.mpm import MpmTransfer
    seed = rs.SEEDS[0]
    failures, worst = [], {}
    g = np.random.Generator(np.random.PCG64(5))
    for family in rs.FAMILIES:
        F, lj = fams[seed][family]
        n = len(F)
        pos = (0.3 + 0.2 * g.random((n, 3))).astype(np.float32)
        zero3, zero9 = np.zeros((n, 3), np.float32), np.zeros((n, 9), np.float32)
        for pset in rs.psets_of(family) + ("eos",):
            k = dict(rs._BASE, model=4) if pset == "eos" else rs.PSETS[pset]
            model = k["model"]
            mt = MpmTransfer(pol, n, 1 / 64, 1e-4, side=4, lane_width=lane_width, volume=rs.VOLUME, cache_stress=True, **k)
            mt.upload(np.ones(n, np.float32), pos, zero3, zero9, F[:, :1] if model == 4 else F, lj if model in (1, 3) else None)
            mt.update_stress()
            pol.syncCtx()
            aos = torch.empty(n, mt.nchn, dtype=torch.float32, device="cuda")
            lib().zs_rocm_tv_to_aos_f32(pol.handle, mt.buf.data_ptr(), n, mt.nchn, mt.L, aos.data_ptr())
            pol.syncCtx()
            a = aos.cpu().numpy()
            S6 = a[:, mt.off["PF"]:mt.off["PF"] + 6]
            PF = S6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
            ljn = a[:, 25] if model in (1, 3) else lj
            assert np.array_equal(a[:, 16:16 + mt.nF], F[:, :mt.nF]), "update_stress must not store the projected F"
            ePF, eF, elj = _gpu_stress(pol, k, F, lj)
            pack = np.stack([ePF[:, 0], 0.5 * (ePF[:, 1] + ePF[:, 3]), 0.5 * (ePF[:, 2] + ePF[:, 6]), ePF[:, 4], 0.5 * (ePF[:, 5] + ePF[:, 7]),
                             ePF[:, 8]], 1).astype(np.float32)
            if model == 4:
                scale = np.maximum(np.abs(np.where(np.isfinite(pack), pack, 0)).max(1), rs.material(k).bulk * rs.VOLUME)
            else:
                R = rs.evaluate(pset, F, lj, rs.MEASURED_SVD[family][0])
                scale = R.scale
                _collect(failures, rs.check_stress, family, pset, R, PF, R.F, ljn, what="gpu update_stress L%d" % lane_width)
            fin = np.isfinite(pack).all(1)
            if not np.array_equal(np.isfinite(S6).all(1), fin) or (model in (1, 3) and not np.array_equal(np.isfinite(ljn), np.isfinite(elj))):
                failures.append("%s %s: finite pattern of update_stress differs from the test entry's" % (family, pset))
            with np.errstate(all="ignore"):
                gap = (np.abs(S6.astype(np.float64) - pack).max(1) / scale)[fin]
                gl = np.abs(ljn.astype(np.float64) - elj)[np.isfinite(elj)] if model in (1, 3) else np.zeros(1)
            gap = gap.max() if gap.size else 0.0
            gl = gl.max() if gl.size else 0.0
            print("REF64 stress gpu update_stress L%d %s %s: vs test entry PF %s logJp %s" % (lane_width, family, pset, _fmt(gap), _fmt(gl)))
            worst[model] = max(worst.get(model, 0.0), gap)
            if gap > 4 * PROD_GAP[model]:
                failures.append("%s %s: update_stress differs from the test entry by %.3g of the scale" % (family, pset, gap))
            if model in PROD_GAP_LOGJP and gl > 4 * PROD_GAP_LOGJP[model]:
                failures.append("%s %s: logJp of update_stress differs from the test entry's by %.3g" % (family, pset, gl))
    print("REF64 stress gpu update_stress L%d worst gap per model %s" % (lane_width, {m: "%.2e" % v for m, v in worst.items()}))
    assert not failures, "\n".join(failures)
