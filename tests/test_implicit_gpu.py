"""The implicit-MPM system on the GPU: zs_rocm_mpm_implicit_force stage by stage against the float64 reference (tests/ref64_implicit.py)
and the oracle's stress, the two paths against each other (fresh and stale bins), multiply / project / precondition, the dof operators
and the CG solve on the configuration with a closed-form answer.  Prints one `IMPLICIT <what> <worst err / bound>` line per check."""
import ctypes as C

import numpy as np
import pytest

import ref64
import ref64_implicit as ri
from util import rng, move_after_binning, OracleMpm, oracle_stress

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_mpm_ref64_gpu import _read_all, _fields, _stress_tol  # noqa: E402  (the project's own stress tolerance, not a new one)

DX, DT = ri.DX, ri.DT
U = ref64.U


def _setup(pol, model, side, cloud, binned, with_mass=False, layout=None, **over):
    from zpc_amd.mpm import MpmTransfer
    m, x, v, Cm, state, lj = ri.implicit_case(cloud, model)
    n = x.shape[0]
    kw = dict(ri.model_kw(model))
    kw.update(over)
    mt = MpmTransfer(pol, n, DX, DT, model=model, side=side, volume=DX ** 3 / 8, **dict(kw, **(layout or {})))
    mt.upload(m, x, v, Cm, state, lj if model in (1, 3) else None)
    mt.build_partition(n)
    if mt.key_is_origin:
        assert (mt.active_keys() % side == 0).all()
    if binned:
        mt.rebin()
    if with_mass:
        mt.clear_grid()
        mt.p2g()
        pol.syncCtx()
    coords = ri.dof_world(mt, np.zeros((mt.nblocks * side ** 3, 3)))[0]
    vin = ri.trial_velocity(coords, ri.cloud_centre(x), scale=ri.TRIAL_SCALE[cloud])
    return mt, x, coords, vin, kw


def _force(mt, vin_t, binned, trial=True):
    out = mt.dof_vector()
    tr = torch.full((mt.n, 27), float("nan"), dtype=torch.float32, device="cuda") if trial else None
    mt.implicit_force(vin_t, out, trial=tr, binned=binned)
    mt.pol.syncCtx()
    return out.cpu().numpy(), (tr.cpu().numpy() if trial else None)


def _mass(mt):
    return mt.grid.cpu().numpy().reshape(mt.nblocks, 7, mt.side ** 3)[:, 0, :].reshape(-1)


# ------------------------------------------------------------------------------------------------ 4: the force operator, stage by stage
@pytest.mark.parametrize("cloud", ri.CLOUDS)
@pytest.mark.parametrize("side", [4, 8])
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("binned", [False, True])
def test_implicit_force_stage_by_stage(pol, oracle, binned, model, side, cloud):
    _stage_by_stage(pol, oracle, binned, model, side, cloud)


LAYOUTS = {"origin_keys": dict(key_is_origin=True), "lanes32": dict(lane_width=32), "aos": dict(aos=True)}


@pytest.mark.parametrize("binned", [False, True])
@pytest.mark.parametrize("side,model", [(8, 0), (4, 1), (8, 4)])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_implicit_force_other_keys_and_particle_layouts(pol, oracle, layout, side, model, binned):
    """the same stage-by-stage check with the SparseGrid key convention (partition keys are block origins) on the cloud that straddles
    0, with 32-lane tiles and with AoS particle storage (the generic iterator ports): the kscale arithmetic and the LW = 32 / 0
    instantiations of the binned kernel"""
    _stage_by_stage(pol, oracle, binned, model, side, "edge", layout=LAYOUTS[layout])


def _stage_by_stage(pol, oracle, binned, model, side, cloud, layout=None):
    """C_trial and F_trial / J_trial of every particle against ref64.g2p64 on the same dof velocities (b_C, b_F / b_J); the stored
    P F^T vol against the oracle's stress of the GPU's own stored F_trial within 1e-4 of the row scale (_stress_tol), every particle
    (CPU: test_oracle_stress_is_finite_on_every_trial_state); fOut against the float64 scatter of the GPU's own stored P F^T vol, every
    node, e_in = 0; the particle buffer bit-identical afterwards (logJp included)."""
    mt, x, coords, vin, kw = _setup(pol, model, side, cloud, binned, layout=layout)
    vin_t = torch.from_numpy(vin).cuda()
    before = mt.buf.clone()
    f, tr = _force(mt, vin_t, binned)
    assert torch.equal(before.view(torch.int32), mt.buf.view(torch.int32)), "the operator changed the particle buffer"
    assert np.isfinite(tr).all(), "trial hook: particles without a record"
    a = _read_all(mt)
    p = _fields(a, mt)
    lj = a[:, 25] if model in (1, 3) else None
    path = "force[%s m%d s%d %s%s]" % ("binned" if binned else "particle", model, side, cloud, " " + str(layout) if layout else "")
    r = ri.trial64((coords, vin), p["x"], p["F"], model)
    out = [ref64.check_particles(tr[:, :9], r["C"], r["b_C"], path + " C_trial")]
    if model == 4:
        out.append(ref64.check_particles(tr[:, 9], r["J"], r["b_J"], path + " J_trial"))
        assert (tr[:, 10:18] == 0).all()
    else:
        out.append(ref64.check_particles(tr[:, 9:18], r["F"], r["b_F"], path + " F_trial"))
    om = OracleMpm(oracle, model, DX, DT, side, DX ** 3 / 8, **kw)
    Ft, PF = np.ascontiguousarray(tr[:, 9:18]), tr[:, 18:27]
    PFo = oracle_stress(oracle, om, np.ascontiguousarray(tr[:, :9]), Ft, lj)
    assert np.isfinite(PFo).all()
    tol = _stress_tol(om, PFo, Ft)
    ratio = np.abs(PF - PFo) / tol
    out.append(float(ratio.max()))
    assert (ratio <= 1).all(), "%s: %d stress components over 1e-4 of the row scale, worst %.3g" % (path, int((ratio > 1).sum()), ratio.max())
    ref = ri.force64(PF, p["x"], DX)
    out.append(np.nanmax(ref64.check_grid(ref, ri.dof_world(mt, f), range(4, 7), path + " fOut")))
    print("IMPLICIT %s C %.3f F/J %.3f stress %.3f fOut %.3f" % (path, *out))


# ------------------------------------------------------------------------------------------------ 5, 6: the two paths, the hook
def _two_bounds_ratio(mt, p, fa, tra, fb, trb, propagate):
    """worst |fa - fb| / (bound_a + bound_b) over the touched nodes, each bound from that run's own stored P F^T vol (e_in = 0);
    propagate: plus the scatter of |PF_a - PF_b|, ref64's e_in of an input that is itself a kernel result"""
    ra = ri.force64(tra[:, 18:27], p["x"], DX, ePF=np.abs(tra[:, 18:27].astype(np.float64) - trb[:, 18:27]) if propagate else None)
    rb = ri.force64(trb[:, 18:27], p["x"], DX)
    assert np.array_equal(ra.keys, rb.keys)
    bound = ra.bound()[:, 4:7] + rb.bound()[:, 4:7]
    coords, _ = ri.dof_world(mt, fa)
    row = ra.lookup(coords)
    fa, fb = fa.reshape(-1, 3).astype(np.float64), fb.reshape(-1, 3).astype(np.float64)
    assert (fa[row < 0] == 0).all() and (fb[row < 0] == 0).all()
    assert (np.sort(row[row >= 0]) == np.arange(len(ra.keys))).all()
    return float((np.abs(fa - fb)[row >= 0] / bound[row[row >= 0]]).max())


def _both_paths(pol, model, side, cloud):
    """(stage, mt, particles, binned fOut / trial, particle-order fOut / trial, binned fOut without the hook) for fresh bins and after
    a sixth of the inner particles moved after binning (another cell of the bin, another bin, another block)"""
    mt, x, coords, vin, kw = _setup(pol, model, side, cloud, True)
    vin_t = torch.from_numpy(vin).cuda()
    for stage in ("fresh", "stale"):
        if stage == "stale":
            _, moved = move_after_binning(mt, x, frac=0.9)   # (the inner region of the 6-cell lattice cloud holds 64 particles)
            assert moved.sum() > 20
        p = _fields(_read_all(mt), mt)
        fb, trb = _force(mt, vin_t, True)
        fp, trp = _force(mt, vin_t, False)
        fn, _ = _force(mt, vin_t, True, trial=False)
        # fresh or stale, the binned path is judged by the float64 scatter node by node
        ref64.check_grid(ri.force64(trb[:, 18:27], p["x"], DX), ri.dof_world(mt, fb), range(4, 7), "binned fOut, %s bins" % stage)
        yield stage, mt, p, fb, trb, fp, trp, fn


PATH_CASES = [(m, s, c) for c in ri.CLOUDS for s in (4, 8) for m in (0, 1, 2, 3, 4)]


@pytest.mark.parametrize("model,side,cloud", PATH_CASES)
def test_binned_path_equals_particle_order_path_with_fresh_and_stale_bins(pol, model, side, cloud):
    """fOut of the two paths within the sum of their two node bounds (each from its own stored P F^T vol, e_in = 0), with fresh bins
    and with stale ones.

    This holds because both paths form C_trial by the same arithmetic: the particle-order kernel fetches its 27 node velocities by
    hash query and then sums them with g2p_gather_lds on a private 3^3 arena, in the binned kernel's sum-factorised order.  It does
    NOT sum in the reference's node-by-node order.  An earlier node-by-node gather passed every stage check but missed this one by
    5-50x (FixedCorotated 17.7, DruckerPrager 52.1, fluid 5.4 at worst): a few ulp of difference in F_trial become ~100 u of
    P F^T vol ~ 2 mu (F - R) vol at 1 % strain, against (N + 23) u ~ 30-90 u per node from the scatter itself.
    The price: a defect in g2p_gather_lds would show alike on both paths and this test could not see it; the check of C_trial against
    ref64.g2p64 (test_implicit_force_stage_by_stage, both paths) is the independent one."""
    worst = {}
    for stage, mt, p, fb, trb, fp, trp, fn in _both_paths(pol, model, side, cloud):
        worst[stage] = _two_bounds_ratio(mt, p, fb, trb, fp, trp, False)
        assert np.array_equal(trb[:, :18].view(np.uint32), trp[:, :18].view(np.uint32)), "the two paths formed different trial states"
    print("IMPLICIT paths[m%d s%d %s] binned vs particle, e_in = 0: %s" % (model, side, cloud, worst))
    assert max(worst.values()) <= 1, worst


@pytest.mark.parametrize("model,side,cloud", PATH_CASES)
def test_trial_hook_changes_no_value_and_paths_agree_within_propagated_bounds(pol, model, side, cloud):
    """the trial hook changes no value: with and without it the binned kernel's fOut lie within the two node bounds (e_in = 0) of each
    other.  And the path comparison once more with the stress difference of the two runs propagated (f_a = S(PF_a) +- bound_a, f_b =
    S(PF_b) +- bound_b, S linear: |f_a - f_b| <= bound_a + bound_b + S_abs(|PF_a - PF_b|), ref64's e_in): the form that holds for
    any two correct gathers, looser than the test above."""
    for stage, mt, p, fb, trb, fp, trp, fn in _both_paths(pol, model, side, cloud):
        r = _two_bounds_ratio(mt, p, fb, trb, fp, trp, True)
        h = _two_bounds_ratio(mt, p, fb, trb, fn, trb, False)
        print("IMPLICIT paths[m%d s%d %s %s] binned vs particle (propagated) %.3f, hook vs no hook %.3f" % (model, side, cloud, stage, r, h))
        assert r <= 1 and h <= 1


# ------------------------------------------------------------------------------------------------ 7: multiply
@pytest.mark.parametrize("side,binned,model", [(8, True, 0), (4, True, 1), (8, False, 4), (4, False, 0)])
def test_implicit_multiply_entrywise(pol, side, binned, model):
    """out = (f dt dt + m) v on entries whose node has mass, 0 elsewhere, from the GPU's own fOut (a launch of its own), m and vIn,
    within 3 u (|f| dt^2 + m) |v| + dt^2 |v| bound(f), bound(f) = (N + C_F) u T of the node (ref64).
    The first term: the kernel computes fl(fma(fl(f dt), dt, m) v), three roundings, each of relative size u on a quantity bounded by
    (|f| dt^2 + m) |v| (ref64's first-order counting: every factor's relative error once).  The second: the f inside the multiply's
    launch is another sum of the same terms.  Against the fOut read back here, itself a rounded sum, that term is asserted as
    specified (one bound(f)); against the float64 scatter of the stored P F^T vol (the exact sum both launches approximate: the hook
    changes no value, the stress of a particle is the same bits in both) the same bound is rigorous, and is asserted too."""
    mt, x, coords, vin, kw = _setup(pol, model, side, "lattice", binned, with_mass=True)
    vin_t = torch.from_numpy(vin).cuda()
    f, tr = _force(mt, vin_t, binned)
    out = torch.full_like(vin_t, float("nan"))
    mt.implicit_multiply(vin_t, out, binned=binned)
    pol.syncCtx()
    got = out.cpu().numpy().reshape(-1, 3).astype(np.float64)
    mass = _mass(mt).astype(np.float64)
    has = mass > 0
    v64, dt = vin.astype(np.float64), float(np.float32(DT))
    ref = ri.force64(tr[:, 18:27], _fields(_read_all(mt), mt)["x"], DX)
    row = ref.lookup(coords)
    bf = np.where(row[:, None] >= 0, ref.bound()[np.maximum(row, 0), 4:7], 0.0)
    exact = np.where(row[:, None] >= 0, ref.val[np.maximum(row, 0), 4:7], 0.0)
    assert has.sum() > 100 and (~has).sum() > 100
    worst = []
    for f64 in (f.reshape(-1, 3).astype(np.float64), exact):
        want = (f64 * dt * dt + mass[:, None]) * v64
        bound = 3 * U * (np.abs(f64) * dt * dt + mass[:, None]) * np.abs(v64) + dt * dt * np.abs(v64) * bf
        err = np.abs(got - want)[has]
        worst.append(float(np.where(err > 0, err / np.maximum(bound[has], 1e-300), 0.0).max()))
    print("IMPLICIT multiply[s%d %s m%d] from the GPU's fOut %.3f, from the float64 scatter %.3f" % (side, "binned" if binned else "particle",
                                                                                                  model, worst[0], worst[1]))
    assert worst[0] <= 1 and worst[1] <= 1, worst
    assert (got[~has] == 0).all()


# ------------------------------------------------------------------------------------------------ 8: project
@pytest.mark.parametrize("ctype", [0, 1, 2])
@pytest.mark.parametrize("geometry", ["sphere", "plane"])
@pytest.mark.parametrize("side", [4, 8])
def test_implicit_project_equals_collider_resolve_bit_for_bit(pol, side, geometry, ctype):
    from zpc_amd import lib
    from zpc_amd.mpm import make_collider, SPHERE, PLANE
    mt, x, coords, vin, kw = _setup(pol, 0, side, "lattice", False, with_mass=True)
    c0 = ri.cloud_centre(x)
    col = make_collider(SPHERE, ctype, (c0[0], c0[1], c0[2], 2.5 * DX)) if geometry == "sphere" else \
        make_collider(PLANE, ctype, (c0[0], c0[1], c0[2], 0.0, 1.0, 0.0))
    nn = coords.shape[0]
    v0 = rng(77).standard_normal((nn, 3)).astype(np.float32)
    pos = torch.from_numpy(np.ascontiguousarray(coords.astype(np.float32) * np.float32(DX))).cuda()   # (float)node * dx, as the kernel
    want = torch.from_numpy(v0).cuda()
    inside = torch.zeros(nn, dtype=torch.int32, device="cuda")
    lib().zs_rocm_collider_resolve(pol.handle, C.byref(col), pos.data_ptr(), want.data_ptr(), nn, inside.data_ptr())
    got = torch.from_numpy(v0).cuda()
    mt.implicit_project(col, got)
    only_zero = torch.from_numpy(v0).cuda()
    mt.implicit_project(None, only_zero)
    pol.syncCtx()
    has = _mass(mt) > 0
    got, want, only_zero, inside = got.cpu().numpy(), want.cpu().numpy(), only_zero.cpu().numpy(), inside.cpu().numpy()
    assert (inside[has] != 0).sum() > 20 and (inside[has] == 0).sum() > 20
    assert np.array_equal(got[has].view(np.uint32), want[has].view(np.uint32))
    assert (got[~has] == 0).all() and (only_zero[~has] == 0).all()
    assert np.array_equal(only_zero[has].view(np.uint32), v0[has].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 9: precondition
@pytest.mark.parametrize("side", [4, 8])
def test_implicit_precondition(pol, side):
    """out = in / m by an IEEE division: one rounding (u |in / m|); entries of nodes without mass keep their bits"""
    mt, x, coords, vin, kw = _setup(pol, 0, side, "mixed", False, with_mass=True)
    nn = coords.shape[0]
    a = rng(5).standard_normal((nn, 3)).astype(np.float32)
    sentinel = rng(6).standard_normal((nn, 3)).astype(np.float32)
    out = torch.from_numpy(sentinel).cuda()
    mt.implicit_precondition(torch.from_numpy(a).cuda(), out)
    pol.syncCtx()
    got = out.cpu().numpy()
    mass = _mass(mt).astype(np.float64)
    has = mass > 0
    want = a[has].astype(np.float64) / mass[has, None]
    assert (np.abs(got[has] - want) <= U * np.abs(want) + ref64.FLT_MIN).all()
    assert np.array_equal(got[~has].view(np.uint32), sentinel[~has].view(np.uint32)) and (~has).sum() > 100


# ------------------------------------------------------------------------------------------------ 10: dof operators
@pytest.mark.parametrize("n", [1, 1000, 300007])
def test_dof_operators(pol, n):
    from zpc_amd import lib
    L, g = lib(), rng(n)
    a, b = g.standard_normal(n).astype(np.float32), (g.standard_normal(n) + 0.1).astype(np.float32)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    tc = torch.empty_like(ta)
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    L.zs_rocm_dof_assign(pol.handle, ta.data_ptr(), tc.data_ptr(), n)
    pol.syncCtx()
    assert np.array_equal(bits(tc), a.view(np.uint32))
    L.zs_rocm_dof_fill(pol.handle, tc.data_ptr(), 0.3, n)
    pol.syncCtx()
    assert np.array_equal(bits(tc), np.full(n, 0.3, np.float32).view(np.uint32))
    for op, fn in ((0, np.add), (1, np.multiply), (2, np.subtract)):
        assert L.zs_rocm_dof_compwise(pol.handle, op, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), n) == 0
        pol.syncCtx()
        assert np.array_equal(bits(tc), fn(a, b).view(np.uint32)), op
    assert L.zs_rocm_dof_compwise(pol.handle, 3, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), n) == 0
    pol.syncCtx()
    q = a.astype(np.float64) / b.astype(np.float64)
    assert (np.abs(tc.cpu().numpy() - q) <= U * np.abs(q) + ref64.FLT_MIN).all()
    tc.fill_(7.0)
    assert L.zs_rocm_dof_compwise(pol.handle, 4, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), n) == -1
    pol.syncCtx()
    assert (tc == 7.0).all()
    m_, n_ = np.float32(0.37), np.float32(-1.9)
    L.zs_rocm_dof_linear_combine(pol.handle, float(m_), ta.data_ptr(), float(n_), tb.data_ptr(), tc.data_ptr(), n)
    pol.syncCtx()
    ma, nb = float(m_) * a.astype(np.float64), float(n_) * b.astype(np.float64)
    assert (np.abs(tc.cpu().numpy() - (ma + nb)) <= 2 * U * (np.abs(ma) + np.abs(nb)) + 2 * ref64.FLT_MIN).all()
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    L.zs_rocm_dof_dot(pol.handle, ta.data_ptr(), tb.data_ptr(), n, out.data_ptr())
    pol.syncCtx()
    prod = a.astype(np.float64) * b.astype(np.float64)
    err = abs(float(out.item()) - prod.sum())
    print("IMPLICIT dot n=%d err / bound %.3g" % (n, err / (n * U * np.abs(prod).sum())))
    assert err <= n * U * np.abs(prod).sum() + n * ref64.FLT_MIN


# ------------------------------------------------------------------------------------------------ 11: solve
@pytest.mark.parametrize("side,binned", [(8, True), (4, False)])
def test_implicit_solve_closed_form(pol, side, binned):
    """Fluid with bulk = 0 and viscosity = 0: P F^T vol = 0, so A = diag(m) on nodes with mass and the preconditioner is its inverse: CG
    returns x = P(b / m) after one iteration in exact arithmetic; a second one is allowed for a rounding-size residual.
    b = s m v_target with s = 1 / sqrt(sum m v_target^2): the first preconditioned norm sqrt(r . M r) is then 1, localTol =
    min(0.5 * 1, 1e-6) = 1e-6, and the residual after the first iteration, |1 - alpha| ~ a few u times that norm, lies below it.
    Error of x on free nodes: start x = 0, so r = b exactly, q = p = fl(b / m) (1 u), temp = fl(m p) (1 more u); alpha = (r . q) /
    (temp . p) is 1 in exact arithmetic; each dot product is within n u of its sum of magnitudes (the bound of test_dof_operators; all
    its terms are >= 0, so that is a relative error) and its terms carry 1 u and 3 u: |alpha - 1| <= 2 n u + 4 u.  x = fl(alpha p): two
    more roundings.  A second iteration adds a correction of relative size |alpha - 1| computed with the same relative error, i.e.
    second order, and three more roundings (its own q, alpha p, the sum).  Bound: (2 n + 10) u |b / m|, n = entries of a dof vector."""
    from zpc_amd import lib
    from zpc_amd.mpm import make_collider, SPHERE, STICKY
    mt, x, coords, vin, kw = _setup(pol, 4, side, "lattice", binned, with_mass=True, bulk=0.0, viscosity=0.0)
    nn = coords.shape[0]
    mass = _mass(mt).astype(np.float64)
    has = mass > 0
    c0 = ri.cloud_centre(x)
    col = make_collider(SPHERE, STICKY, (c0[0], c0[1], c0[2], 2.5 * DX))
    pos = coords.astype(np.float64) * DX
    stuck = has & (np.linalg.norm(pos - c0, axis=1) < 2.4 * DX)
    free = has & (np.linalg.norm(pos - c0, axis=1) > 2.6 * DX)
    assert stuck.sum() > 20 and free.sum() > 100
    vt = rng(21).standard_normal((nn, 3))
    s = 1.0 / np.sqrt((mass[:, None] * vt ** 2).sum())
    b = (s * mass[:, None] * vt).astype(np.float32)
    b[~has] = rng(22).standard_normal(((~has).sum(), 3)).astype(np.float32)   # junk on nodes without mass: projected away
    tb, tx = torch.from_numpy(b).cuda(), mt.dof_vector()
    iters = mt.implicit_solve(tb, tx, collider=col, binned=binned)
    pol.syncCtx()
    got = tx.cpu().numpy().astype(np.float64)
    assert 1 <= iters <= 2, iters
    assert (got[stuck] == 0).all() and (got[~has] == 0).all()
    want = b[free].astype(np.float64) / mass[free, None]
    bound = (2 * 3 * nn + 10) * U * np.abs(want) + 10 * ref64.FLT_MIN
    ratio = np.abs(got[free] - want) / bound
    print("IMPLICIT solve[s%d %s] iters %d err / bound %.3g, worst relative error %.3g" % (side, "binned" if binned else "particle", iters,
                                                                                        ratio.max(), (np.abs(got[free] - want) / np.abs(want)).max()))
    assert (ratio <= 1).all()
    # argument checks: maxIters = 0 leaves x as it is; a bad side is refused with nothing written
    sentinel = rng(23).standard_normal((nn, 3)).astype(np.float32)
    tx = torch.from_numpy(sentinel).cuda()
    assert mt.implicit_solve(tb, tx, max_iters=0, collider=col, binned=binned) == 0
    pol.syncCtx()
    assert np.array_equal(tx.cpu().numpy().view(np.uint32), sentinel.view(np.uint32))
    good = mt.params.side
    try:
        mt.params.side = 5
        it = C.c_int(-7)
        rc = lib().zs_rocm_mpm_implicit_solve(pol.handle, C.byref(mt.params), mt.particles(), mt.table.handle, mt.grid.data_ptr(), mt.nblocks,
                                              None, None, None, None, tb.data_ptr(), tx.data_ptr(), 10, 1e-6, 0.5, C.byref(it))
        rf = lib().zs_rocm_mpm_implicit_force(pol.handle, C.byref(mt.params), mt.particles(), mt.table.handle, mt.nblocks, None, None, None,
                                              tb.data_ptr(), tx.data_ptr(), None)
    finally:
        mt.params.side = good
    pol.syncCtx()
    assert rc == -1 and rf == -1 and it.value == -7
    assert np.array_equal(tx.cpu().numpy().view(np.uint32), sentinel.view(np.uint32))
