"""Float64 reference of the 3x3 SVD and of the five constitutive models of zpc_amd/csrc/mpm_math.hpp, written from the model
definitions (not from the float32 algorithm): numpy.linalg.svd in float64 brought to the math::svd convention, then every model as a
function of the singular values.  All five are isotropic, so with F = U diag(s) V^T

    P F^T vol   = U diag(k) U^T          k_i = principal Kirchhoff stress times the volume
    projected F = U diag(s') V^T

and the reference needs (k, s', logJp') as functions of (s, logJp) only.  The constants and clamps of the header (1e-4 on the singular
values, 1e-5 in the NACC yield pressure, the hardening guards) are part of the operation and are kept.  Parameters are the float32
values the kernels receive (make_dev), the arithmetic on them is float64.

Every model also returns a branch label per sample and, for every branch condition of the header, the float64 value of the quantity
that is compared with 0 there (`q`).  `margins()` propagates a singular-value error to these quantities (central differences of the
same float64 function), so that a caller can tell which samples sit too close to a branch boundary for a float32 evaluation to be held
to the float64 branch.  The 1e-4 clamps are continuous (a max), they are reported (`clamp`) but exclude nothing.

SCALE of a relative error, per sample:

    S, reconstruction      ||F||_2 (the largest float64 singular value), at least 2^-126
    P F^T vol              max(|PF64| row max, (2 mu + lam) vol max(1, |F - I|max, Jterm))      (bulk vol for the fluid)
                           Jterm = J^2 for FixedCorotated and von Mises, whose volumetric Kirchhoff stress lam (J - 1) J grows with
                           J^2 (the x1e3 family), 0 for the logarithmic and the projected models; for F near I this is the row scale
                           of tests/test_mpm_gpu.py::test_svd_and_stress_blocks
    projected F            max(|F|max, |F'64|max)
    logJp                  max(1, |logJp'64|)

Matrices are 9-vectors in column-major order (M[r + 3 c]).  numpy only; shared by tests/test_stress_ref64_cpu.py (oracle/mpm.c
against this reference) and tests/test_stress_ref64_gpu.py (the kernels against it, under the ceilings measured from the oracle)."""
import numpy as np

from ref64 import U as U32, FLT_MIN, _mat, _vec9

VOLUME = 2.5e-7
YIELD_SURFACE = 0.816496580927726 * 2.0 * 0.5 / (3.0 - 0.5)
N_FAMILY = 2048
SEEDS = (20260, 20261, 20262)   # MEASURED_* is the worst of the three; the tests run all three

# parameter sets: name -> keyword arguments in the spelling of zpc_amd.mpm.MpmTransfer
_BASE = dict(E=5e4, nu=0.4, cohesion=0.0, beta=1.0, yield_surface=YIELD_SURFACE, vol_correction=True, yield_stress=500.0, xi=0.8,
             friction_angle=45.0, hardening=True, bulk=4e4, viscosity=0.0)
PSETS = {
    "fc": dict(_BASE, model=0),
    "sand": dict(_BASE, model=1),
    "sand_coh": dict(_BASE, model=1, cohesion=0.05, beta=0.5),      # cohesion != 0: exp(cohesion), the shifted cone
    "sand_novc": dict(_BASE, model=1, vol_correction=False),
    "sand_mu0": dict(_BASE, model=1, E=0.0),                        # mu == 0: the corner that is labelled, not valued
    "vm": dict(_BASE, model=2),
    "nacc": dict(_BASE, model=3, beta=0.5),
    "nacc_nohard": dict(_BASE, model=3, beta=0.5, hardening=False),
}
MAIN_PSETS = ("fc", "sand", "vm", "nacc")
EXTRA_PSETS = ("sand_coh", "sand_novc", "sand_mu0", "nacc_nohard")
EXTRA_FAMILIES = ("benign", "near_identity", "compressed")           # the families the extra parameter sets run on
MODEL_NAMES = {0: "FixedCorotated", 1: "DruckerPrager", 2: "VonMisesFixedCorotated", 3: "NACC", 4: "EquationOfState"}
# Samples near a branch boundary are left out of the value comparisons by rule (evaluate), per output, and the share left out of an
# output is capped at EXCLUDED_CAP.  On the pairs below the rule leaves out (nearly) a whole family by construction of the family, so
# the cap on the named outputs says nothing there and is not asserted; everything else -- the finite pattern, the ceilings, the
# asymmetry and the comparison with the oracle on the samples the rule keeps, and the cap on the other outputs -- stays.
#   rank1, tiny x all models: projected F.  Two vanishing singular values (rank 1), or an F under the absolute guards of the SVD (tiny:
#       1e-20 on the squared off-diagonal of F^T F, 1e-12 in the QR; no rotation is made and S is wrong by O(||F||), MEASURED_SVD): the
#       rotations U, V are not unique, so U diag(s') V^T is not.  P F^T vol = U diag(k) U^T has k1 = k2 there and is well-posed.
#   rank2, rank1, tiny, wide x NACC: all outputs.  J = s0 s1 s2 is 0 up to the rounding of F (wide: s2 reaches under the family's S
#       error), and NACC takes the logarithm, the reciprocal and a fractional power of J: its sign is noise.
#   x1e3 x von Mises: all outputs.  At tau ~ lam J^2 = 1e23 the deviator is lost to rounding (1e16 against 1e11), every sample yields and
#       projects to s' ~ 1e9, where P ~ lam J s'^2 = 1e52 overflows float32 in kernel and oracle alike.  The reference marks the samples
#       whose float64 stress leaves the float32 range (`beyond`) and they count as near a boundary.
_ALL = ("PF", "F", "lj")
CAP_EXEMPT = {(f, p): ("F",) for f in ("rank1", "tiny") for p in ("fc", "sand", "vm")}
CAP_EXEMPT.update({(f, "nacc"): _ALL for f in ("rank2", "rank1", "tiny", "wide")})
CAP_EXEMPT[("scaled_up", "vm")] = _ALL
EXCLUDED_CAP = 0.05
COND_ROUND, COND_TOL = 16 * 2.0 ** -24, 1e-4
MARGIN_FACTOR = 4.0
FLT_MAX = 3.4028234663852886e38
# ceilings: CEIL_FACTOR x the measured error of the oracle, never below a rounding floor (see ceiling())
CEIL_FACTOR = 2.0
FLOOR_SVD, FLOOR_STRESS = 16 * U32, 256 * U32
# Pairs on which the ORACLE's P F^T vol is further from float64 than the 1e-4 the kernels are held to it, for a reason that is the
# oracle's own: it forms sand's P F_e^T through V, and V^T V - I (1e-7) is amplified there by s_max / s_min, where the kernel forms
# U diag(tau) U^T (measured on the MI355X, 2026-10-18: kernel against float64 1.9e-5 on rank2 and 4.5e-7 on rank1; 3.0 ... 3.7e-3 on
# wide, where the truncation error of log s2 dominates both, with up to 2.3e-3 between them).  Value: the oracle's measured error
# against float64 (MEASURED_STRESS, CPU).  Only on these pairs may a sample differ
# from the oracle by more than the tolerance, and then it has to be no further from float64 than the oracle is, plus the tolerance.
ORACLE_OWN_ERROR = {("wide", "sand"): 3.75e-3, ("rank2", "sand"): 3.48e-3, ("rank1", "sand"): 3.78e-3}
# the float64 quantities whose boundary separates a finite from a non-finite result
NONFINITE_Q = ("disc", "Je")


def psets_of(family):
    return MAIN_PSETS + (EXTRA_PSETS if family in EXTRA_FAMILIES else ())


# ------------------------------------------------------------------------------------------------ material
class Material:
    """the float32 parameters the kernels work with (make_dev, mpm_particles.hpp), as Python floats"""

    def __init__(self, model, E, nu, cohesion, beta, yield_surface, vol_correction, yield_stress, xi, friction_angle, hardening, bulk,
                 viscosity, volume=VOLUME):
        f = np.float32
        E, nu = f(E), f(nu)
        self.model = model
        self.volume = float(f(volume))
        self.mu = float(f(0.5 * float(E) / (1 + float(nu))))
        self.lam = float(f(float(E) * float(nu) / ((1 + float(nu)) * (1 - 2 * float(nu)))))
        self.cohesion, self.beta, self.yield_surface = float(f(cohesion)), float(f(beta)), float(f(yield_surface))
        self.vol_correction, self.hardening = bool(vol_correction), bool(hardening)
        self.yield_stress, self.xi = float(f(yield_stress)), float(f(xi))
        self.bm = float(f(2) / f(3) * (E / (f(2) * (f(1) + nu))) + E * nu / ((f(1) + nu) * (f(1) - f(2) * nu)))
        sin_phi = f(np.sin(f(friction_angle)))                       # NACCConfig: the angle goes to sin() as it is
        mcf = f(np.sqrt(f(2) / f(3))) * f(2) * sin_phi / (f(3) - sin_phi)
        M = mcf * f(3) / f(np.sqrt(f(2) / f(3)))
        self.Msqr = float(M * M)
        self.bulk, self.viscosity = float(f(bulk)), float(f(viscosity))
        smu = f(2) * f(self.mu)
        with np.errstate(all="ignore"):
            self.dp_coef = float((f(3) * f(self.lam) + smu) / smu)   # NaN for mu == 0, where it is never used
        self.modulus = (2 * self.mu + self.lam) if model != 4 else self.bulk


def material(pset):
    return Material(**PSETS[pset]) if isinstance(pset, str) else Material(**pset)


# ------------------------------------------------------------------------------------------------ SVD
def svd64(F):
    """F [n, 9] -> U [n, 3, 3], s [n, 3], V [n, 3, 3] in float64 with F = U diag(s) V^T, U and V rotations, |s0| >= |s1| >= |s2| and
    the sign on s2 (math::svd convention)"""
    A = _mat(F)
    Um, s, Vh = np.linalg.svd(A)
    Vm = Vh.transpose(0, 2, 1).copy()
    Um, s = Um.copy(), s.copy()
    for M in (Um, Vm):
        neg = np.linalg.det(M) < 0
        M[neg, :, 2] *= -1
        s[neg, 2] *= -1
    return Um, s, Vm


def _rot(g, n):
    q, r = np.linalg.qr(g.standard_normal((n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    q[np.linalg.det(q) < 0, :, 2] *= -1
    return q


FAMILIES = ("benign", "rotation", "near_identity", "repeated", "nearly_repeated", "wide", "inverted", "rank2", "rank1", "scaled_up",
            "scaled_down", "identity", "zero", "diagonal", "tiny", "compressed")


def families(seed, n=N_FAMILY):
    """name -> (F [n, 9] float32, logJp [n] float32).  F = U diag(s) V^T is built in float64 with random rotations and rounded to
    float32; the float32 matrix is the input of both sides.  logJp = -|0.2 N(0, 1)|, positive for 3 % of the samples: an unhardened
    NACC particle (logJp >= 0) has the yield pressure 1e-5 bm, so at J = 1 it sits closer to the case-2 boundary than any float32 SVD
    resolves, and a family near the rotations could not keep its excluded share under the cap with more of them."""
    g = np.random.Generator(np.random.PCG64(seed))
    eye = np.eye(3)[None]
    out = {}

    def usv(s, scale=1.0):
        return np.einsum("nik,nk,njk->nij", _rot(g, n), s, _rot(g, n)) * scale

    uni = lambda lo, hi, k=3: g.uniform(lo, hi, (n, k))
    out["benign"] = eye + 0.2 * g.standard_normal((n, 3, 3))                       # today's test input
    out["rotation"] = _rot(g, n)
    out["near_identity"] = eye + 1e-4 * g.standard_normal((n, 3, 3))
    ab = uni(0.5, 1.5, 2)
    rep = np.where((g.random(n) < 0.5)[:, None], ab[:, [0, 0, 1]], ab[:, [0, 1, 1]])
    out["repeated"] = usv(rep)
    out["nearly_repeated"] = usv(rep * (1 + 1e-5 * g.standard_normal((n, 3))))
    s0 = uni(0.5, 2.0, 1)
    out["wide"] = usv(np.concatenate([s0, s0 * 10 ** uni(-2, 0, 1), 10 ** uni(-4, -1, 1)], 1))
    s = -np.sort(-uni(0.3, 1.5), 1)
    s[:, 2] *= -1
    out["inverted"] = usv(s)
    s = uni(0.5, 1.5)
    s[:, 2] = 0
    out["rank2"] = usv(s)
    s = uni(0.5, 1.5)
    s[:, 1:] = 0
    out["rank1"] = usv(s)
    out["scaled_up"] = usv(uni(0.5, 1.5), 1e3)
    out["scaled_down"] = usv(uni(0.5, 1.5), 1e-3)
    out["identity"] = np.broadcast_to(eye, (n, 3, 3)).copy()
    out["zero"] = np.zeros((n, 3, 3))
    d = np.zeros((n, 3, 3))
    d[:, [0, 1, 2], [0, 1, 2]] = uni(0.5, 1.5)
    out["diagonal"] = d
    out["tiny"] = usv(uni(0.5, 1.5)) * 10 ** uni(-13, -10, 1)[:, :, None]       # straddles the 1e-20 and 1e-24 guards
    out["compressed"] = 0.9 * eye + 0.1 * g.standard_normal((n, 3, 3))            # mostly sand case I
    assert tuple(out) == FAMILIES
    lj = (np.abs(0.2 * g.standard_normal(n)) * np.where(g.random(n) < 0.03, 1.0, -1.0)).astype(np.float32)
    return {k: (np.ascontiguousarray(_vec9(v).astype(np.float32)), lj.copy()) for k, v in out.items()}


def eos_J(seed, n=N_FAMILY):
    """J of the fluid: around 1, and log-uniform over [1e-4, 1e5] (J^7 = 1e35 and bulk J^-7 = 4e32 stay inside the float32 range: the
    model has no clamp)"""
    g = np.random.Generator(np.random.PCG64(seed + 77))
    J = np.concatenate([1 + 0.05 * g.standard_normal(n // 2), 10 ** g.uniform(-4, 5, n - n // 2)])
    return J.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the models in principal space
INF = np.inf


def _sign_q(s):
    """math::svd puts the sign on the smallest singular value; for an inverted F with |s1| ~ |s2| the other placement is as good a
    decomposition and gives another polar rotation: a branch of the SVD itself"""
    return np.abs(s[:, 1]) + np.minimum(s[:, 2], 0.0)


def _fc(m, s, lj):
    J = s.prod(1)
    P = 2 * m.mu * (s - 1) + (m.lam * (J - 1))[:, None] * np.stack([s[:, 1] * s[:, 2], s[:, 0] * s[:, 2], s[:, 0] * s[:, 1]], 1)
    return dict(k=P * s * m.volume, s=s.copy(), lj=lj.copy(), label=np.full(len(s), "elastic", object), q={"sign": _sign_q(s)},
                clamp=np.full(len(s), INF))


def _sand(m, s, lj):
    n = len(s)
    a = np.maximum(np.abs(s), 1e-4)
    eps = np.log(a) - m.cohesion
    sum_eps = eps.sum(1)
    tr = sum_eps + lj
    eh = eps - tr[:, None] / 3
    ehn = np.sqrt((eh ** 2).sum(1))
    dg = ehn + m.dp_coef * tr * m.yield_surface
    tip = tr >= 0
    inside = ~tip & (dg <= 0)
    H = np.where(tip[:, None], m.cohesion, np.where(inside[:, None], eps + m.cohesion, eps - (dg / ehn)[:, None] * eh + m.cohesion))
    ljn = np.where(tip, (m.beta * sum_eps + lj) if m.vol_correction else lj, 0.0)
    label = np.where(tip, "II", np.where(inside, "I", "III")).astype(object)
    k = (2 * m.mu * H + m.lam * H.sum(1, keepdims=True)) * m.volume
    sn = np.exp(H)
    if m.mu == 0:   # the reference's corner: F is not projected, New_S = 0, P = U diag(-inf / 0) V^T.  Labelled, not valued.
        c = ~tip
        label[c] = "non-finite"
        k[c], sn[c], ljn[c] = np.nan, s[c], lj[c]
    return dict(k=k, s=sn, lj=ljn, label=label, q={"tr": tr, "dg": np.where(tip | (m.mu == 0), INF, dg), "sign": _sign_q(s)},
                clamp=(np.abs(s) - 1e-4).min(1))


def _vm(m, s, lj):
    Sc = np.maximum(s, 1e-4)
    J = Sc.prod(1)
    tau = 2 * m.mu * (Sc - 1) * Sc + (m.lam * (J - 1) * J)[:, None]
    tr = tau.sum(1)
    st = tau - tr[:, None] / 3
    s_norm = np.sqrt((st ** 2).sum(1))
    tauy = np.sqrt(2.0 / 3.0) * m.yield_stress
    yq = s_norm - tauy
    yields = yq > 0
    tau_new = (tauy / s_norm)[:, None] * st + tr[:, None] / 3
    disc = m.mu * m.mu + 2 * m.mu * tau_new
    Sn = np.where(yields[:, None], (m.mu + np.sqrt(disc)) / (2 * m.mu), s)
    J = Sn.prod(1)
    P = 2 * m.mu * (Sn - 1) + (m.lam * (J - 1))[:, None] * np.stack([Sn[:, 1] * Sn[:, 2], Sn[:, 0] * Sn[:, 2], Sn[:, 0] * Sn[:, 1]], 1)
    bad = yields & (disc < 0).any(1)
    label = np.where(bad, "non-finite", np.where(yields, "yield", "elastic")).astype(object)
    return dict(k=P * Sn * m.volume, s=Sn, lj=lj.copy(), label=label,
                q={"yield": yq, "disc": np.where(yields, disc.min(1), INF), "sign": _sign_q(s)}, clamp=(s - 1e-4).min(1))


def _nacc(m, s, lj):
    bm, beta, Msqr, mu = m.bm, m.beta, m.Msqr, m.mu
    p0 = bm * (1e-5 + np.sinh(m.xi * np.maximum(-lj, 0)))
    p_min = -beta * p0
    Je = s.prod(1)
    Bh = s * s
    trB = Bh.sum(1) / 3
    Jm = mu * Je ** (-2.0 / 3.0)
    sh = Jm[:, None] * (Bh - trB[:, None])
    p_trial = -(bm * 0.5 * (Je - 1 / Je)) * Je
    ys = 1.5 * (1 + 2 * beta)
    yp = Msqr * (p_trial - p_min) * (p_trial - p0)
    sn = (sh ** 2).sum(1)
    y = ys * sn + yp
    c1 = p_trial > p0
    c2 = ~c1 & (p_trial < p_min)
    c3 = ~c1 & ~c2 & (y >= 1e-4)
    Je_tip = np.sqrt(-2 * np.where(c1, p0, p_min) / bm + 1)
    Bs = Je ** (2.0 / 3.0) / mu * np.sqrt(-yp / ys) / np.sqrt(sn)
    S3 = np.sqrt(sh * Bs[:, None] + trB[:, None])
    Sn = np.where((c1 | c2)[:, None], np.cbrt(Je_tip)[:, None], np.where(c3[:, None], S3, s))
    ljn = lj + np.where((c1 | c2) & m.hardening, np.log(Je / Je_tip), 0.0)
    guards = np.minimum(np.minimum(p0 - 1e-4, p0 - 1e-4 - p_trial), p_trial - 1e-4 - p_min)
    hard = c3 & m.hardening & (guards > 0)
    pc = (1 - beta) * p0 / 2
    q_trial = np.sqrt(1.5 * sn)
    d0, d1 = pc - p_trial, -q_trial
    dn = np.sqrt(d0 * d0 + d1 * d1)
    d0, d1 = d0 / dn, d1 / dn
    Cq = Msqr * (pc - p_min) * (pc - p0)
    Bq = Msqr * d0 * (2 * pc - p0 - p_min)
    Aq = Msqr * d0 * d0 + (1 + 2 * beta) * d1 * d1
    root = np.sqrt(Bq * Bq - 4 * Aq * Cq)
    p1, p2 = pc + (-Bq + root) / (2 * Aq) * d0, pc + (-Bq - root) / (2 * Aq) * d0
    pf = np.where((p_trial - pc) * (p1 - pc) > 0, p1, p2)
    Jf = np.sqrt(np.abs(-2 * pf / bm + 1))
    ljn = ljn + np.where(hard & (Jf > 1e-4), np.log(Je / Jf), 0.0)
    J = Sn.prod(1)
    B2 = Sn * Sn
    k = ((mu * J ** (-2.0 / 3.0))[:, None] * (B2 - B2.sum(1, keepdims=True) / 3) + (bm * 0.5 * (J * J - 1))[:, None]) * m.volume
    label = np.where(c1, "case1", np.where(c2, "case2", np.where(hard, "case3_hard", np.where(c3, "case3_nohard", "inside")))).astype(object)
    label[~(np.isfinite(k).all(1) & np.isfinite(ljn))] = "non-finite"
    window = ~c1 & ~c2
    q = {"p_hi": p_trial - p0, "p_lo": p_trial - p_min, "y": np.where(window, y - 1e-4, INF),
         "guard": np.where(c3 & m.hardening, guards, INF), "Jf": np.where(hard, Jf - 1e-4, INF), "Je": Je, "sign": _sign_q(s)}
    return dict(k=k, s=Sn, lj=ljn, label=label, q=q, clamp=np.full(len(s), INF))


_MODELS = {0: _fc, 1: _sand, 2: _vm, 3: _nacc}


def principal(m, s, lj):
    with np.errstate(all="ignore"):
        return _MODELS[m.model](m, np.asarray(s, np.float64), np.asarray(lj, np.float64))


def margins(m, s, lj, h):
    """first-order propagation of a singular-value error h [n] to every branch quantity: sum_i |dq/ds_i| h by central differences.  A
    quantity that is not finite on one side of the difference gets an infinite margin."""
    out = None
    for i in range(3):
        e = np.zeros_like(s)
        e[:, i] = h
        qp, qm = principal(m, s + e, lj)["q"], principal(m, s - e, lj)["q"]
        with np.errstate(all="ignore"):
            d = {k: np.where(np.isinf(qp[k]) & np.isinf(qm[k]), 0.0, np.abs(qp[k] - qm[k]) / 2) for k in qp}
        for k in d:
            d[k] = np.where(np.isnan(d[k]), INF, d[k])
        out = d if out is None else {k: out[k] + d[k] for k in d}
    return out


class Ref:
    """float64 result of one (family, parameter set): PF, F (projected), lj [n, ...]; label; q, margin per branch quantity; scale,
    fscale, ljscale.  near_of[output] [n]: the samples left out of the value comparison of that output (see evaluate); near: their
    union; near_nf: near a boundary behind which the result is not finite; beyond: float64 intermediates outside the float32 range"""


def evaluate(pset, F, lj, s_err):
    """the reference of one parameter set on F [n, 9] float32, logJp [n] float32.  s_err: relative singular-value error (of ||F||_2)
    that the branch margins are built from (the family's measured value)."""
    m = material(pset)
    Um, s, Vm = svd64(F)
    lj = np.asarray(lj, np.float64)
    r = principal(m, s, lj)
    R = Ref()
    R.m, R.U, R.s, R.V = m, Um, s, Vm
    k = r["k"]
    PF = np.zeros((len(s), 3, 3))
    for a in range(3):          # the upper triangle, mirrored: the Kirchhoff stress of an isotropic model is exactly symmetric
        for b in range(a, 3):
            PF[:, a, b] = PF[:, b, a] = (Um[:, a, :] * k * Um[:, b, :]).sum(1)
    R.PF = _vec9(PF)
    R.F = _vec9(np.einsum("nik,nk,njk->nij", Um, r["s"], Vm))
    R.lj, R.label, R.q, R.clamp = r["lj"], r["label"], r["q"], r["clamp"]
    nrm = np.maximum(np.abs(s[:, 0]), FLT_MIN)
    R.norm = nrm
    R.margin = margins(m, s, lj, s_err * nrm)
    # Condition number of the polar rotation U V^T, which the projected F = U diag(s') V^T carries: a perturbation dF moves it by at
    # most 2 |dF| / (s1 + s2) (R.-C. Li, New perturbation bounds for the unitary polar factor, SIAM J. Matrix Anal. Appl. 16, 1995; s2
    # signed as here), so a relative difference d between two float32 SVDs arrives in the projected F multiplied by up to
    # 2 ||F|| / (s1 + s2): 1 for F near a rotation, 1e2 ... 1e4 on the wide family.
    with np.errstate(all="ignore"):
        gap12 = np.abs(s[:, 1]) + s[:, 2]
        R.ampF = np.where(gap12 > 0, np.maximum(1.0, 2 * nrm / gap12), INF)
    # Near a branch boundary: the float64 branch quantity is within MARGIN_FACTOR propagated singular-value errors of 0.  A float32
    # evaluation may take the other branch there, so every output is left out of the value comparison.
    near_q = {}
    for name, q in R.q.items():
        with np.errstate(all="ignore"):
            near_q[name] = np.abs(q) < MARGIN_FACTOR * R.margin[name]
    # the first Piola-Kirchhoff stress k / (s' vol) that the float32 code forms on the way to P F^T vol leaves the float32 range
    # (a factor 4 for the order of its summation): finite in float64, inf or NaN in float32
    with np.errstate(all="ignore"):
        R.beyond = np.nan_to_num(np.abs(k / (r["s"] * m.volume)), nan=0.0, posinf=0.0).max(1) > FLT_MAX / 4
    branch = R.beyond.copy()
    for name, v in near_q.items():
        if name != "sign":
            branch |= v
    # The SVD's own branch (`sign`): |s1| ~ |s2| with s2 <= 0, where the sign may sit on either and the polar rotation is not unique.
    # On inverted F its condition number ||F|| / (|s1| - |s2|) also turns the rounding of the SVD's intermediates (COND_ROUND = 16 u)
    # into a difference between two correct float32 implementations; near where that reaches COND_TOL = 1e-4.  This always leaves out
    # the projected F = U diag(s') V^T.  It leaves out P F^T vol = U diag(k) U^T only where F is inverted by more than the margin, so
    # that k1 != k2; with |s1|, |s2| both inside the margin of 0 (rank 1, tiny F) k1 = k2 and P F^T vol does not depend on the choice.
    rot = near_q["sign"] | ((s[:, 2] < 0) & (np.abs(R.q["sign"]) * COND_TOL < COND_ROUND * nrm))
    inverted = s[:, 2] < -MARGIN_FACTOR * s_err * nrm
    R.near_of = dict(PF=branch | (rot & inverted), F=branch | rot, lj=branch)
    R.near = R.near_of["F"]
    nf = R.beyond.copy()
    for name in NONFINITE_Q + (("tr",) if m.model == 1 and m.mu == 0 else ()):
        if name in near_q:
            nf |= near_q[name]
    R.near_nf = nf
    Fm = np.asarray(F, np.float64)
    J2 = s.prod(1) ** 2 if m.model in (0, 2) else 0.0
    amb = np.maximum(np.maximum(1.0, np.abs(Fm - np.eye(3).reshape(1, 9)).max(1)), J2)
    with np.errstate(all="ignore"):
        R.scale = np.fmax(np.fmax(np.abs(np.where(np.isfinite(R.PF), R.PF, 0)).max(1), m.modulus * m.volume * amb), FLT_MIN)
        R.fscale = np.maximum(np.maximum(np.abs(Fm).max(1), np.abs(np.where(np.isfinite(R.F), R.F, 0)).max(1)), FLT_MIN)
        R.ljscale = np.maximum(1.0, np.abs(np.where(np.isfinite(R.lj), R.lj, 0)))
    return R


# ------------------------------------------------------------------------------------------------ the checker
def ceiling(measured, floor=None):
    """2 x the oracle's measured error, and never below a rounding floor.  Where the oracle's error is rounding and not truncation
    (F = I, diagonal F, the rotations), twice its value does not bound another correct implementation: the roundings of two
    implementations are independent, and on diagonal F the oracle is exact by coincidence (IEEE a / sqrt(a a) = 1, where the kernel's
    a * rsq(a a) is 1 ulp off).  FLOOR_SVD = 16 u for S and the reconstruction (a singular value is the end of a chain of a few dozen
    operations that mostly cancel); FLOOR_STRESS = 256 u for P F^T vol, the projected F and logJp: a 1-ulp change of S passes through
    the model's conditioning (the von Mises root near a vanishing discriminant, the NACC hardening quadratic: up to 1e2).  Both lie
    below every ceiling that the truncation error sets (>= 1e-5) and far below what a lost sweep or a wrong branch costs (>= 1e-3)."""
    return max(CEIL_FACTOR * measured, FLOOR_SVD if floor is None else floor)


def svd_errors(F, Uv, S, Vv):
    """errors of a float32 SVD (U, V as column-major 9-vectors, S [n, 3]) of F against svd64, relative to ||F||_2, per sample"""
    Um, Vm, S = _mat(Uv), _mat(Vv), np.asarray(S, np.float64)
    _, s, _ = svd64(F)
    nrm = np.maximum(np.abs(s[:, 0]), FLT_MIN)
    eye = np.eye(3)
    rec = np.einsum("nik,nk,njk->nij", Um, S, Vm) - _mat(F)
    aS = np.abs(S)
    return dict(S=np.abs(S - s).max(1) / nrm, recon=np.abs(rec).max((1, 2)) / nrm,
                order=np.maximum(aS[:, 1] - aS[:, 0], aS[:, 2] - aS[:, 1]) / nrm,
                ortho=np.maximum(np.abs(np.einsum("nki,nkj->nij", Um, Um) - eye).max((1, 2)), np.abs(np.einsum("nki,nkj->nij", Vm, Vm) - eye).max((1, 2))),
                det=np.minimum(np.linalg.det(Um), np.linalg.det(Vm)), finite=np.isfinite(Um).all((1, 2)) & np.isfinite(Vm).all((1, 2)) & np.isfinite(S).all(1))


def check_svd(family, F, Uv, S, Vv, ceil=None, what="svd"):
    """the invariants that hold at any accuracy, and the family's ceilings (MEASURED_SVD unless `ceil` = (S, recon) is given).  Returns
    the worst S, reconstruction, ordering and orthonormality errors."""
    e = svd_errors(F, Uv, S, Vv)
    cS, cR = ceil if ceil is not None else (ceiling(MEASURED_SVD[family][0]), ceiling(MEASURED_SVD[family][1]))
    assert e["finite"].all(), "%s %s: non-finite output" % (what, family)
    assert e["ortho"].max() <= 1e-5, "%s %s: orthonormality %.3g" % (what, family, e["ortho"].max())
    assert (e["det"] > 0).all(), "%s %s: det U or det V <= 0" % (what, family)
    # ordering up to the measured S error: a pair out of order by d has one member at least d / 2 from the ordered truth
    assert (e["order"] <= 2 * e["S"] + 4 * U32).all(), "%s %s: |S| not ordered by %.3g" % (what, family, e["order"].max())
    assert e["S"].max() <= cS, "%s %s: S error %.3g > %.3g" % (what, family, e["S"].max(), cS)
    assert e["recon"].max() <= cR, "%s %s: reconstruction error %.3g > %.3g" % (what, family, e["recon"].max(), cR)
    return dict(S=e["S"].max(), recon=e["recon"].max(), order=max(e["order"].max(), 0.0), ortho=e["ortho"].max())


def stress_errors(R, PF, Fp, lj):
    """per-sample relative errors of a float32 result against the reference R (NaN where either side is not finite), the finite
    patterns and the asymmetry of PF relative to the same scale"""
    PF, Fp, lj = np.asarray(PF, np.float64), np.asarray(Fp, np.float64), np.asarray(lj, np.float64)
    with np.errstate(all="ignore"):
        ePF = np.abs(PF - R.PF).max(1) / R.scale
        eF = np.abs(Fp - R.F).max(1) / R.fscale
        elj = np.abs(lj - R.lj) / R.ljscale
        asym = np.abs(PF[:, [1, 2, 5]] - PF[:, [3, 6, 7]]).max(1) / R.scale
    return dict(PF=ePF, F=eF, lj=elj, asym=asym, fin_PF=np.isfinite(PF).all(1), fin_F=np.isfinite(Fp).all(1), fin_lj=np.isfinite(lj))


def check_stress(family, pset, R, PF, Fp, lj, ceil=None, what="stress", per_sample=None):
    """Invariants and ceilings of one (family, parameter set), per output o in PF, F, logJp:
      - the share of samples near a branch boundary (R.near_of[o]) is at most EXCLUDED_CAP, except where CAP_EXEMPT names o
      - finite wherever the reference is finite and no boundary to a non-finite result is near (R.near_nf): every other sample, near a
        boundary or not; and the finite pattern equals the reference's on the samples that are not near
      - the error of the samples that are not near is under the ceiling (MEASURED_STRESS unless ceil = (PF, F, logJp) is given), and the
        asymmetry of PF under twice that of PF
      - per_sample = (PF, F, lj, tol), a second float32 result (the oracle's): on the samples that are not near, the same finite pattern
        and every output within tol of its scale.  Only on the pairs of ORACLE_OWN_ERROR, and only for P F^T vol, may a sample be
        further from the oracle, if it is no further from float64 than the oracle plus tol.  For the projected F the tolerance of a
        sample is tol * R.ampF, the condition number of the polar rotation from the float64 singular values (evaluate): tol is a
        tolerance on a relative difference of the two decompositions, and the rotation passes it on multiplied by up to
        2 ||F|| / (s1 + s2).  Measured on the MI355X (2026-10-18): at plain 1e-4 only von Mises (up to 4.3e-4, 23-29 of 2048 samples)
        and NACC (up to 1.8e-4, 1-4 samples) on the wide family miss it, at s1 + s2 = 0.01 ... 0.02 ||F|| (factor 1e2); every other
        pair, and P F^T vol and logJp everywhere, meet the plain 1e-4.
    Returns the worst errors, the excluded share (of any output) and the worst gaps to the second result."""
    e = stress_errors(R, PF, Fp, lj)
    tag = "%s %s %s" % (what, family, pset)
    out = dict(excluded=R.near.mean(), PF=np.nan, F=np.nan, lj=np.nan, asym=np.nan, gap=np.nan, gapF=np.nan, gaplj=np.nan)
    exempt = CAP_EXEMPT.get((family, pset), ())
    for o in _ALL:
        share = R.near_of[o].mean()
        assert o in exempt or share <= EXCLUDED_CAP, "%s: %.1f %% of the samples are near a branch boundary of %s" % (tag, 100 * share, o)
    ref_fin = dict(PF=np.isfinite(R.PF).all(1), F=np.isfinite(R.F).all(1), lj=np.isfinite(R.lj))
    for o in _ALL:
        must = ref_fin[o] & ~R.near_nf
        assert e["fin_" + o][must].all(), "%s: %s is not finite where the reference is, at %s" % (tag, o, np.flatnonzero(must & ~e["fin_" + o])[:5])
        use = ~R.near_of[o]
        # non-finite exactly where the reference says so (per output: NACC at J < 0 projects to a finite stress in cases 1 and 2 while
        # logJp takes the log of a negative number)
        assert np.array_equal(e["fin_" + o][use], ref_fin[o][use]), "%s: finite pattern of %s differs at %s" % (
            tag, o, np.flatnonzero(use & (e["fin_" + o] != ref_fin[o]))[:5])
    cP, cF, cL = ceil if ceil is not None else tuple(ceiling(v, FLOOR_STRESS) for v in MEASURED_STRESS[(family, pset)])
    for o, c, name in (("PF", cP, "PF"), ("F", cF, "projected F"), ("lj", cL, "logJp")):
        val = ~R.near_of[o] & ref_fin[o]
        if val.any():
            out[o] = e[o][val].max()
            assert out[o] <= c, "%s: %s error %.3g > %.3g at sample %d" % (tag, name, out[o], c, int(np.flatnonzero(val)[e[o][val].argmax()]))
    val = ~R.near_of["PF"] & ref_fin["PF"]
    if val.any():
        # the reference is exactly symmetric, so an asymmetry of PF is error: never more than twice the bound on one component
        out["asym"] = e["asym"][val].max()
        assert out["asym"] <= 2 * cP, "%s: PF asymmetry %.3g" % (tag, out["asym"])
    if per_sample is not None:
        out.update(_per_sample(tag, R, (PF, Fp, lj), per_sample, (family, pset) in ORACLE_OWN_ERROR))
    return out


def per_sample_gaps(R, got, other):
    """|got - other| of the three outputs relative to their scales, per sample (NaN where either side is not finite)"""
    sc = dict(PF=R.scale[:, None], F=R.fscale[:, None], lj=R.ljscale)
    out = {}
    for o, a, b in zip(_ALL, got, other):
        with np.errstate(all="ignore"):
            d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / sc[o]
        out[o] = d.max(1) if d.ndim == 2 else d
    return out


def _per_sample(tag, R, got, per_sample, own_error):
    """every sample that is not near a boundary against a second float32 result (the oracle's), output by output"""
    other, tol = per_sample[:3], per_sample[3]
    gaps = per_sample_gaps(R, got, other)
    res = {}
    for o, key, a, b in zip(_ALL, ("gap", "gapF", "gaplj"), got, other):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        fa, fb = (np.isfinite(a).all(1), np.isfinite(b).all(1)) if a.ndim == 2 else (np.isfinite(a), np.isfinite(b))
        sel = ~R.near_of[o]
        assert np.array_equal(fa[sel], fb[sel]), "%s: finite pattern of %s differs from the oracle's at %s" % (tag, o, np.flatnonzero(sel & (fa != fb))[:5])
        both = sel & fb
        if not both.any():
            res[key] = 0.0
            continue
        gap = np.where(both, gaps[o], 0.0)
        ok = gap <= (tol * R.ampF if o == "F" else tol)
        eg = eo = np.zeros(len(gap))
        if o == "PF" and own_error:
            with np.errstate(all="ignore"):
                ref_fin = np.isfinite(R.PF).all(1)
                eg = np.where(both & ref_fin, np.abs(a - R.PF).max(1) / R.scale, np.inf)
                eo = np.where(both & ref_fin, np.abs(b - R.PF).max(1) / R.scale, 0.0)
            ok = ok | (eg <= eo + tol)
        i = int(np.where(~ok, gap, -1).argmax())
        assert np.all(ok), "%s: |kernel - oracle| of %s = %.3g of the scale at sample %d, %d samples over %.3g (error against float64 %.3g, the oracle's %.3g)" % (
            tag, o, gap[i], i, int((~ok).sum()), tol, eg[i], eo[i])
        res[key] = gap.max()
    return res


def branch_shares(R):
    return {l: float((R.label == l).mean()) for l in np.unique(R.label)}


# every branch of every model; each must hold >= 2 % of some (family, parameter set)
BRANCHES = {0: ("elastic",), 1: ("I", "II", "III", "non-finite"), 2: ("elastic", "yield", "non-finite"),
            3: ("case1", "case2", "case3_hard", "case3_nohard", "inside", "non-finite")}


# ------------------------------------------------------------------------------------------------ float32 port with a sweep count
def svd3_f32(F, sweeps=4):
    """numpy float32 port of svd3 (mpm_math.hpp / oracle/mpm.c), vectorised, with the number of Jacobi sweeps as an argument: the
    negative control `three sweeps`.  Returns U, S, V as the C entry points do (column-major 9-vectors)."""
    f = np.float32
    A = np.asarray(F, f)
    n = len(A)
    col = lambda i: A[:, 3 * i:3 * i + 3]
    S = np.empty((n, 3, 3), f)
    for i in range(3):
        for j in range(3):
            ci, cj = col(i), col(j)
            S[:, i, j] = (ci[:, 0] * cj[:, 0] + ci[:, 1] * cj[:, 1]) + ci[:, 2] * cj[:, 2]
    q = np.zeros((n, 4), f)
    q[:, 0] = 1
    gam, cst, sst = f(5.8284273147583007813), f(0.9238795325112867), f(0.3826834323650898)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for (X, Y, Z) in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                sh = S[:, X, Y] * f(0.5)
                ch = S[:, X, X] - S[:, Y, Y]
                ok = sh * sh >= f(1e-20)
                sh = np.where(ok, sh, f(0))
                ch = np.where(ok, ch, f(1))
                sh2, ch2 = sh * sh, ch * ch
                w = f(1) / np.sqrt(sh2 + ch2)
                sh, ch = sh * w, ch * w
                fix = ch2 <= gam * sh2
                sh, ch = np.where(fix, sst, sh), np.where(fix, cst, ch)
                sh2, ch2 = sh * sh, ch * ch
                c, s = ch2 - sh2, f(2) * sh * ch
                sxx, sxy, syy, sxz, syz = S[:, X, X].copy(), S[:, X, Y].copy(), S[:, Y, Y].copy(), S[:, X, Z].copy(), S[:, Y, Z].copy()
                t1, t2 = c * sxx + s * sxy, c * sxy + s * syy
                t3, t4 = -s * sxx + c * sxy, -s * sxy + c * syy
                S[:, X, X] = c * t1 + s * t2
                S[:, X, Y] = S[:, Y, X] = c * t3 + s * t4
                S[:, Y, Y] = -s * t3 + c * t4
                S[:, X, Z] = S[:, Z, X] = c * sxz + s * syz
                S[:, Y, Z] = S[:, Z, Y] = -s * sxz + c * syz
                qw, qx, qy, qz = q[:, 0].copy(), q[:, 1 + X].copy(), q[:, 1 + Y].copy(), q[:, 1 + Z].copy()
                q[:, 0] = qw * ch - qz * sh
                q[:, 1 + X] = qx * ch + qy * sh
                q[:, 1 + Y] = qy * ch - qx * sh
                q[:, 1 + Z] = qz * ch + qw * sh
        nq = f(1) / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        w, x, y, z = q[:, 0] * nq, q[:, 1] * nq, q[:, 2] * nq, q[:, 3] * nq
        V = np.empty((n, 3, 3), f)
        one, two = f(1), f(2)
        V[:, 0, 0], V[:, 0, 1], V[:, 0, 2] = one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)
        V[:, 1, 0], V[:, 1, 1], V[:, 1, 2] = two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)
        V[:, 2, 0], V[:, 2, 1], V[:, 2, 2] = two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)
        B = np.empty((n, 3, 3), f)
        for r in range(3):
            for c in range(3):
                B[:, r, c] = (A[:, r] * V[:, 0, c] + A[:, r + 3] * V[:, 1, c]) + A[:, r + 6] * V[:, 2, c]
        rho = (B[:, 0, :] * B[:, 0, :] + B[:, 1, :] * B[:, 1, :]) + B[:, 2, :] * B[:, 2, :]
        for (a, b) in ((0, 1), (0, 2), (1, 2)):
            sw = rho[:, a] < rho[:, b]
            ra, rb = rho[:, a].copy(), rho[:, b].copy()
            rho[:, a], rho[:, b] = np.where(sw, rb, ra), np.where(sw, ra, rb)
            for M in (B, V):
                ma, mb = M[:, :, a].copy(), M[:, :, b].copy()
                M[:, :, a] = np.where(sw[:, None], mb, ma)
                M[:, :, b] = np.where(sw[:, None], -ma, mb)
        Um = np.zeros((n, 3, 3), f)
        Um[:, [0, 1, 2], [0, 1, 2]] = 1
        for (P, R) in ((0, 1), (0, 2), (1, 2)):
            a1, a2 = B[:, P, P], B[:, R, P]
            rh = np.sqrt(a1 * a1 + a2 * a2)
            ok = rh > f(1e-12)
            c, s = np.where(ok, a1 / rh, f(1)), np.where(ok, a2 / rh, f(0))
            bp, br = B[:, P, :].copy(), B[:, R, :].copy()
            B[:, P, :], B[:, R, :] = c[:, None] * bp + s[:, None] * br, -s[:, None] * bp + c[:, None] * br
            up, ur = Um[:, :, P].copy(), Um[:, :, R].copy()
            Um[:, :, P], Um[:, :, R] = c[:, None] * up + s[:, None] * ur, -s[:, None] * up + c[:, None] * ur
    Sg = np.stack([B[:, 0, 0], B[:, 1, 1], B[:, 2, 2]], 1)
    return _vec9(Um).astype(f), Sg.astype(f), _vec9(V).astype(f)


# ------------------------------------------------------------------------------------------------ measured accuracy of the oracle
# The error of oracle/mpm.c -- the same 4-sweep algorithm in float32 -- against this reference, as tests/test_stress_ref64_cpu.py prints
# it (`REF64 stress` lines; the worst of the three SEEDS, n = 2048 per family; 0 where no sample of the pair is compared).  The ceilings
# are CEIL_FACTOR times these and hold for the kernels too.  Where a ceiling of the projected F is wide (von Mises on `wide`: the
# yield projection divides by a vanishing deviator), what holds the kernel is the per-sample comparison with the oracle at 1e-4.
# BEGIN MEASURED
MEASURED_DATE = "2026-10-18"
MEASURED_SVD = {   # family: (max S error, max reconstruction error), of ||F||_2
    "benign": (7.86e-06, 0.000761),
    "rotation": (4.6e-07, 6.9e-07),
    "near_identity": (4.95e-07, 7.76e-07),
    "repeated": (4.44e-07, 8.2e-06),
    "nearly_repeated": (1.82e-06, 1.24e-05),
    "wide": (0.0008, 0.00501),
    "inverted": (1.83e-05, 0.00257),
    "rank2": (1.6e-05, 0.000954),
    "rank1": (3.57e-07, 1.65e-05),
    "scaled_up": (3e-05, 0.00172),
    "scaled_down": (6.65e-05, 0.00108),
    "identity": (0, 0),
    "zero": (0, 0),
    "diagonal": (0, 0),
    "tiny": (2, 0.99),
    "compressed": (1.93e-05, 0.00143),
}
MEASURED_STRESS = {   # (family, parameter set): (P F^T vol, projected F, logJp), of their scales
    ("benign", "fc"): (0.00032, 8.88e-15, 0),
    ("benign", "sand"): (0.000221, 0.000959, 7.56e-07),
    ("benign", "vm"): (9.85e-06, 0.000499, 0),
    ("benign", "nacc"): (1.11e-05, 0.000698, 8.07e-07),
    ("benign", "sand_coh"): (0.000221, 0.000959, 3.76e-07),
    ("benign", "sand_novc"): (0.000221, 0.000959, 0),
    ("benign", "sand_mu0"): (0, 0.000388, 7.56e-07),
    ("benign", "nacc_nohard"): (1.11e-05, 0.000698, 0),
    ("rotation", "fc"): (7.79e-07, 1.13e-14, 0),
    ("rotation", "sand"): (7.79e-07, 7.8e-07, 6.03e-07),
    ("rotation", "vm"): (7.79e-07, 1.13e-14, 0),
    ("rotation", "nacc"): (7.59e-07, 1.13e-14, 0),
    ("near_identity", "fc"): (7.12e-07, 9.93e-15, 0),
    ("near_identity", "sand"): (6.57e-07, 8.34e-07, 6.46e-07),
    ("near_identity", "vm"): (7.12e-07, 9.93e-15, 0),
    ("near_identity", "nacc"): (7.05e-07, 3e-07, 6.64e-07),
    ("near_identity", "sand_coh"): (1.81e-06, 1.04e-06, 3.08e-07),
    ("near_identity", "sand_novc"): (6.57e-07, 8.34e-07, 0),
    ("near_identity", "sand_mu0"): (0, 3.64e-07, 6.46e-07),
    ("near_identity", "nacc_nohard"): (7.05e-07, 3e-07, 0),
    ("repeated", "fc"): (4.16e-06, 1.39e-14, 0),
    ("repeated", "sand"): (1.03e-06, 9.53e-06, 7.44e-07),
    ("repeated", "vm"): (1.05e-05, 6.6e-06, 0),
    ("repeated", "nacc"): (1.14e-05, 3.66e-05, 9.67e-07),
    ("nearly_repeated", "fc"): (4.71e-06, 1.27e-14, 0),
    ("nearly_repeated", "sand"): (2.01e-06, 1.4e-05, 9.03e-07),
    ("nearly_repeated", "vm"): (1.05e-05, 1.11e-05, 0),
    ("nearly_repeated", "nacc"): (1.89e-06, 1.14e-05, 9.42e-07),
    ("wide", "fc"): (0.00342, 1.37e-14, 0),
    ("wide", "sand"): (0.00375, 0.0108, 0),
    ("wide", "vm"): (0.00158, 0.238, 0),
    ("wide", "nacc"): (4.25e-07, 0.145, 1.47e-06),
    ("inverted", "fc"): (0.00827, 9.58e-15, 0),
    ("inverted", "sand"): (0.000404, 0.0273, 7.8e-07),
    ("inverted", "vm"): (4.63e-05, 0.0392, 0),
    ("inverted", "nacc"): (2.19e-07, 0.0385, 0),
    ("rank2", "fc"): (0.00132, 9.58e-15, 0),
    ("rank2", "sand"): (0.00348, 0.00128, 0),
    ("rank2", "vm"): (1.9e-05, 0.00185, 0),
    ("rank2", "nacc"): (0, 0, 0),
    ("rank1", "fc"): (5.5e-06, 0, 0),
    ("rank1", "sand"): (0.00378, 0, 0),
    ("rank1", "vm"): (1.34e-06, 0, 0),
    ("rank1", "nacc"): (0, 0, 0),
    ("scaled_up", "fc"): (0.00304, 9.5e-15, 0),
    ("scaled_up", "sand"): (0, 1.91e-06, 1.45e-07),
    ("scaled_up", "vm"): (0, 0, 0),
    ("scaled_up", "nacc"): (5.48e-10, 1.98e-06, 1.11e-07),
    ("scaled_down", "fc"): (2.63e-07, 9.93e-15, 0),
    ("scaled_down", "sand"): (2.96e-05, 0.00175, 0),
    ("scaled_down", "vm"): (2.63e-07, 9.93e-15, 0),
    ("scaled_down", "nacc"): (1.46e-05, 0.0014, 3.99e-06),
    ("identity", "fc"): (0, 0, 0),
    ("identity", "sand"): (0, 0, 0),
    ("identity", "vm"): (0, 0, 0),
    ("identity", "nacc"): (0, 0, 0),
    ("zero", "fc"): (0, 0, 0),
    ("zero", "sand"): (4.18e-08, 9.8e-08, 0),
    ("zero", "vm"): (0, 0, 0),
    ("zero", "nacc"): (0, 0, 0),
    ("diagonal", "fc"): (1.22e-07, 0, 0),
    ("diagonal", "sand"): (2.55e-07, 9.71e-08, 9.05e-08),
    ("diagonal", "vm"): (1.42e-06, 8.36e-07, 0),
    ("diagonal", "nacc"): (4.93e-06, 1.29e-05, 2.5e-07),
    ("tiny", "fc"): (1.4e-11, 0, 0),
    ("tiny", "sand"): (4.76e-07, 0, 0),
    ("tiny", "vm"): (1.4e-11, 0, 0),
    ("tiny", "nacc"): (0, 0, 0),
    ("compressed", "fc"): (0.000638, 8.51e-15, 0),
    ("compressed", "sand"): (0.000342, 0.00156, 5.35e-07),
    ("compressed", "vm"): (7.75e-06, 6.99e-05, 0),
    ("compressed", "nacc"): (7.33e-05, 0.00106, 7.62e-07),
    ("compressed", "sand_coh"): (0.000342, 0.00156, 1.93e-07),
    ("compressed", "sand_novc"): (0.000342, 0.00156, 0),
    ("compressed", "sand_mu0"): (0, 5.62e-06, 5.35e-07),
    ("compressed", "nacc_nohard"): (7.33e-05, 0.00106, 0),
}
MEASURED_EOS = 0.0
# END MEASURED
