"""CPU tests of the mesh incremental potential's replay (tests/ref64_potential.py) and of include/zensim_rocm/potential_device.hpp on the
host:

1  in float64 on tiny2, sheets5, fan and stack the gradient agrees with the central difference of the energy along random directions, for
   every subset of terms and with fixed vertices.  Step and bound are those of the barrier's own check (tests/test_barrier_cpu.py): h = 1e-7
   and 1e-5 of the largest gradient entry per coordinate, so 1e-5 max|g| |r|_1 along a direction r;
2  the float32 replay follows the float64 one, gradient=False gives the energies of gradient=True, and fixed vertices have no inertia
   energy and a zero gradient row;
3  the line-search cases the GPU test relies on, in the float64 replay on `sheets` along multiples of the float64 PCG direction
   (ref64_potential.SEARCH_CASES), and a NaN in the target;
4  the header compiled with g++ under the address and undefined-behaviour sanitizers gives the bytes of the float32 replay for the inertia
   and gradient epilogue, the trial positions and the decisions, on random inputs and on the edge cases (fixed vertices, an infinite energy,
   equality in the Armijo test).
"""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import ref64_potential as rq
import ref64_solve as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = ("elastic", "barrier", "friction")


@functools.lru_cache(maxsize=None)
def _potential(name, terms=TERMS, dtype=np.float64, fixed=False):
    S = rs.cpu_system(name, dtype, terms)
    v, t, _ = rs.scene(name)
    if fixed:
        S.fixed = np.zeros(S.nv, np.uint8)
        S.fixed[::3] = 1
    x, target, start = rq.step_arrays(v, t)
    return rq.Potential(S, target, start), x


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", ("tiny2", "sheets5", "fan", "stack"))
def test_the_gradient_against_central_differences_for_every_subset_of_terms(name):
    h = 1e-7
    g = np.random.default_rng(31)
    worst = 0.0
    for n in range(4):
        for terms in itertools.combinations(TERMS, n):
            for fixed in (False, True):
                P, x = _potential(name, terms, np.float64, fixed)
                x = x.astype(np.float64)
                v = P.evaluate(x)
                assert np.isfinite(v["energy"]) and not v["grad"][P.fx].any()
                scale = np.abs(v["grad"]).max()
                for _ in range(3):
                    r = np.where(P.fx[:, None], 0.0, g.standard_normal(x.shape))
                    fd = (P.evaluate(x + h * r, grad=False)["energy"] - P.evaluate(x - h * r, grad=False)["energy"]) / (2 * h)
                    err = abs(fd - (v["grad"] * r).sum())
                    worst = max(worst, err / (scale * np.abs(r).sum()))
                    assert err <= 1e-5 * scale * np.abs(r).sum(), (terms, fixed, err, scale)
    print("POTENTIAL differences[%s]: closed form - central difference at most %.2e of max|g| |r|_1" % (name, worst))


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", ("tiny2", "sheets5"))
def test_the_float32_replay_follows_the_float64_one(name):
    for fixed in (False, True):
        P64, x = _potential(name, TERMS, np.float64, fixed)
        P32, _ = _potential(name, TERMS, np.float32, fixed)
        a, b = P64.evaluate(x), P32.evaluate(x)
        assert b["grad"].dtype == np.float32 and abs(b["energy"] - a["energy"]) <= 1e-4 * abs(a["energy"])
        assert np.abs(b["grad"] - a["grad"]).max() <= 1e-3 * np.abs(a["grad"]).max()
        e = P32.evaluate(x, grad=False)
        assert e["grad"] is None and np.array_equal(e["parts"], b["parts"]) and e["energy"] == b["energy"]
        assert b["energy"] == b["parts"][0] + np.float64(np.float32(rs.SCALE)) * ((b["parts"][1] + b["parts"][2]) + b["parts"][3])
        if fixed:
            assert not b["grad"][::3].any() and b["grad"][1::3].any()
            free, _ = _potential(name, TERMS, np.float32, False)
            assert b["parts"][0] < free.evaluate(x)["parts"][0]


# ------------------------------------------------------------------------------------------------ 3
def test_the_line_search_cases_on_sheets():
    P, x = _potential("sheets")
    x = x.astype(np.float64)
    S = P.S
    v = P.evaluate(x)
    S.linearize(x, x - P.start)
    d = rs.pcg(S.multiply, S.blocks()["inverse"], -v["grad"], None, 400, rel_tol=1e-3, dtype=np.float64)
    assert d["flag"] == "converged"
    for name, (mult, kw, flag, trials) in rq.SEARCH_CASES.items():
        r = P.line_search(x, mult * d["x"], 1.0, **kw)
        print("%s: flag %s after %d trials, t = %g, energies %s" % (name, r["flag"], r["trials"], r["t"], r["energies"]))
        assert (r["flag"], r["trials"]) == (flag, trials), name
        assert len(r["energies"]) == r["trials"] + 1 and r["energies"][0] == v["energy"]
        if flag == "accepted":
            assert r["energy"] == r["energies"][-1] < v["energy"] and r["t"] == 0.5 ** (trials - 1) and (r["energies"][1:-1] > v["energy"]).all()
            assert np.array_equal(r["x"], x + r["t"] * (mult * d["x"]))
        else:
            assert r["t"] == 0.0 and np.array_equal(r["x"], x) and r["energy"] == v["energy"]
    target = P.target.copy()
    target[5, 1] = np.nan
    r = rq.Potential(S, target, P.start).line_search(x, d["x"], 1.0)
    assert r["flag"] == "not_finite" and r["trials"] == 0 and len(r["energies"]) == 1
    for t_max in (0.0, -1.0, np.inf, np.nan):
        assert P.line_search(x, d["x"], t_max)["flag"] == "not_finite"


# ------------------------------------------------------------------------------------------------ 4
def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_potential")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_potential.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    f, n = np.float32, 20000
    g = np.random.default_rng(41)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype.itemsize == 4 else np.uint64)
    run = lambda *a: subprocess.run([exe] + [str(z) for z in a], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    clean = lambda r: r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    # vertices: x, target, p, start, acc (3 each), mass, scale, t, the fixed byte as a float
    x, target, p, start = (g.standard_normal((n, 3)).astype(f) for _ in range(4))
    acc = (10.0 ** g.uniform(-3, 3, (n, 1)) * g.standard_normal((n, 3))).astype(f)
    mass, scale, t = (10.0 ** g.uniform(-4, 2, n)).astype(f), (10.0 ** g.uniform(-4, 0, n)).astype(f), g.uniform(0, 1, n).astype(f)
    mass[:5] = (0, -1, np.nan, np.inf, 1)       # masses that are not finite and positive mark fixed vertices
    byte = np.zeros(n, f)
    byte[4:200:2] = 1
    p[10], acc[11] = np.nan, np.inf
    rows = np.concatenate([x, target, p, start, acc, mass[:, None], scale[:, None], t[:, None], byte[:, None]], axis=1).astype(f)
    fin, fout = str(tmp_path / "verts.bin"), str(tmp_path / "verts.out")
    rows.tofile(fin)
    r = run("vertices", fin, fout)
    assert clean(r), r.stderr
    out = np.fromfile(fout, np.dtype([("e", f), ("g", f, 3), ("xk", f, 3), ("uk", f, 3), ("fixed", np.int32)]))
    assert len(out) == n
    fx = rs.fixed_mask(mass, byte)
    assert np.array_equal(out["fixed"], fx.astype(np.int32)) and fx[:4].all() and not fx[5] and fx[4]
    e, d = rq.inertia(x, target, mass, fx)
    with np.errstate(all="ignore"):
        want_g = np.where(fx[:, None], f(0), mass[:, None] * d + scale[:, None] * acc).astype(f)      # rq.gradient with one scale per row
        xk = np.where(fx[:, None], x, x + t[:, None] * p).astype(f)                                   # rq.trial with one t per row
    assert np.array_equal(bits(out["e"]), bits(e)) and np.array_equal(bits(out["g"]), bits(want_g))
    assert np.array_equal(bits(out["xk"]), bits(xk)) and np.array_equal(bits(out["uk"]), bits((xk - start).astype(f)))
    assert not out["e"][fx].any() and not out["g"][fx].any() and np.array_equal(out["xk"][fx], x[fx])
    # searches: records of 8 doubles = scale, tMax, c1, shrink, maxTrials, slope, the four parts of E_0; then maxTrials x 4 parts per trial
    max_trials = 6
    m = 4000
    slope = -10.0 ** g.uniform(-3, 2, m)
    parts = 10.0 ** g.uniform(-3, 2, (m, 1 + max_trials, 4))
    parts[:, 1:] *= 10.0 ** g.uniform(-0.5, 0.5, (m, max_trials, 1))
    sc, tm, c1, sh = (10.0 ** g.uniform(-3, 0, m)).astype(f), g.uniform(0.1, 1, m).astype(f), (10.0 ** g.uniform(-6, -1, m)).astype(f), g.uniform(0.1, 0.9, m).astype(f)
    slope[:4] = (0.0, 1.0, np.nan, -np.inf)                    # not_descent twice, not_finite twice
    tm[4:8] = (0.0, -1.0, np.inf, np.nan)                      # not_finite
    parts[8, 0, 0] = np.inf                                    # E_0 infinite: not_finite
    parts[9, 1, 2], parts[9, 2:] = np.inf, parts[9, :1] * 0.5  # the barrier's +inf rejects the first trial, the second is accepted
    parts[10, 1:, 1] = np.nan                                  # every trial NaN: max_trials
    # equality in the Armijo test: E_1 = E_0 + c1 t slope exactly in float64 (powers of two)
    parts[11, 0], parts[11, 1], sc[11], tm[11], c1[11], slope[11] = (4.0, 0, 0, 0), (3.5, 0, 0, 0), 1.0, 1.0, 0.25, -2.0
    parts[12] = parts[11]
    parts[12, 1, 0], sc[12], tm[12], c1[12], slope[12] = np.nextafter(3.5, 4.0), 1.0, 1.0, 0.25, -2.0      # one ulp above: rejected
    head = np.stack([sc, tm, c1, sh, np.full(m, max_trials), slope], axis=1).astype(np.float64)
    recs = np.concatenate([head, parts.reshape(m, -1)], axis=1)
    fin, fout = str(tmp_path / "search.bin"), str(tmp_path / "search.out")
    recs.tofile(fin)
    r = run("searches", fin, fout, max_trials)
    assert clean(r), r.stderr
    out = np.fromfile(fout, np.dtype([("trials", np.int32), ("flag", np.int32), ("t", f), ("next", f), ("energy", np.float64), ("slope", np.float64),
                                      ("history", np.float64, max_trials + 1)]))
    assert len(out) == m
    flags = []
    for i in range(m):
        energies = [rq.compose(parts[i, k], sc[i]) for k in range(1 + max_trials)]
        calls = iter(energies[1:])
        w = rq.search(lambda xk, uk: next(calls), np.zeros((1, 3), f), np.zeros((1, 3), f), energies[0], slope[i], tm[i], np.zeros(1, bool), None,
                      c1[i], sh[i], max_trials)
        flags.append(w["flag"])
        got = out[i]
        assert rq.FLAGS[got["flag"]] == w["flag"] and got["trials"] == w["trials"], i
        assert np.array_equal(bits(got["history"][:w["trials"] + 1]), bits(w["energies"])), i
        assert bits(f(got["t"])) == bits(f(w["t"])) and bits(np.float64(got["energy"])) == bits(np.float64(w["energy"])), i
    assert flags[:4] == ["not_descent", "not_descent", "not_finite", "not_finite"] and flags[4:9] == ["not_finite"] * 5
    assert (flags[9], out["trials"][9]) == ("accepted", 2) and flags[10] == "max_trials"
    assert (flags[11], out["trials"][11]) == ("accepted", 1) and (flags[12], out["trials"][12] > 1) == (flags[12], True)
    assert {"accepted", "max_trials"} <= set(flags[13:])
