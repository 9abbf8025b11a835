"""CPU tests of the mesh Newton system's replay (tests/ref64_solve.py) and of include/zensim_rocm/solve_device.hpp on the host:

1  the blocks built the device's way (every element's own corner blocks at unit directions, gathered in run order) equal, in float64, the
   diagonal blocks of the definition (component i at v of the term's product with e_{v,j}) on tiny2, fan, stack and sheets, and every
   block is symmetric positive semi-definite within float64 rounding;
2  the replay of the 3 x 3 inverse times the block is the identity within a bound from the block's condition number, and the fallback is
   taken by a singular block and by a negative diagonal;
3  on tiny2 and on two 5 x 5-vertex sheets 2 / 3 dhat apart the dense matrix (column by column) is symmetric positive definite and the
   float64 PCG reaches numpy.linalg.solve under the iteration limit, with the preconditioner in no more iterations than without;
4  the header compiled with g++ under the address and undefined-behaviour sanitizers gives the bytes of the float32 replay on random
   symmetric positive definite blocks and on the fallback cases.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import ref64_solve as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ITERS = 400


@functools.lru_cache(maxsize=None)
def _system(name):
    return rs.cpu_system(name)


def random_spd_blocks(n, seed, dtype=np.float32):
    """[n, 6] blocks Q diag(l) Q^T: sizes over six decades, condition numbers up to 100"""
    g = np.random.default_rng(seed)
    Q = np.linalg.qr(g.standard_normal((n, 3, 3)))[0]
    lam = 10.0 ** g.uniform(-3, 3, (n, 1)) * 10.0 ** g.uniform(-1, 1, (n, 3))
    M = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    return np.stack([M[:, i, j] for i, j in rs.SLOT], axis=1).astype(dtype)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", ("tiny2", "fan", "stack", "sheets"))
def test_blocks_equal_the_unit_direction_products_and_are_psd(name):
    S = _system(name)
    verts = range(S.nv) if S.nv <= 130 else np.unique(np.concatenate([np.arange(0, S.nv, 7), [0, S.nv - 1]]))
    mine = S.term_blocks()
    want = S.term_blocks_by_products(list(verts))
    for got, ref in zip(mine, want):
        size = np.abs(ref).max()
        assert size > 0
        # the same per-element numbers added in the same order: equal up to the rounding of the zeros that the other corners add
        assert np.abs(got[list(verts)] - ref).max() <= 1e-13 * size
    for blk in mine:
        M = rs.block_matrix(blk)
        assert np.array_equal(M, M.transpose(0, 2, 1))
        lo = np.linalg.eigvalsh(M)[:, 0]
        assert (lo >= -1e-12 * np.abs(M).max(axis=(1, 2))).all()


# ------------------------------------------------------------------------------------------------ 2
def test_the_inverse_within_the_condition_bound_and_the_fallbacks():
    D = random_spd_blocks(4000, 1)
    mass = np.ones(len(D), np.float32)
    inv, fb = rs.inverse(D, mass, np.float32)
    M, Mi = rs.block_matrix(D).astype(np.float64), rs.block_matrix(inv).astype(np.float64)
    cond = np.linalg.cond(M)
    # adjugate / determinant in float32, L the largest eigenvalue: an entry of the block carries u L (its own rounding), a cofactor is two
    # products of entries and a difference, 5 u L^2 absolute; one entry of (adjugate M) is three such terms times an entry, 15 u L^3, and
    # the determinant the same; over det >= L^3 / cond^2 that is 15 u cond^2 for the numerator and as much again, relative, for the
    # division by the rounded determinant: 32 u cond^2 with the six quotients' own roundings
    bound = 32 * 2.0 ** -24 * cond ** 2
    keep = ~fb
    assert keep.all() and bound.max() < 0.05
    err = np.abs(np.einsum("nij,njk->nik", Mi, M) - np.eye(3)).max(axis=(1, 2))
    assert (err[keep] <= bound[keep]).all(), (err[keep] / bound[keep]).max()
    # a singular block, a negative diagonal, an indefinite block with positive diagonal, an overflowing determinant
    bad = np.array([[1, 1, 1, 1, 1, 1], [-2, 0, 0, 3, 0, 4], [1, 2, 0, 1, 0, 1], [1e30, 0, 0, 1e30, 0, 1e30]], np.float32)
    m = np.array([2, 4, 8, 16], np.float32)
    inv, fb = rs.inverse(bad, m, np.float32)
    assert fb.all()
    assert np.array_equal(inv[0], np.array([1, 0, 0, 1, 0, 1], np.float32))
    assert np.array_equal(inv[1], np.array([0.25, 0, 0, np.float32(1) / np.float32(3), 0, 0.25], np.float32))
    assert np.array_equal(inv[2], np.array([1, 0, 0, 1, 0, 1], np.float32))
    assert np.array_equal(inv[3], np.full(6, 1e-30, np.float32) * np.array([1, 0, 0, 1, 0, 1], np.float32))
    # fixed vertices and masses that are not positive and finite get the zero block and are counted
    D = random_spd_blocks(6, 2)
    inv, nfb, nbad = rs.precondition(D, np.array([1, 0, -1, np.nan, np.inf, 1], np.float32), np.array([0, 0, 0, 0, 0, 1]), np.float32)
    assert nbad == 4 and nfb == 0 and not inv[1:].any() and inv[0].any()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", rs.SMALL)
def test_float64_pcg_reaches_the_dense_solve(name):
    S = _system(name)
    A = S.dense()
    assert np.abs(A - A.T).max() <= 1e-10 * np.abs(A).max()
    assert np.linalg.eigvalsh(0.5 * (A + A.T))[0] > 0
    B = S.blocks()
    assert B["fallbacks"] == 0 and B["fixed_masses"] == 0
    assert np.allclose(rs.block_matrix(B["combined"]), np.stack([A[3 * v:3 * v + 3, 3 * v:3 * v + 3] for v in range(S.nv)]), rtol=1e-12, atol=0)
    b = np.random.default_rng(9).standard_normal((S.nv, 3))
    want = np.linalg.solve(A, b.reshape(-1)).reshape(-1, 3)
    with_p = rs.pcg(S.multiply, B["inverse"], b, max_iters=MAX_ITERS, rel_tol=1e-10, dtype=np.float64)
    without = rs.pcg(S.multiply, None, b, max_iters=MAX_ITERS, rel_tol=1e-10, dtype=np.float64)
    for r in (with_p, without):
        assert r["flag"] == "converged" and r["iters"] < MAX_ITERS and len(r["residuals"]) == r["iters"] + 1
        assert np.abs(r["x"] - want).max() <= 1e-8 * np.abs(want).max()
    assert with_p["iters"] <= without["iters"]
    print("%s: %d iterations with the block-Jacobi preconditioner, %d without" % (name, with_p["iters"], without["iters"]))


def test_fixed_vertices_stay_and_the_float32_replay_follows_the_float64_one():
    S64, S32 = rs.cpu_system("tiny2", np.float64), rs.cpu_system("tiny2", np.float32)
    for S in (S64, S32):
        S.fixed = np.array([1, 0, 0, 0, 0, 0])
    x = np.random.default_rng(3).standard_normal((S64.nv, 3)).astype(np.float32)
    q64, q32 = S64.multiply(x), S32.multiply(x)
    assert not q64[0].any() and not q32[0].any()
    assert np.abs(q32 - q64).max() <= 1e-4 * np.abs(q64).max()
    b = np.random.default_rng(4).standard_normal((S64.nv, 3)).astype(np.float32)
    x0 = np.ones((S64.nv, 3), np.float32)
    r64 = rs.pcg(S64.multiply, S64.blocks()["inverse"], b, x0, 50, rel_tol=1e-4, dtype=np.float64)
    r32 = rs.pcg(S32.multiply, S32.blocks()["inverse"], b, x0, 50, rel_tol=1e-4, dtype=np.float32)
    assert r32["flag"] == r64["flag"] == "converged" and np.array_equal(r32["x"][0], x0[0])
    assert np.abs(r32["x"] - r64["x"]).max() <= 1e-3 * np.abs(r64["x"]).max()
    assert rs.pcg(S32.multiply, S32.blocks()["inverse"], b, x0, 0, dtype=np.float32)["flag"] == "max_iters"
    S32.scale = -S32.scale
    assert rs.pcg(S32.multiply, S32.blocks()["inverse"], b, None, 50, dtype=np.float32)["flag"] in ("breakdown", "not_finite")


# ------------------------------------------------------------------------------------------------ 4
def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "host_solve")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_solve.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    f = np.float32
    n = 20000
    g = np.random.default_rng(11)
    el, ba, fr = random_spd_blocks(n, 21), random_spd_blocks(n, 22), random_spd_blocks(n, 23)
    scale, mass = (10.0 ** g.uniform(-4, 0, n)).astype(f), (10.0 ** g.uniform(-4, 2, n)).astype(f)
    # the fallback cases: singular, negative diagonal, indefinite, a determinant beyond the float range, a negative scale
    el[:4], ba[:4], fr[:4], scale[:4], mass[:4] = 0, 0, 0, 1, 0.5
    el[0] = [0.5, 1, 1, 0.5, 1, 0.5]      # (all ones with the mass)
    el[1] = [-2, 0, 0, 3, 0, 4]
    el[2] = [1, 2, 0, 1, 0, 1]
    el[3] = [1e30, 0, 0, 1e30, 0, 1e30]
    scale[4:200] = -scale[4:200] * 1e3
    rows = np.concatenate([el, ba, fr, scale[:, None], mass[:, None]], axis=1).astype(f)
    fin, fout = str(tmp_path / "blocks.bin"), str(tmp_path / "blocks.out")
    rows.tofile(fin)
    r = subprocess.run([exe, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    out = np.fromfile(fout, np.dtype([("D", f, 6), ("inv", f, 6), ("z", f, 3), ("st", np.int32)]))
    assert len(out) == n
    with np.errstate(all="ignore"):
        D = scale[:, None] * ((el + ba) + fr)      # rs.combine with one scale per row
        for k in (0, 3, 5):
            D[:, k] = D[:, k] + mass
    inv, fb = rs.inverse(D, mass, f)
    z = rs.apply_block(inv, np.broadcast_to(np.array([1, -2, 3], f), (n, 3)))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(out["D"]), bits(D))
    assert np.array_equal(bits(out["inv"]), bits(inv))
    assert np.array_equal(bits(out["z"]), bits(z.astype(f)))
    assert np.array_equal(out["st"], fb.astype(np.int32))
    assert fb[:4].all() and fb[4:200].any() and not fb[200:].all()
