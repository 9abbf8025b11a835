"""Mesh proximity pairs without a GPU (tests/ref64_proximity.py, include/zensim_rocm/distance_device.hpp ee_closest): the float64
segment-segment distance against closed forms, the float32 replay of the device chain against float64 on 10^6 pairs down to angles of
1e-7 rad (the evidence for the bound's constant), the header itself compiled for the host under the sanitizers, and the edge list.
Prints one `PROX <what> ...` line per check."""
import os
import subprocess

import numpy as np

import ref64_mesh as rm
import ref64_proximity as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = rp.U


def _one(a0, a1, b0, b1):
    d2, s, t, cat, _ = rp.ee_closest(*(np.array([x], np.float64) for x in (a0, a1, b0, b1)))
    return float(np.sqrt(d2[0])), float(s[0]), float(t[0]), int(cat[0])


def test_ee_closest_float64_against_closed_forms():
    h = 0.037
    # perpendicular crossing segments at height h: interior - interior, the distance is the height
    d, s, t, cat = _one((-1, 0, 0), (1, 0, 0), (0.2, -1, h), (0.2, 3, h))
    assert cat == 8 and abs(d - h) < 1e-15 and abs(s - 0.6) < 1e-15 and abs(t - 0.25) < 1e-15
    # collinear disjoint segments: the gap between the facing endpoints (a1 and b0)
    d, s, t, cat = _one((0, 0, 0), (1, 0, 0), (1.5, 0, 0), (4, 0, 0))
    assert cat == 1 * 3 + 0 and abs(d - 0.5) < 1e-15 and (s, t) == (1.0, 0.0)
    # ... and the other way round (a0 and b1)
    d, s, t, cat = _one((1.5, 0, 0), (4, 0, 0), (0, 0, 0), (1, 0, 0))
    assert cat == 0 * 3 + 1 and abs(d - 0.5) < 1e-15 and (s, t) == (0.0, 1.0)
    # a T: b ends 0.1 above the interior of a
    d, s, t, cat = _one((0, 0, 0), (2, 0, 0), (0.5, 0.1, 0), (0.5, 3, 0))
    assert cat == 2 * 3 + 0 and abs(d - 0.1) < 1e-15 and abs(s - 0.25) < 1e-15 and t == 0.0
    # a zero-length edge: the distance from the point to the other segment
    d, s, t, cat = _one((0.3, 0.4, 0), (0.3, 0.4, 0), (0, 0, 0), (1, 0, 0))
    assert abs(d - 0.4) < 1e-15 and cat == 0 * 3 + 2 and s == 0.0 and abs(t - 0.3) < 1e-15
    d, s, t, cat = _one((0, 0, 0), (1, 0, 0), (0.3, 0.4, 0), (0.3, 0.4, 0))
    assert abs(d - 0.4) < 1e-15 and cat == 2 * 3 + 0 and abs(s - 0.3) < 1e-15 and t == 0.0
    # parallel overlapping segments 0.2 apart: a boundary pair realises it
    d, s, t, cat = _one((0, 0, 0), (1, 0, 0), (0.5, 0.2, 0), (2, 0.2, 0))
    assert abs(d - 0.2) < 1e-15 and cat in (1 * 3 + 2, 2 * 3 + 0)


def seeded_pairs(n, seed):
    """n segment pairs in float32 inside [0.2, 0.8]^3: lengths 0.015 .. 0.075, separations up to 0.03, angles log-uniform in [1e-7, 1] rad.
    Half of them cross in projection (the minimiser is interior unless they are too parallel), the others are offset along the edge."""
    g = np.random.default_rng(seed)

    def unit(x):
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    e1 = unit(g.standard_normal((n, 3)))
    e2 = unit(np.cross(e1, g.standard_normal((n, 3))))
    e3 = np.cross(e1, e2)
    la, lb = g.uniform(0.015, 0.075, n), g.uniform(0.015, 0.075, n)
    ang = np.exp(g.uniform(np.log(1e-7), 0.0, n))
    sep = g.uniform(0.0, 0.03, n)
    dirb = np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2
    c = g.uniform(0.3, 0.7, (n, 3))                      # the crossing point of the projections
    fa, fb = g.uniform(-0.3, 1.3, n), g.uniform(-0.3, 1.3, n)
    half = g.random(n) < 0.5
    fa, fb = np.where(half, g.uniform(0.05, 0.95, n), fa), np.where(half, g.uniform(0.05, 0.95, n), fb)
    a0 = c - (fa * la)[:, None] * e1
    b0 = c - (fb * lb)[:, None] * dirb + sep[:, None] * e3
    return tuple(x.astype(np.float32) for x in (a0, a0 + la[:, None] * e1, b0, b0 + lb[:, None] * dirb))


def _bound(d, a0, a1, b0, b1):
    a0, a1, b0, b1 = (np.asarray(x, np.float64) for x in (a0, a1, b0, b1))
    S = d + np.linalg.norm(a1 - a0, axis=1) + np.linalg.norm(b1 - b0, axis=1)
    M = np.abs(np.stack([a0, a1, b0, b1])).max(axis=(0, 2))
    return rp.K_EE * U * (S + M) + 1e-37


def test_float32_replay_of_ee_closest_stays_within_the_bound():
    n = 1 << 20
    P = seeded_pairs(n, 11)
    d64, s64, t64, c64, _ = rp.ee_closest(*(x.astype(np.float64) for x in P))
    d64 = np.sqrt(d64)
    d2, s, t, cat, par = rp.ee_closest(*P, parallel=rp.PARALLEL32)
    assert d2.dtype == np.float32 and np.isfinite(d2).all()
    d32 = np.sqrt(d2.astype(np.float64))
    b = _bound(d64, *P)
    ratio = np.abs(d32 - d64) / b
    below = (d64 - d32) / b
    interior = c64 == 8
    print("PROX replay: %d pairs, %d interior in float64 (%d in float32), %d through the parallel test; worst |d32 - d64| %.3f of the bound "
          "(K = %g), worst below %.3f; categories agree on %.4f" % (n, interior.sum(), (cat == 8).sum(), par.sum(), ratio.max(), rp.K_EE,
                                                                      below.max(), (cat == c64).mean()))
    assert n >= 10 ** 6 and interior.sum() >= 10 ** 4
    assert (ratio <= 1).all()
    assert (below <= 1).all()


def _host_program(tmp):
    exe = os.path.join(tmp, "host_ee_closest")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_ee_closest.cpp"),
                           "-o", exe])
    return exe


def test_the_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = _host_program(str(tmp_path))
    n = 200000
    P = seeded_pairs(n, 12)
    # degenerate input next to the seeded pairs: zero-length edges, identical edges, exactly parallel ones
    z = np.float32
    extra = np.array([[[.3, .3, .3], [.3, .3, .3], [.4, .3, .3], [.5, .3, .3]], [[.3, .3, .3], [.3, .3, .3], [.3, .3, .3], [.3, .3, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.3, .3, .3], [.4, .3, .3]], [[.3, .3, .3], [.4, .3, .3], [.35, .32, .3], [.45, .32, .3]],
                      [[.3, .3, .3], [.4, .3, .3], [.6, .3, .3], [.5, .3, .3]]], z)
    P = tuple(np.concatenate([x, extra[:, k]]) for k, x in enumerate(P))
    n = len(P[0])
    fin, fout = str(tmp_path / "pairs.bin"), str(tmp_path / "out.bin")
    np.stack(P, axis=1).astype(np.float32).tofile(fin)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    rec = np.fromfile(fout, np.dtype([("d2", np.float32), ("s", np.float32), ("t", np.float32), ("cat", np.int32)]))
    assert len(rec) == n
    d2, s, t, cat = rec["d2"], rec["s"], rec["t"], rec["cat"]
    # the numpy replay is the same chain: bit for bit
    r2, rs, rt, rc, _ = rp.ee_closest(*P, parallel=rp.PARALLEL32)
    assert np.array_equal(d2.view(np.uint32), r2.view(np.uint32)) and np.array_equal(cat, rc)
    assert np.array_equal(s.view(np.uint32), rs.astype(np.float32).view(np.uint32)) and np.array_equal(t.view(np.uint32), rt.astype(np.float32).view(np.uint32))
    P64 = tuple(x.astype(np.float64) for x in P)
    d64 = np.sqrt(rp.ee_closest(*P64)[0])
    b = _bound(d64, *P)
    d32 = np.sqrt(d2.astype(np.float64))
    assert np.isfinite(d2).all() and (np.abs(d32 - d64) <= b).all()
    # the category says where (s, t) lies
    u_c, v_c = cat // 3, cat % 3
    assert (cat >= 0).all() and (cat < 9).all()
    assert np.array_equal(u_c == 0, s == 0) and np.array_equal(u_c == 1, s == 1) and np.array_equal(v_c == 0, t == 0) and np.array_equal(v_c == 1, t == 1)
    assert ((s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)).all()
    # the point pair at (s, t), evaluated in float64, is that far apart
    a0, a1, b0, b1 = P64
    q = (a0 + s[:, None].astype(np.float64) * (a1 - a0)) - (b0 + t[:, None].astype(np.float64) * (b1 - b0))
    dq = np.linalg.norm(q, axis=1)
    print("PROX host: %d pairs, categories %s, |d32 - d64| %.3f of the bound, point pair %.3f" %
          (n, np.bincount(cat, minlength=9).tolist(), (np.abs(d32 - d64) / b).max(), (np.abs(dq - d32) / b).max()))
    assert (np.abs(dq - d32) <= b).all()
    assert (np.bincount(cat, minlength=9) > 0).all()


def test_edges_of_the_reference_equal_the_edge_set_of_mesh64():
    v, t = rm.icosphere(1)
    open_v, open_t = rp.grid_sheet(4, 0.5, 0.0, 0)
    rep_t = np.concatenate([t, t[3:4], t[3:4, [1, 2, 0]]])          # a triangle three times, once rotated
    for verts, tris in ((v, t), (open_v, open_t), (v, rep_t)):
        e = rp.edges(tris)
        want = set()
        for tri in np.asarray(tris).tolist():
            for k in range(3):
                a, b = tri[k], tri[(k + 1) % 3]
                want.add((min(a, b), max(a, b)))
        assert set(map(tuple, e.tolist())) == want and len(e) == len(want)
        assert (e[:, 0] < e[:, 1]).all()
        assert e.tolist() == sorted(e.tolist())
        m = rm.Mesh64(verts, tris)
        if tris is t:          # closed: every edge has two faces
            assert m.stats["boundary_edges"] == 0 and 2 * len(e) == 3 * len(tris)
        elif tris is open_t:   # a disk: Euler's formula
            assert m.stats["boundary_edges"] == 12 and len(verts) - len(e) + len(tris) == 1
        else:
            assert m.stats["nonmanifold_edges"] == 3 and len(e) == len(rp.edges(t))
    assert len(rp.edges(t)) == 30 * 4 and len(rp.edges(np.zeros((0, 3), np.int32))) == 0
    assert rp.edges(np.array([[2, 2, 5], [1, 1, 1]])).tolist() == [[2, 5]]
