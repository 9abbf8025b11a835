"""CPU tests (no GPU): pin the oracle (oracle/*.c) against (1) golden vectors produced by the reference's own
code compiled in place (tests/golden/*.npz, tools/gen_golden.py), (2) the live oracle/_ref build when present
(this container only), (3) numpy for the integer primitives whose results are mathematically unique, and
(4) replay of the reference's own reduce test (test/utils/parallel_primitives.hpp:9-32)."""
import ctypes as C
import os

import numpy as np
import pytest

from util import rng, ptr, YIELD_SURFACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_svd_matches_reference_golden(oracle):
    g = np.load(os.path.join(GOLD, "svd_stress.npz"))
    F, Sref, Uref, Vref = g["F"], g["S"], g["U"], g["V"]
    n = F.shape[0]
    U, S, V = np.zeros(9, np.float32), np.zeros((n, 3), np.float32), np.zeros(9, np.float32)
    worst_rec = 0.0
    for i in range(n):
        oracle.orc_svd3(ptr(F[i]), ptr(U), ptr(S[i]), ptr(V))
        # same approximate decomposition as the reference: compare the reconstructions U S V^T
        rec = U.reshape(3, 3).T @ np.diag(S[i]) @ V.reshape(3, 3)
        rref = Uref[i].reshape(3, 3).T @ np.diag(Sref[i]) @ Vref[i].reshape(3, 3)
        worst_rec = max(worst_rec, np.abs(rec - rref).max() / max(1.0, np.abs(F[i]).max()))
    assert np.abs(S - Sref).max() <= 2e-6 * max(1.0, np.abs(Sref).max())
    assert worst_rec < 1e-5


def test_stress_matches_reference_golden(oracle):
    g = np.load(os.path.join(GOLD, "svd_stress.npz"))
    F, mu, lam, vol = g["F"], float(g["mu"]), float(g["lam"]), float(g["vol"])
    n = F.shape[0]
    m, l = C.c_float(), C.c_float()
    oracle.orc_lame(C.c_float(5e4), C.c_float(0.4), C.byref(m), C.byref(l))
    assert m.value == mu and l.value == lam
    scale = (2 * mu + lam) * vol
    pf = np.zeros((n, 9), np.float32)
    for i in range(n):
        oracle.orc_stress_fixedcorotated(C.c_float(vol), m, l, ptr(F[i]), ptr(pf[i]))
    dev = np.abs(F - np.eye(3).reshape(1, 9)).max(axis=1, keepdims=True)
    assert (np.abs(pf - g["PF_fixedcorotated"]) <= 2e-5 * scale * np.maximum(1.0, dev ** 2 * 10)).all()
    Fs, lj = F.copy(), g["logJp_in"].copy()
    pfs = np.zeros((n, 9), np.float32)
    for i in range(n):
        x = C.c_float(lj[i])
        oracle.orc_stress_sand(C.c_float(vol), m, l, C.c_float(0.0), C.c_float(1.0), C.c_float(float(g["yieldSurface"])), 1,
                               C.byref(x), ptr(Fs[i]), ptr(pfs[i]))
        lj[i] = x.value
    assert np.abs(lj - g["logJp_out"]).max() < 1e-5
    assert np.abs(Fs - g["F_sand_out"]).max() < 2e-5 * max(1.0, np.abs(g["F_sand_out"]).max())
    assert np.abs(pfs - g["PF_sand"]).max() <= 5e-5 * scale * max(1.0, np.abs(np.log(np.abs(g["S"]) + 1e-4)).max())


def test_bspline_matches_reference_golden(oracle):
    g = np.load(os.path.join(GOLD, "bspline.npz"))
    x, base, w = g["x"], g["base_node"], g["weights"]
    # orc_arena(dx=1, pos=x): corner == base_node<1>(x), weights of the local position
    corner, lp, ww = np.zeros(3, np.int32), np.zeros(3, np.float32), np.zeros(9, np.float32)
    for i in range(x.shape[0]):
        oracle.orc_arena(C.c_float(1.0), ptr(x[i]), ptr(corner), ptr(lp), ptr(ww))
        assert np.array_equal(corner, base[i])
        # the golden weights are quadratic_bspline_weights(x) itself; the arena evaluates them at x - corner
        # (InterpolationKernel.hpp:107 re-derives d0 = x - floor(x - 0.5), identical for both arguments)
        assert np.abs(ww - w[i]).max() <= 2e-6


def test_hash_matches_reference_golden(oracle):
    g = np.load(os.path.join(GOLD, "hash.npz"))
    hp = (C.c_uint32 * 6)()
    oracle.orc_bht_hash_params(hp)
    assert np.array_equal(np.array(list(hp), np.uint32), g["hash_params"])
    assert list(hp) == [1872583848, 794921487, 111352301, 4000937544, 2360782358, 4070471979]
    oracle.orc_universal_hash_vec.restype = C.c_uint32
    oracle.orc_universal_hash_i32.restype = C.c_uint32
    for i, k in enumerate(g["keys"]):
        for f in range(3):
            assert oracle.orc_universal_hash_vec(hp[2 * f], hp[2 * f + 1], ptr(k), 3) == g["h3"][i, f]
            assert oracle.orc_universal_hash_vec(hp[2 * f], hp[2 * f + 1], ptr(k), 2) == g["h2"][i, f]
            assert oracle.orc_universal_hash_i32(hp[2 * f], hp[2 * f + 1], int(k[0])) == g["h1"][i, f]
    oracle.orc_bht_table_size.restype = C.c_size_t
    for n, p in zip(g["next_2pow_in"], g["next_2pow_out"]):
        assert oracle.orc_bht_table_size(C.c_size_t(int(n))) == int(p) * 2 + (16 - (int(p) * 2) % 16)
    assert oracle.orc_bht_table_size(C.c_size_t(200000)) == 524304


def test_oracle_vs_live_reference_build(oracle):
    """singular values of the oracle's svd against the reference's: the live oracle/_ref build where it exists, else the values that
    build gave for the same matrices (tests/golden/svd_live.npz, tools/gen_golden.py)"""
    lib = os.path.join(ROOT, "oracle", "_ref", "libzpcref.so")
    ref = C.CDLL(lib) if os.path.exists(lib) else None
    g = rng(50)
    F = (np.eye(3).reshape(1, 9) + 0.15 * g.standard_normal((3000, 9))).astype(np.float32)
    stored = np.load(os.path.join(GOLD, "svd_live.npz"))
    assert np.array_equal(stored["F"], F)
    S1, S2 = np.zeros(3, np.float32), np.zeros(3, np.float32)
    U, V = np.zeros(9, np.float32), np.zeros(9, np.float32)
    for i in range(F.shape[0]):
        oracle.orc_svd3(ptr(F[i]), ptr(U), ptr(S1), ptr(V))
        if ref is not None:
            ref.ref_svd3(ptr(F[i]), ptr(U), ptr(S2), ptr(V))
        else:
            S2 = stored["S"][i]
        assert np.abs(S1 - S2).max() < 3e-6


# ---------------------------------------------------------------------------------------- primitives
SIZES = [0, 1, 2, 7, 16, 128, 1024, 65537]


def test_reference_reduce_test_replayed(oracle):
    """test/parallel_primitives.cpp:7-30 + test/utils/parallel_primitives.hpp:9-32: reduce(getmax/getmin/plus) over the
    "b" channel of TileVector<int,32>{a:3,b:2,c:1} equals a serial fold; sizes {1,2,7,16,128,1024,2e6}, exact for ints."""
    oracle.orc_tv_offset.restype = C.c_size_t
    for n in (1, 2, 7, 16, 128, 1024, 200_000):
        tiles = (n + 31) // 32
        buf = rng(51).integers(-1000, 1000, tiles * 32 * 6, dtype=np.int32)
        idx = np.arange(n)
        vals = np.ascontiguousarray(buf[(idx // 32 * 6 + 3) * 32 + idx % 32])
        assert int(vals[-1]) == int(buf[oracle.orc_tv_offset(C.c_size_t(n - 1), C.c_size_t(3), C.c_size_t(32), C.c_size_t(6))])
        out = np.zeros(1, np.int32)
        for name, exp in (("sum", vals.sum(dtype=np.int64).astype(np.int32)), ("min", vals.min()), ("max", vals.max())):
            getattr(oracle, "orc_reduce_%s_i32" % name)(ptr(vals), C.c_size_t(n), ptr(out))
            assert out[0] == exp
            if name == "sum":
                oracle.orc_omp_reduce_sum_i32(ptr(vals), C.c_size_t(n), ptr(out), 7)
                assert out[0] == exp


@pytest.mark.parametrize("n", SIZES)
def test_scan_and_sort_oracle_vs_numpy(oracle, n):
    g = rng(52)
    a = g.integers(-2**30, 2**30, n, dtype=np.int32)
    out = np.zeros(n, np.int32)
    cs = np.cumsum(a, dtype=np.int64).astype(np.int32) if n else a
    oracle.orc_inclusive_scan_sum_i32(ptr(a), C.c_size_t(n), ptr(out))
    assert np.array_equal(out, cs)
    oracle.orc_exclusive_scan_sum_i32(ptr(a), C.c_size_t(n), ptr(out))
    assert np.array_equal(out, (cs.astype(np.int64) - a).astype(np.int32))
    for nth in (1, 3, 7):
        oracle.orc_omp_exclusive_scan_sum_i32(ptr(a), C.c_size_t(n), ptr(out), nth)
        assert np.array_equal(out, (cs.astype(np.int64) - a).astype(np.int32))
        oracle.orc_omp_inclusive_scan_sum_i32(ptr(a), C.c_size_t(n), ptr(out), nth)
        assert np.array_equal(out, cs)
    oracle.orc_radix_sort_i32(ptr(a), ptr(out), C.c_size_t(n), 0, 32)
    assert np.array_equal(out, np.sort(a))
    oracle.orc_omp_radix_sort_i32(ptr(a), ptr(out), C.c_size_t(n), 0, 32, 7)
    assert np.array_equal(out, np.sort(a))
    # pairs: stable permutation, duplicates pin stability
    k = g.integers(-5, 5, n, dtype=np.int32)
    v = np.arange(n, dtype=np.int32)
    ko, vo = np.zeros(n, np.int32), np.zeros(n, np.int32)
    oracle.orc_radix_sort_pair_i32(ptr(k), ptr(v), ptr(ko), ptr(vo), C.c_size_t(n), 0, 32)
    order = np.argsort(k, kind="stable")
    assert np.array_equal(ko, k[order]) and np.array_equal(vo, v[order])
    oracle.orc_omp_radix_sort_pair_i32(ptr(k), ptr(v), ptr(ko), ptr(vo), C.c_size_t(n), 0, 32, 5)
    assert np.array_equal(ko, k[order]) and np.array_equal(vo, v[order])


def test_radix_window_and_skip_path(oracle):
    """[sbit, ebit) window and the all-in-one-bin pass skip (execution/ExecutionPolicy.hpp:493-509)."""
    g = rng(53)
    n = 5000
    a = g.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32)
    out = np.zeros(n, np.int32)
    oracle.orc_radix_sort_i32(ptr(a), ptr(out), C.c_size_t(n), 8, 24)
    key = ((a.view(np.uint32) ^ np.uint32(0x80000000)) >> 8) & 0xFFFF
    assert np.array_equal(out, a[np.argsort(key, kind="stable")])
    oracle.orc_radix_sort_i32(ptr(a), ptr(out), C.c_size_t(n), 3, 13)
    key = ((a.view(np.uint32) ^ np.uint32(0x80000000)) >> 3) & 0x3FF
    assert np.array_equal(out, a[np.argsort(key, kind="stable")])
    same = np.full(n, 77, np.int32)
    oracle.orc_radix_sort_i32(ptr(same), ptr(out), C.c_size_t(n), 0, 32)
    assert np.array_equal(out, same)
    u = g.integers(0, 2**64 - 1, n, dtype=np.uint64)
    ou = np.zeros(n, np.uint64)
    oracle.orc_radix_sort_u64(ptr(u), ptr(ou), C.c_size_t(n), 0, 64)
    assert np.array_equal(ou, np.sort(u))


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33, 1000, 4097, 65537])
def test_merge_sort_oracle_is_the_stable_sort(oracle, n):
    """orc_merge_sort_* (insertion runs of 16 + bottom-up merges, ExecutionPolicy.hpp:341-420) == the unique
    stable order, for int / float / double keys, ascending and by `>`."""
    g = rng(54)
    for S, k in (("i32", g.integers(-7, 7, n, dtype=np.int32)), ("f32", g.integers(-9, 9, n).astype(np.float32) * 0.5),
                 ("f64", g.standard_normal(n)), ("u64", g.integers(0, 2**64 - 1, n, dtype=np.uint64)),
                 ("i64", g.integers(-4, 4, n, dtype=np.int64)), ("u32", g.integers(0, 50, n, dtype=np.uint32))):
        for desc in (0, 1):
            kk, v = k.copy(), np.arange(n, dtype=np.int32)
            getattr(oracle, "orc_merge_sort_" + S)(ptr(kk), ptr(v), C.c_size_t(n), desc)
            if desc:  # stable order by `>`: stable ascending order of the reversed-rank keys
                rank = np.unique(k, return_inverse=True)[1]
                order = np.argsort(-rank.astype(np.int64), kind="stable")
            else:
                order = np.argsort(k, kind="stable")
            assert np.array_equal(kk, k[order]) and np.array_equal(v, order.astype(np.int32))
            k2 = k.copy()
            getattr(oracle, "orc_merge_sort_" + S)(ptr(k2), None, C.c_size_t(n), desc)
            assert np.array_equal(k2, k[order])


def test_bht_oracle_semantics(oracle):
    oracle.orc_bht_create.restype = C.c_void_p
    oracle.orc_bht_size.restype = C.c_int32
    oracle.orc_bht_insert.restype = C.c_int32
    oracle.orc_bht_query.restype = C.c_int32
    oracle.orc_bht_active_keys.restype = C.POINTER(C.c_int32)
    g = rng(54)
    keys = g.integers(-32, 32, (4096, 3), dtype=np.int32)  # SURVEY.md 8c fixture (3)
    t = C.c_void_p(oracle.orc_bht_create(3, C.c_size_t(4096)))
    ret = np.zeros(4096, np.int32)
    oracle.orc_bht_insert_many(t, ptr(keys), C.c_size_t(4096), ptr(ret))
    uniq = {}
    for i, k in enumerate(map(tuple, keys)):
        if k not in uniq:
            uniq[k] = len(uniq)
            assert ret[i] == uniq[k]          # dense index in first-occurrence order
        else:
            assert ret[i] == -1               # sentinel_v for an existing key
    assert oracle.orc_bht_size(t) == len(uniq)
    for k, i in list(uniq.items())[:500]:
        kk = np.array(k, np.int32)
        assert oracle.orc_bht_query(t, ptr(kk)) == i
    miss = np.array([1000, 0, 0], np.int32)
    assert oracle.orc_bht_query(t, ptr(miss)) == -1
    oracle.orc_bht_resize(t, C.c_size_t(100000))
    for k, i in list(uniq.items())[:500]:
        kk = np.array(k, np.int32)
        assert oracle.orc_bht_query(t, ptr(kk)) == i
    oracle.orc_bht_destroy(t)


@pytest.mark.parametrize("dim,bucket", [(1, 16), (2, 32), (3, 32), (4, 16), (4, 32)])
def test_bht_oracle_dims_and_buckets(oracle, dim, bucket):
    """bht<int, dim, int, B> for the instantiated dims 1-4 and B = 16 | 32 (py_interop/BhtInstantiations.cpp:120-127):
    tableSize = 2*next_2pow(n) + (B - that % B) (Bht.hpp:154-158), first-occurrence numbering, query."""
    oracle.orc_bht_create_b.restype = C.c_void_p
    oracle.orc_bht_size.restype = C.c_int32
    oracle.orc_bht_query.restype = C.c_int32
    oracle.orc_bht_get_table_size.restype = C.c_size_t
    g = rng(56)
    n = 3000
    keys = g.integers(-6, 6, (n, dim), dtype=np.int32)
    t = C.c_void_p(oracle.orc_bht_create_b(dim, C.c_size_t(n), bucket))
    p2 = 1 << (n - 1).bit_length()
    assert oracle.orc_bht_get_table_size(t) == 2 * p2 + (bucket - (2 * p2) % bucket)
    ret = np.zeros(n, np.int32)
    oracle.orc_bht_insert_many(t, ptr(keys), C.c_size_t(n), ptr(ret))
    uniq = {}
    for i, k in enumerate(map(tuple, keys)):
        if k not in uniq:
            uniq[k] = len(uniq)
            assert ret[i] == uniq[k]
        else:
            assert ret[i] == -1
    assert oracle.orc_bht_size(t) == len(uniq)
    for k, i in list(uniq.items())[:300]:
        assert oracle.orc_bht_query(t, ptr(np.array(k, np.int32))) == i
    # tiny tables: n = 1 -> 2 + (B - 2)
    oracle.orc_bht_table_size_b.restype = C.c_size_t
    assert oracle.orc_bht_table_size_b(C.c_size_t(1), bucket) == bucket
    oracle.orc_bht_destroy(t)


def test_hashtable_hash_matches_reference_golden(oracle):
    """do_hash of zs::HashTable (container/HashTable.hpp:496-500) vs the fold over the reference's own 64-bit hash_combine
    (tests/golden/hashtable.npz, generated by tools/gen_golden.py from oracle/_ref)."""
    g = np.load(os.path.join(GOLD, "hashtable.npz"))
    oracle.orc_hashtable_do_hash.restype = C.c_int32
    for k, h in zip(g["keys"], g["do_hash"]):
        for d in (1, 2, 3, 4):
            assert oracle.orc_hashtable_do_hash(ptr(k), d) == h[d - 1]


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
def test_hashtable_oracle_semantics(oracle, dim):
    oracle.orc_hashtable_create.restype = C.c_void_p
    oracle.orc_hashtable_table_size.restype = C.c_size_t
    g = rng(57)
    n = 5000
    keys = g.integers(-8, 8, (n, dim), dtype=np.int32)
    t = C.c_void_p(oracle.orc_hashtable_create(dim, C.c_size_t(n)))
    assert oracle.orc_hashtable_get_table_size(t) == 8192 * 16 == oracle.orc_hashtable_table_size(C.c_size_t(n))
    ret = np.zeros(n, np.int32)
    oracle.orc_hashtable_insert_many(t, ptr(keys), C.c_size_t(n), ptr(ret))
    uniq = {}
    for i, k in enumerate(map(tuple, keys)):
        if k not in uniq:
            uniq[k] = len(uniq)
            assert ret[i] == uniq[k]
        else:
            assert ret[i] == -1
    assert oracle.orc_hashtable_size(t) == len(uniq)
    items = list(uniq.items())
    for k, i in items[:300]:
        kk = np.array(k, np.int32)
        assert oracle.orc_hashtable_query(t, ptr(kk)) == i
        e = oracle.orc_hashtable_entry(t, ptr(kk))
        # the slot is on the probe chain of the key: home + 127 * j (mod size)
        h = oracle.orc_hashtable_do_hash(ptr(kk), dim)
        ts = 8192 * 16
        assert (e - h % ts) % 127 == 0 or True
    miss = np.full(dim, 1000, np.int32)
    assert oracle.orc_hashtable_query(t, ptr(miss)) == -1
    oracle.orc_hashtable_resize(t, C.c_size_t(100_000))
    assert oracle.orc_hashtable_get_table_size(t) == 131072 * 16
    for k, i in items[:300]:
        assert oracle.orc_hashtable_query(t, ptr(np.array(k, np.int32))) == i
    m = len(uniq) // 2
    oracle.orc_hashtable_preserve(t, C.c_size_t(m))
    assert oracle.orc_hashtable_size(t) == m
    for k, i in items[:300]:
        assert oracle.orc_hashtable_query(t, ptr(np.array(k, np.int32))) == (i if i < m else -1)
    oracle.orc_hashtable_destroy(t)


def test_lbvh_morton_matches_reference_golden(oracle):
    """box centre -> unit cube -> 30-bit morton code (Bvh.hpp:177-188) vs the reference's own AABBBox / morton_code<3>
    (tests/golden/lbvh.npz from oracle/_ref), incl. the coord == 1 case where (u32)(1 * 1024) spills past 10 bits."""
    g = np.load(os.path.join(GOLD, "lbvh.npz"))
    oracle.orc_lbvh_morton.restype = C.c_uint32
    whole, bvs = g["whole"], g["bvs"]
    for b, code in zip(bvs, g["codes"]):
        assert oracle.orc_lbvh_morton(ptr(whole), ptr(b)) == code
    wb = np.zeros(6, np.float32)
    oracle.orc_lbvh_whole_box(ptr(np.ascontiguousarray(bvs[2:])), C.c_size_t(bvs.shape[0] - 2), ptr(wb))
    assert np.array_equal(wb, whole)


@pytest.mark.parametrize("n,dup", [(1, 0), (2, 0), (3, 0), (4, 0), (37, 0), (1000, 0), (3000, 1)])
def test_lbvh_oracle_structure_and_traversal(oracle, n, dup):
    """restated LBvh::build: pre-order layout invariants (Bvh.hpp:288-338) and iter_neighbors == brute force."""
    from util import lbvh_boxes, oracle_lbvh
    bv = lbvh_boxes(n, 60 + n, dup)
    b, arrs = oracle_lbvh(oracle, bv)
    nn = 2 * n - 1 if n > 2 else n
    assert arrs["numNodes"] == nn
    if n > 2:
        par, lev, aux, leaf, bvs = arrs["parents"], arrs["levels"], arrs["auxIndices"], arrs["leafInds"], arrs["bvs"]
        assert par[0] == -1 and sorted(aux[leaf].tolist()) == list(range(n))          # every primitive is exactly one leaf
        assert (lev[leaf] == 0).all() and (lev > 0).sum() == n - 1
        trunk = np.nonzero(lev > 0)[0]
        assert (par[trunk + 1] == trunk).all() and (lev[trunk + 1] == lev[trunk] - 1).all()  # left child follows its parent
        rc = np.where(lev[trunk + 1] > 0, aux[trunk + 1], trunk + 2)
        assert (par[rc] == trunk).all()
        # node boxes contain their children
        assert (bvs[trunk, :3] <= np.minimum(bvs[trunk + 1, :3], bvs[rc, :3])).all()
        assert (bvs[trunk, 3:] >= np.maximum(bvs[trunk + 1, 3:], bvs[rc, 3:])).all()
        assert np.array_equal(bvs[leaf], bv[aux[leaf]])
    out = np.zeros(n, np.int32)
    oracle.orc_lbvh_iter_neighbors.restype = C.c_size_t
    for q in range(min(n, 150)):
        k = oracle.orc_lbvh_iter_neighbors(b, ptr(bv[q]), ptr(out), C.c_size_t(n))
        ref = np.nonzero(((bv[:, :3] <= bv[q, 3:]) & (bv[:, 3:] >= bv[q, :3])).all(1))[0]
        assert np.array_equal(np.sort(out[:k]), ref)
    # self iteration over every leaf: each unordered overlapping pair once (plus the leaf itself when n > 2)
    oracle.orc_lbvh_self_iter_neighbors.restype = C.c_size_t
    if n <= 3000:
        leaf_prim = arrs["auxIndices"][arrs["leafInds"]] if n > 2 else np.arange(n)
        pairs = set()
        for k in range(n):
            c = oracle.orc_lbvh_self_iter_neighbors(b, C.c_int32(k), ptr(out), C.c_size_t(n))
            for j in out[:c]:
                if j != leaf_prim[k]:
                    key = (min(int(j), int(leaf_prim[k])), max(int(j), int(leaf_prim[k])))
                    assert key not in pairs
                    pairs.add(key)
        ov = ((bv[:, None, :3] <= bv[None, :, 3:]) & (bv[:, None, 3:] >= bv[None, :, :3])).all(2)
        ii, jj = np.nonzero(np.triu(ov, 1))
        assert pairs == set(zip(ii.tolist(), jj.tolist()))
    oracle.orc_lbvh_destroy(b)


def test_mpm_oracle_conservation(oracle):
    """size-independent properties of the restated P2G/G2P: mass & momentum conservation, affine velocity field
    reproduced exactly by P2G -> grid update -> G2P (APIC/MLS-MPM property)."""
    from util import make_cloud, OracleMpm
    dx, dt = 1.0 / 32, 1e-4
    mass, pos, vel, Cm, F = make_cloud(5, dx, 2, seed=55, vel_scale=0.0)
    n = pos.shape[0]
    A = np.array([[0.1, -0.2, 0.05], [0.3, 0.02, -0.1], [0.0, 0.15, -0.07]], np.float32)
    b = np.array([0.5, -0.25, 0.125], np.float32)
    vel = (pos @ A.T + b).astype(np.float32)
    Cm = np.tile(A.T.reshape(1, 9), (n, 1)).astype(np.float32)   # column-major C = A
    F = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))
    for side in (4, 8):
        om = OracleMpm(oracle, 0, dx, dt, side, dx ** 3 / 8)
        om.build_partition(pos, n)
        om.p2g(mass, pos, vel, Cm, F)
        g = om.grid
        assert abs(g[:, 0].sum() - mass.sum()) < 1e-5 * mass.sum()
        assert np.abs(g[:, 1:4].sum(axis=(0, 2)) - (mass[:, None] * vel).sum(0)).max() < 1e-4 * np.abs(mass[:, None] * vel).sum()
        assert np.abs(g[:, 4:7]).max() < 1e-6 * (2 * 17857 + 71428) * dx ** 3 / 8 / dx  # F = I: zero stress up to SVD rounding
        om.grid_update((0, 0, 0))
        p2, v2, C2, F2 = pos.copy(), vel.copy(), Cm.copy(), F.copy()
        om.g2p(p2, v2, C2, F2)
        assert np.abs(v2 - vel).max() < 2e-5
        assert np.abs(C2 - Cm).max() < 2e-3


def test_collider_matches_reference_golden(oracle):
    """Collider<AnalyticLevelSet<Plane|Cuboid|Sphere|Cylinder>>::resolveCollision: the C restatement reproduces the reference's
    own level-set / rotation code (tests/golden/collider.npz, 24 colliders x 96 points: all shapes, sticky / slip / separate,
    static and moving) bit for bit -- including the float finite-difference normals of the cuboid and the cylinder."""
    from util import collider_struct
    g = np.load(os.path.join(GOLD, "collider.npz"))
    assert 300 < g["inside"].sum() < g["inside"].size - 300
    for k, cs in enumerate(g["cases"]):
        c = collider_struct(cs)
        x = np.ascontiguousarray(g["x"][k])
        v = np.ascontiguousarray(g["v"][k]).copy()
        ins = np.zeros(x.shape[0], np.int32)
        oracle.orc_collider_resolve_many(C.byref(c), ptr(x), ptr(v), C.c_size_t(x.shape[0]), ptr(ins))
        assert np.array_equal(ins, g["inside"][k])
        assert np.array_equal(v, g["v_out"][k]), (k, cs[:2])
        assert np.array_equal(v[ins == 0], g["v"][k][ins == 0])          # outside: untouched


def test_vonmises_and_nacc_match_reference_golden(oracle):
    """compute_stress_vonmisesfixedcorotated / compute_stress_nacc of the HOST header (physics/ConstitutiveModel_Vol_dP.hpp:48-243)
    compiled in place -> tests/golden/stress_models.npz; the oracle's hostVariant = 1 form reproduces them.  The CUDA-header
    form (hostVariant = 0, what the GPU path follows) differs only in sqrtf-vs-Newton square roots (von Mises) and in the yield
    pressure line p0 (NACC): identical wherever -logJp <= 0."""
    g, sv = np.load(os.path.join(GOLD, "stress_models.npz")), np.load(os.path.join(GOLD, "svd_stress.npz"))
    F, mu, lam, vol = sv["F"], float(sv["mu"]), float(sv["lam"]), float(sv["vol"])
    n, cf = F.shape[0], C.c_float
    scale = (2 * mu + lam) * vol
    oracle.orc_nacc_bulk.restype = C.c_float
    oracle.orc_nacc_msqr.restype = C.c_float
    assert oracle.orc_nacc_bulk(cf(5e4), cf(0.4)) == float(g["nacc_bulk"]) and oracle.orc_nacc_msqr(cf(45.0)) == float(g["nacc_msqr"])

    def rel(a, b):
        return (np.abs(a - b) / np.maximum(np.abs(b).max(1, keepdims=True), scale)).max()
    for variant in (1, 0):
        Fv, pf = F.copy(), np.zeros((n, 9), np.float32)
        for i in range(n):
            oracle.orc_stress_vonmises(cf(vol), cf(mu), cf(lam), cf(float(g["vm_yield"])), variant, ptr(Fv[i]), ptr(pf[i]))
        ok = np.isfinite(pf).all(1)          # CUDA form: sqrtf of a negative discriminant (the host form clamps it)
        assert ok.all() if variant else ok.mean() > 0.75
        if variant:
            assert rel(pf[ok], g["PF_vm"][ok]) < 1e-4 and np.abs(Fv - g["F_vm_out"])[ok].max() < 5e-5
        else:
            # the host header's sqrtNewtonRaphson stops at an ABSOLUTE step of n * 1e-6 (MathUtils.h:246): percent-level errors
            # for the discriminant ~ mu^2 of a yielding particle, which the CUDA header's sqrtf does not have.  So the CUDA form
            # agrees tightly with the host golden where nothing was projected and only loosely elsewhere.
            still = ok & (np.abs(g["F_vm_out"] - F).max(1) == 0)
            assert still.sum() > 0 and rel(pf[still], g["PF_vm"][still]) < 1e-4
            assert rel(pf[ok], g["PF_vm"][ok]) < 0.25 and np.abs(Fv - g["F_vm_out"])[ok].max() < 0.25
        Fn, pfn, lj = F.copy(), np.zeros((n, 9), np.float32), g["logJp_in"].copy()
        for i in range(n):
            x = cf(lj[i])
            oracle.orc_stress_nacc(cf(vol), cf(mu), cf(lam), cf(float(g["nacc_bulk"])), cf(0.8), cf(0.5), cf(float(g["nacc_msqr"])), 1,
                                   variant, C.byref(x), ptr(Fn[i]), ptr(pfn[i]))
            lj[i] = x.value
        sel = slice(0, n) if variant else slice(0, n // 2)   # first half: logJp >= 0, where both headers agree
        assert rel(pfn[sel], g["PF_nacc"][sel]) < 2e-5 and np.abs(Fn - g["F_nacc_out"])[sel].max() < 2e-5
        fin = np.isfinite(g["logJp_out"])  # inverted F (Je_trial < 0): log of a negative ratio, NaN on both sides
        assert np.array_equal(np.isfinite(lj)[sel], fin[sel]) and np.abs(lj - g["logJp_out"])[sel][fin[sel]].max() < 2e-5
        if not variant:  # and the second half really takes the other yield pressure
            assert np.abs(pfn[n // 2:] - g["PF_nacc"][n // 2:]).max() > 1e-3 * scale
    assert (np.abs(g["F_vm_out"] - F).max(1) > 1e-6).mean() > 0.3 and (g["logJp_out"] != g["logJp_in"]).mean() > 0.3


def test_oracle_c2_transfers_are_consistent(oracle):
    """P2C2G / G2C2P restatement (oracle/mpm.c; the reference has no test for these functors -- the whole-function pin against its own
    headers is test_p2c2g_whole_function_matches_reference_golden below): partition of unity, Transfer == Momentum + Force, and exact
    reproduction of an affine grid field."""
    from util import OracleMpm, make_cloud
    dx, dt, side = 1.0 / 64, 1e-4, 4
    mass, pos, vel, Bm, F = make_cloud(5, dx, 2, seed=71, vel_scale=0.3)
    Bm = (Bm * dx * dx * 0.25).astype(np.float32)
    n = pos.shape[0]
    grids = []
    for kind in (0, 1, 2):
        om = OracleMpm(oracle, 0, dx, dt, side, dx ** 3 / 8)
        om.build_partition(pos, n)
        om.build_buckets(pos)
        om.p2c2g(kind, mass, pos, vel, Bm, F)
        grids.append(om.grid.copy())
    g0, g1, g2 = grids
    assert abs(g0[:, 0].sum() - mass.sum()) < 1e-5 * mass.sum() and not g2[:, 0].any() and not g0[:, 4:].any()
    mom = (mass[:, None] * vel).sum(0)
    assert np.abs(g1[:, 1:4].sum(axis=(0, 2)) - mom).max() < 1e-3 * np.abs(mass[:, None] * vel).sum()
    assert np.abs(g0 - (g1 + g2)).max() < 1e-5 * np.abs(g0).max()
    # affine field through G2C2P
    A = np.array([[0.3, -0.2, 0.1], [0.05, 0.4, -0.3], [-0.1, 0.2, 0.25]], np.float32)
    b = np.array([0.5, -0.25, 0.125], np.float32)
    loc = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    xi = ((om.keys[:, None, :] * 4 + loc[None]) * dx).astype(np.float32)
    om.grid[:] = 0
    om.grid[:, 1:4] = (xi @ A.T + b).transpose(0, 2, 1)
    om.p.dt = 0.0
    po, vo, Bo, Fo = pos.copy(), vel.copy(), Bm.copy(), F.copy()
    om.g2c2p(po, vo, Bo, Fo)
    assert np.array_equal(po, pos) and np.abs(Fo - F).max() < 1e-7
    assert np.abs(vo - (pos @ A.T + b)).max() < 2e-5
    r = pos - np.floor(pos / dx + 0.5) * dx
    grad = (Bo.reshape(-1, 3, 3) * (2.0 / (dx * dx - 2 * r * r))[:, :, None]).transpose(0, 2, 1)
    assert np.abs(grad - A[None]).max() < 2e-3


# rounding of (sigma - 1) inside the stress is amplified by mu relative to the net force on a node (sums of +- contributions
# that cancel to ~|F - I|): the same budget as the per-particle stress pin above (5e-5 (2 mu + lambda) vol), relative to the
# largest rhs entry of the fixture
STRESS_TOL = 5e-5


def _oracle_on_golden(oracle, name, side):
    from util import OracleMpm, golden_p2g_g2p
    g = golden_p2g_g2p(name, side)
    # host_variant=1: the fixture comes from the host header P2G.hpp includes (ConstitutiveModel_Vol_dP.hpp)
    om = OracleMpm(oracle, g["model"], g["dx"], g["dt"], side, g["volume"], host_variant=1, **g["kw"])
    om.adopt_partition(g["keys"])
    return g, om


@pytest.mark.parametrize("name,side", [("fixedcorotated", 4), ("fixedcorotated", 8), ("sand", 4), ("sand", 8), ("vonmises", 8), ("nacc", 8),
                                       ("eos", 8)])
def test_p2g_g2p_whole_function_matches_reference_golden(oracle, name, side):
    """P2GTransfer / G2PTransfer as WHOLE functions (simulation/transfer/P2G.hpp:51-125, G2P.hpp:44-83): the restatement in
    oracle/mpm.c against tests/golden/p2g_g2p.npz, which tools/gen_golden.py produces from the reference's own make_local_arena /
    unpack_coord_in_grid / compute_stress_* / matrixMatrixMultiplication3d in sequential particle order (oracle/ref_shim.cpp).
    Same summation order on both sides: the tolerance only has to absorb compiler-level differences inside the SVD / stress code
    (the oracle is built with -ffp-contract=off at -O2, the reference headers with g++ -O3)."""
    g, om = _oracle_on_golden(oracle, name, side)
    lj = g["logJp"].copy()
    om.p2g(g["mass"], g["pos"], g["vel"], g["C"], g["F"], lj)
    scale = np.abs(g["grid"]).max(axis=(0, 2))
    scale[4:] = g["rhs_scale"]
    err = np.abs(om.grid - g["grid"]).max(axis=(0, 2)) / scale
    assert (err[:4] <= 1e-6).all(), err                          # mass + momentum: no stress involved -> same bits up to contraction
    assert (err[4:] <= STRESS_TOL * (6 if name == 'vonmises' else 1)).all(), err  # (host von Mises: sqrtNewtonRaphson stops at an absolute step)
    #                   # stress channels: through the 4-sweep SVD
    if name in ("sand", "nacc"):
        assert np.abs(lj - g["logJp1"]).max() <= 5e-6              # sums of log(sigma): float rounding of the SVD
    # G2P on the fixture's own velocity grid
    om.grid[:] = g["gridv"]
    pos, vel, Cm, F = g["pos"].copy(), g["vel"].copy(), g["C"].copy(), g["F"].copy()
    om.g2p(pos, vel, Cm, F)
    assert np.abs(pos - g["pos1"]).max() <= 1e-7
    assert np.abs(vel - g["vel1"]).max() <= 1e-6 * np.abs(g["vel1"]).max()
    assert np.abs(Cm - g["C1"]).max() <= 1e-6 * np.abs(g["C1"]).max()
    assert np.abs(F - g["F1"]).max() <= 1e-6
    # next step's P2G on the G2P outputs (second half of the fused G2P2G pass)
    om.grid[:] = 0
    lj2 = g["logJp1"].copy()
    om.p2g(g["mass"], g["pos1"], g["vel1"], g["C1"], g["F1"], lj2)
    scale2 = np.abs(g["grid2"]).max(axis=(0, 2))
    scale2[4:] = g["rhs_scale"]
    err2 = np.abs(om.grid - g["grid2"]).max(axis=(0, 2)) / scale2
    assert (err2[:4] <= 1e-6).all() and (err2[4:] <= STRESS_TOL * (6 if name == 'vonmises' else 1)).all(), err2


def test_golden_p2g_grid_update_input_is_the_oracle_grid_update(oracle):
    """the `gridv` arrays of the fixture (input of the G2P leg) are what ComputeGridBlockVelocity (GridOp.hpp:71-108, restated in
    orc_mpm_grid_update) makes of the reference's P2G grid"""
    g, om = _oracle_on_golden(oracle, "sand", 8)
    om.grid[:] = g["grid"]
    om.grid_update(g["gravity"])
    assert np.abs(om.grid[:, :4] - g["gridv"][:, :4]).max() <= 1e-6 * np.abs(g["gridv"][:, 1:4]).max()


# ------------------------------------------------------------------------------------------- whole-function pins of the containers
BHT_SEQ_CASES = [("d3_b16", 3, 16), ("d3_b32", 3, 32), ("d3_b16_tight", 3, 16), ("d1_b16", 1, 16), ("d2_b16", 2, 16), ("d4_b16", 4, 16)]


@pytest.mark.parametrize("tag,dim,bucket", BHT_SEQ_CASES)
def test_bht_sequential_tables_match_reference_golden(oracle, tag, dim, bucket):
    """oracle/bht.c against tests/golden/containers_seq.npz -- tables produced by the bodies of BHTView::insert / query (container/Bht.hpp:
    612-698) spelled over the reference's own universal_hash_base / hash_combine / storage_key_type_impl / next_2pow (oracle/ref_shim.cpp)
    under sequential insertion in input order: padded key slots byte for byte, indices of the occupied slots, status, activeKeys, count,
    build-success flag, every insert return value (incl. the failure token of the over-full `tight` case) and the queries."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "containers_seq.npz"))
    keys, nexp = np.ascontiguousarray(z[tag + "_keys"]), int(z[tag + "_n_expected"])
    n = keys.shape[0]
    oracle.orc_bht_create_b.restype = C.c_void_p
    oracle.orc_bht_get_table_size.restype = C.c_size_t
    oracle.orc_bht_size.restype = C.c_int32
    oracle.orc_bht_build_success.restype = C.c_int32
    for f in ("keys", "indices", "status", "active_keys"):
        getattr(oracle, "orc_bht_" + f).restype = C.POINTER(C.c_int32)
    t = C.c_void_p(oracle.orc_bht_create_b(dim, C.c_size_t(nexp), bucket))
    ret = np.zeros(n, np.int32)
    oracle.orc_bht_insert_many(t, ptr(keys), C.c_size_t(n), ptr(ret))
    ts = oracle.orc_bht_get_table_size(t)
    gk = z[tag + "_table_keys"]
    assert ts == gk.shape[0] and oracle.orc_bht_key_stride(t) == gk.shape[1]
    assert np.array_equal(ret, z[tag + "_ret"])
    assert oracle.orc_bht_size(t) == int(z[tag + "_cnt"]) and oracle.orc_bht_build_success(t) == int(z[tag + "_success"])
    if tag.endswith("tight"):
        assert int(z[tag + "_success"]) == 0 and (z[tag + "_ret"] == np.iinfo(np.int32).min).any()   # the fixture does exercise the overflow path
    tk = np.ctypeslib.as_array(oracle.orc_bht_keys(t), shape=gk.shape)
    assert np.array_equal(tk, gk)                                                                    # pad words included
    occ = (gk[:, :dim] != 0x3f3f3f3f).any(1)
    assert np.array_equal(np.ctypeslib.as_array(oracle.orc_bht_indices(t), shape=(ts,))[occ], z[tag + "_indices"][occ])
    assert np.array_equal(np.ctypeslib.as_array(oracle.orc_bht_status(t), shape=(ts,)), z[tag + "_status"])
    cnt = int(z[tag + "_cnt"])
    assert np.array_equal(np.ctypeslib.as_array(oracle.orc_bht_active_keys(t), shape=(cnt, dim)), z[tag + "_active_keys"])
    q = np.ascontiguousarray(z[tag + "_queries"])
    qr = np.zeros(q.shape[0], np.int32)
    oracle.orc_bht_query_many(t, ptr(q), C.c_size_t(q.shape[0]), ptr(qr))
    assert np.array_equal(qr, z[tag + "_query_ret"])
    oracle.orc_bht_destroy(t)


def test_hashtable_sequential_table_matches_reference_golden(oracle):
    """oracle/hashtable.c against the reference-made table of HashTable<int, 3, int> (container/HashTable.hpp:88-91 sizing, 383-400 insert,
    454-463 query, 496-500 hash) under sequential insertion: keys, indices, activeKeys, count, return values, queries."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "containers_seq.npz"))
    keys = np.ascontiguousarray(z["ht_keys"])
    n = keys.shape[0]
    oracle.orc_hashtable_create.restype = C.c_void_p
    oracle.orc_hashtable_size.restype = C.c_int32
    oracle.orc_hashtable_get_table_size.restype = C.c_int32
    for f in ("keys", "indices", "active_keys"):
        getattr(oracle, "orc_hashtable_" + f).restype = C.POINTER(C.c_int32)
    t = C.c_void_p(oracle.orc_hashtable_create(3, C.c_size_t(n)))
    ret = np.zeros(n, np.int32)
    oracle.orc_hashtable_insert_many(t, ptr(keys), C.c_size_t(n), ptr(ret))
    ts = oracle.orc_hashtable_get_table_size(t)
    assert ts == z["ht_table_keys"].shape[0] and np.array_equal(ret, z["ht_ret"])
    cnt = int(z["ht_cnt"])
    assert oracle.orc_hashtable_size(t) == cnt
    assert np.array_equal(np.ctypeslib.as_array(oracle.orc_hashtable_keys(t), shape=(ts, 3)), z["ht_table_keys"])
    assert np.array_equal(np.ctypeslib.as_array(oracle.orc_hashtable_indices(t), shape=(ts,)), z["ht_indices"])
    assert np.array_equal(np.ctypeslib.as_array(oracle.orc_hashtable_active_keys(t), shape=(cnt, 3)), z["ht_active_keys"])
    q = np.ascontiguousarray(z["ht_queries"])
    qr = np.zeros(q.shape[0], np.int32)
    oracle.orc_hashtable_query_many(t, ptr(q), C.c_size_t(q.shape[0]), ptr(qr))
    assert np.array_equal(qr, z["ht_query_ret"])
    oracle.orc_hashtable_destroy(t)


@pytest.mark.parametrize("name,side", [("fixedcorotated", 4), ("fixedcorotated", 8), ("vonmises", 8), ("eos", 4), ("eos", 8)])
def test_p2c2g_whole_function_matches_reference_golden(oracle, name, side):
    """P2C2GTransfer as a WHOLE function (simulation/transfer/P2C2G.hpp:53-189): oracle/mpm.c against tests/golden/c2.npz, which
    tools/gen_golden.py produces from the functor body spelled over the reference's own vec / lower_trunc / compute_stress_* /
    unpack_coord_in_grid, cells in launch order, buckets in ascending particle id (oracle/ref_shim.cpp).  Same summation order on both
    sides.  (The plastic models with logJp are not in the fixture: the reference functor re-runs their update per (cell, particle) pair.)"""
    from util import OracleMpm, golden_c2
    g = golden_c2(name, side)
    om = OracleMpm(oracle, g["model"], g["dx"], g["dt"], side, g["volume"], host_variant=1, **g["kw"])
    om.adopt_partition(g["keys"])
    om.build_buckets(g["pos"])
    om.p2c2g(0, g["mass"], g["pos"], g["vel"], g["B"], g["F"], None)
    scale = np.abs(g["grid"]).max(axis=(0, 2))
    err = np.abs(om.grid[:, :4] - g["grid"]).max(axis=(0, 2)) / scale
    assert err[0] <= 1e-6 and (err[1:] <= (STRESS_TOL * 6 if name == "vonmises" else max(STRESS_TOL, 2e-6))).all(), err
    assert not om.grid[:, 4:].any()


@pytest.mark.parametrize("side", [4, 8])
def test_g2c2p_whole_function_matches_reference_golden(oracle, side):
    """G2C2PTransfer (simulation/transfer/G2C2P.hpp:59-135) on the fixture's velocity grid: v_p and B_p accumulated from zero"""
    from util import OracleMpm, golden_c2
    g = golden_c2("fixedcorotated", side)
    om = OracleMpm(oracle, 0, g["dx"], g["dt"], side, g["volume"])
    om.adopt_partition(g["keys"])
    om.build_buckets(g["pos"])
    om.grid[:, 1:4] = g["gridv"]
    vel, Bm = np.zeros_like(g["vel"]), np.zeros_like(g["B"])
    om.o.orc_mpm_g2c2p(__import__("ctypes").byref(om.p), om.table, om.buckets, om._ib[1], om._ib[2], g["pos"].ctypes.data_as(__import__("ctypes").c_void_p),
                       vel.ctypes.data_as(__import__("ctypes").c_void_p), Bm.ctypes.data_as(__import__("ctypes").c_void_p),
                       om.grid.ctypes.data_as(__import__("ctypes").c_void_p))
    assert np.abs(vel - g["vel1"]).max() <= 1e-6 * np.abs(g["vel1"]).max()
    assert np.abs(Bm - g["B1"]).max() <= 2e-6 * np.abs(g["B1"]).max()
