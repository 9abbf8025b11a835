"""Size-independent properties at the sizes BASELINE.json names (the parity tests proper run at sizes the oracle finishes in seconds):
config 1 primitives at 1 M ints against numpy; config 2 bht at 16 M keys; config 3 the 8 M-particle jello cube; config 4 the 64 Mi-particle
sand column (fused slotted == fused compact == unfused, nothing lost, particle number conserved); config 5 LBvh at 10 M boxes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])


CHANNELS = (["m"] + ["x%d" % k for k in range(3)] + ["v%d" % k for k in range(3)] + ["C%d" % k for k in range(9)]
            + ["F%d" % k for k in range(9)] + ["logJp"] + ["PFt%d" % k for k in range(6)])


def _same_state(a, b, npart, tol_sum, tol_sq):
    """channel sums and sums of squares of two runs; the failure message names the channels and by how much"""
    a, b = np.array(a), np.array(b)
    nch = len(a) // 2
    names = CHANNELS if nch >= 32 else [c for c in CHANNELS if c != "logJp"]
    scale = np.sqrt(npart * np.maximum(a[nch:], 1e-30))
    r_sum = np.abs(a[:nch] - b[:nch]) / (tol_sum * scale + 1e-12)
    r_sq = np.abs(a[nch:] - b[nch:]) / (tol_sq * np.abs(a[nch:]) + 1e-12)
    bad = [("sum " + names[k], float(r_sum[k]), float(a[k]), float(b[k])) for k in range(nch) if r_sum[k] > 1] + \
          [("sq " + names[k], float(r_sq[k]), float(a[nch + k]), float(b[nch + k])) for k in range(nch) if r_sq[k] > 1]
    assert not bad, "channels outside tolerance (name, |d|/tol, a, b): %r" % (bad,)


def test_config1_primitives_at_1m_ints(pol):
    """BASELINE config 1: reduce / exclusive_scan / radix_sort on 1 M ints, bit-exact against numpy"""
    import zpc_amd as zs
    a = np.random.default_rng(11).integers(-2 ** 31, 2 ** 31 - 1, 1 << 20, dtype=np.int64).astype(np.int32)
    d = torch.from_numpy(a).cuda()
    out = torch.empty_like(d)
    r = torch.zeros(1, dtype=torch.int32, device="cuda")
    zs.reduce(pol, d, None, r)
    assert int(r.item()) == int(np.sum(a, dtype=np.int64).astype(np.int32))
    zs.exclusive_scan(pol, d, out)
    assert np.array_equal(out.cpu().numpy(), (np.cumsum(a, dtype=np.int64) - a).astype(np.int32))
    zs.radix_sort(pol, d, out)
    assert np.array_equal(out.cpu().numpy(), np.sort(a))


def test_scans_above_128_mb_take_the_streaming_store_path(pol):
    """Outputs of >= 128 MB are written with non-temporal stores (r04): exclusive and inclusive scans of 40 M + 1 ints (ragged last tile)
    and 20 M + 3 int64 values, out of place and in place, bit-exact against numpy's wrapping cumsum."""
    import zpc_amd as zs
    g = np.random.default_rng(23)
    a = g.integers(-2 ** 31, 2 ** 31 - 1, 40_000_001, dtype=np.int64).astype(np.int32)
    d = torch.from_numpy(a).cuda()
    out = torch.empty_like(d)
    inc = np.cumsum(a, dtype=np.int64).astype(np.int32)
    zs.exclusive_scan(pol, d, out)
    assert np.array_equal(out.cpu().numpy(), inc - a)
    zs.inclusive_scan(pol, d, out)
    assert np.array_equal(out.cpu().numpy(), inc)
    zs.exclusive_scan(pol, d, d, init=5)
    assert np.array_equal(d.cpu().numpy(), (inc - a + np.int32(5)).astype(np.int32))
    del d, out
    b = g.integers(-2 ** 62, 2 ** 62, 20_000_003, dtype=np.int64)
    db = torch.from_numpy(b).cuda()
    ob = torch.empty_like(db)
    zs.inclusive_scan(pol, db, ob)
    assert np.array_equal(ob.cpu().numpy(), np.cumsum(b))


def test_config2_bht_16m_keys(pol, oracle):
    """BASELINE config 2: bht build over 16 M random cells (10.6 M distinct).  With the reference's sizing (2 next_2pow(n) slots in
    buckets of 16, 15 usable) and its universal hash, a few dozen keys find all three of their buckets full: the reference's insert
    returns its failure token for them and clears `success` (Bht.hpp:536-541; the caller is expected to resize and rebuild).  The
    sequential oracle loses 73 keys on this input, the GPU build -- another insertion order -- about as many.  Checked: every key is
    either stored or reported; stored keys get one dense index each, queries return it, activeKeys[index] == key."""
    from zpc_amd.containers import Bht
    n = 1 << 24
    g = np.random.default_rng(12)
    keys = g.integers(0, 256, (n, 3), dtype=np.int32)
    packed = (keys[:, 0].astype(np.int64) << 16) | (keys[:, 1].astype(np.int64) << 8) | keys[:, 2]
    ndist = np.unique(packed).shape[0]
    oracle.orc_bht_create_b.restype = C.c_void_p
    oracle.orc_bht_size.restype = C.c_int32
    ot = C.c_void_p(oracle.orc_bht_create_b(3, C.c_size_t(n), 16))
    oracle.orc_bht_insert_many(ot, keys.ctypes.data_as(C.c_void_p), C.c_size_t(n), None)
    olost = ndist - oracle.orc_bht_size(ot)
    oracle.orc_bht_destroy(ot)
    tab = Bht(3, n)
    dk = torch.from_numpy(keys).cuda()
    ret = torch.empty(n, dtype=torch.int32, device="cuda")
    tab.insert(pol, dk.data_ptr(), n, ret.data_ptr())
    q = torch.empty(n, dtype=torch.int32, device="cuda")
    tab.query(pol, dk.data_ptr(), n, q.data_ptr())
    pol.syncCtx()
    qi, r = q.cpu().numpy(), ret.cpu().numpy()
    size = tab.size()
    lost = ndist - size
    print("bht 16 M keys: %d distinct, lost by the sequential oracle %d, lost by the GPU build %d" % (ndist, olost, lost))
    # The parallel build inserts in another order than the sequential oracle, so WHICH keys find their buckets full differs from run to
    # run and no bound on the count says anything about the keys.  What Bht.hpp:490-541 promises is checked instead, further down: a
    # key fails only if each of its three buckets is full (more than B - 2 = 14 slots taken: 15 foreign keys) and does not hold it.
    assert lost >= 0
    v = tab.view()
    succ = np.empty(1, np.int32)
    C.CDLL("libamdhip64.so").hipMemcpy(succ.ctypes.data_as(C.c_void_p), C.c_void_p(v.success), C.c_size_t(4), 2)
    assert (succ[0] == 0) == (lost > 0)
    failed = r < -1                                                   # failure_token_v: reported, never silent
    assert np.unique(packed[failed]).shape[0] == lost and (qi[failed] < 0).all()
    if lost:  # every failed key: its three buckets in the FINAL table are full of other keys (nothing is ever removed from a bucket)
        hip = C.CDLL("libamdhip64.so")
        B, PRIME = 16, np.uint64(4294967291)
        fk = keys[failed][np.unique(packed[failed], return_index=True)[1]].astype(np.int64)

        def h1(hx, hy, k):  # universal_hash (py_interop/HashUtils.hpp:23-43): ((hx ^ k) + hy) mod 2^32, then mod prime
            return (((np.uint64(hx) ^ (k.astype(np.uint64) & np.uint64(0xffffffff))) + np.uint64(hy)) & np.uint64(0xffffffff)) % PRIME

        def hkey(hx, hy):   # folded with hash_combine (math/Hash.hpp:19-28), 32-bit arithmetic
            ret = h1(hx, hy, fk[:, 0])
            for d in (1, 2):
                vv = h1(hx, hy, fk[:, d])
                ret = (ret ^ ((vv + np.uint64(0x9e3779b9) + (ret << np.uint64(6)) + (ret >> np.uint64(2))) & np.uint64(0xffffffff))) & np.uint64(0xffffffff)
            return ret
        slot = np.empty(B * 4, np.int32)
        for hx, hy in ((v.hf0x, v.hf0y), (v.hf1x, v.hf1y), (v.hf2x, v.hf2y)):
            bucket = (hkey(hx, hy) % np.uint64(v.numBuckets)).astype(np.int64) * B
            for j in range(fk.shape[0]):
                hip.hipMemcpy(slot.ctypes.data_as(C.c_void_p), C.c_void_p(v.keys + int(bucket[j]) * 16), C.c_size_t(slot.nbytes), 2)
                sl = slot.reshape(B, 4)[:, :3]
                taken = ~(sl == 0x3f3f3f3f).all(1)
                assert taken.sum() >= B - 1, (fk[j], int(taken.sum()))             # load > threshold = B - 2 (Bht.hpp:34, :517)
                assert not (sl[taken] == fk[j]).all(1).any(), fk[j]                # ... and none of them is the key itself
    stored = qi >= 0
    assert stored.sum() == n - np.isin(packed, np.unique(packed[failed])).sum()
    assert qi[stored].max() == size - 1 and (r >= 0).sum() == size   # one winner per stored key
    o = np.argsort(packed, kind="stable")                             # same key <-> same index
    same_key = packed[o][1:] == packed[o][:-1]
    both = stored[o][1:] & stored[o][:-1]
    assert np.array_equal(same_key[both], (qi[o][1:] == qi[o][:-1])[both])
    act = np.empty(size * 3, np.int32)
    C.CDLL("libamdhip64.so").hipMemcpy(act.ctypes.data_as(C.c_void_p), C.c_void_p(v.activeKeys), C.c_size_t(act.nbytes), 2)
    sample = np.nonzero(stored)[0][::83]
    assert np.array_equal(act.reshape(size, 3)[qi[sample]], keys[sample])


def test_config2_tilevector_16m_aosoa_load_store(pol):
    """BASELINE config 2, TileVector half: TileVector<f32, 32>{m:1, x:3, v:3, F:9, C:9} (25 channels, 100 B per particle, 1.6 GB) at 16 M
    particles -- the container through the reference's C ABI (container__tv_float_32, get_iterator_1__tv_float_32), element (chn, i) at
    (i / L * C + chn) * L + i % L (container/TileVector.hpp:108, 397): an AoS -> AoSoA store of every channel, the load + store pass over
    all channels (zs_rocm_tv_scale_f32, the kernel the secondary bench line times), and reads back through the channel iterators -- checked
    against the closed form of the fill on a strided sample of particles and on per-channel sums (reduce over the iterator ABI)."""
    import zpc_amd as zs
    from zpc_amd.containers import TileVector
    from zpc_amd.primitives import Iter
    n, L = 16_000_000, 32
    tags = [("m", 1), ("x", 3), ("v", 3), ("F", 9), ("C", 9)]
    tv = TileVector("float", L, tags, n)
    Cn = tv.numChannels()
    assert Cn == 25 and tv.size() == n and [tv.getPropertyOffset(k) for k in ("m", "x", "v", "F", "C")] == [0, 1, 4, 7, 16]
    # value of (particle i, channel c): small integers, exact in float32 and under the power-of-two scaling
    i = torch.arange(n, device="cuda", dtype=torch.int64)
    aos = torch.stack([((i * (c + 3) + c * 7) % 1021 - 510).float() for c in range(Cn)], dim=1).contiguous()
    zs.lib().zs_rocm_tv_from_aos_f32(pol.handle, aos.data_ptr(), n, Cn, L, tv.data())
    zs.lib().zs_rocm_tv_scale_f32(pol.handle, tv.data(), n, Cn, L, C.c_float(0.5))
    pol.syncCtx()
    raw = np.empty(n * Cn, np.float32)   # n is a multiple of L: no padding tile
    C.CDLL("libamdhip64.so").hipMemcpy(raw.ctypes.data_as(C.c_void_p), C.c_void_p(tv.data()), C.c_size_t(raw.nbytes), 2)
    sample = np.arange(0, n, 4099, dtype=np.int64)
    for c in (0, 1, 6, 7, 15, 16, 24):
        want = (((sample * (c + 3) + c * 7) % 1021) - 510).astype(np.float32) * np.float32(0.5)
        got = raw[(sample // L * Cn + c) * L + sample % L]                       # the layout formula of the reference
        assert np.array_equal(got, want), c
    # per-channel sums through the reference's iterator ABI (exact: the addends are multiples of 0.5 and the sum fits in a double)
    out = torch.zeros(1, dtype=torch.float32, device="cuda")
    full = aos.double().sum(dim=0).cpu().numpy() * 0.5
    for name, comp, c in (("m", 0, 0), ("v", 2, 6), ("C", 8, 24)):
        it = tv.iterator(name) if comp == 0 else tv.iterator(tv.getPropertyOffset(name) + comp)
        last = type(it)(it.base, it.idx + n, it.numTileBits, it.tileMask, it.numChns)
        zs.lib().reduce_sum__rocm_float_1(pol.handle, it, last, Iter.aos(out).port)
        # float32 tree sum of 16 M addends: a few ulp of the sum of magnitudes (the reference's own float test uses 1e-6 relative on
        # 1000 elements, test/utils/parallel_primitives.hpp:30)
        assert abs(float(out.item()) - full[c]) <= 4e-6 * aos[:, c].abs().double().sum().item() * 0.5, (name, float(out.item()), full[c])


def test_config5_lbvh_10m_boxes(pol):
    """BASELINE config 5: LBvh over 10 M boxes: structural invariants of the pre-order layout (parents, levels, escape indices, leaf
    positions, boxes contain their children) and the self-collision pairs of sampled leaves against brute force"""
    from zpc_amd.containers import LBvh
    n = 10_000_000
    g = np.random.default_rng(15)
    c = g.uniform(0, 1, (n, 3)).astype(np.float32)
    e = g.uniform(0.0005, 0.002, (n, 3)).astype(np.float32)
    bv = np.ascontiguousarray(np.concatenate([c - e, c + e], axis=1))
    d = torch.from_numpy(bv).cuda()
    bvh = LBvh()
    bvh.build(pol, d)
    pol.syncCtx()
    v = bvh.view()
    nn = v.numNodes
    assert nn == 2 * n - 1

    def d2h(p, cnt, dt=np.int32):
        out = np.empty(cnt, dt)
        C.CDLL("libamdhip64.so").hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(out.nbytes), 2)
        return out
    par, lev, aux, lin = d2h(v.parents, nn), d2h(v.levels, nn), d2h(v.auxIndices, nn), d2h(v.leafInds, n)
    boxes = d2h(v.orderedBvs, nn * 6, np.float32).reshape(nn, 6)
    assert par[0] == -1 and (par[1:] >= 0).all() and (par[1:] < np.arange(1, nn)).all()       # pre-order: a parent precedes its children
    leaf = lev == 0
    assert leaf.sum() == n and np.array_equal(np.sort(aux[leaf]), np.arange(n))                 # every primitive is one leaf
    assert np.array_equal(np.sort(lin), np.nonzero(leaf)[0])
    trunk = ~leaf
    esc = aux[trunk]
    pos = np.nonzero(trunk)[0]
    assert ((esc == -1) | (esc > pos)).all()                                                    # escape indices point forward
    # a trunk node's box contains the box of the node right behind it (its left child) and of its parent's view of it
    lc = pos + 1
    assert (boxes[pos, :3] <= boxes[lc, :3]).all() and (boxes[pos, 3:] >= boxes[lc, 3:]).all()
    assert np.array_equal(boxes[lin], bv[aux[lin]])                                             # leaf boxes are the primitives' boxes
    # self-collision pairs of 300 sampled primitives vs brute force
    offs, pairs = bvh.self_query(pol)
    pol.syncCtx()
    p = pairs.cpu().numpy()
    sample = g.integers(0, n, 300)
    for s in sample:
        ov = ((bv[:, :3] <= bv[s, 3:]) & (bv[:, 3:] >= bv[s, :3])).all(1)
        want = set(np.nonzero(ov)[0].tolist()) - {int(s)}
        got = set(p[p[:, 0] == s][:, 1].tolist()) | set(p[p[:, 1] == s][:, 0].tolist())
        assert got == want, (s, len(got), len(want))


def test_config3_jello_8m_fused_equals_unfused():
    """BASELINE config 3 (8 M-particle FixedCorotated cube on the 256^3 grid): three steps, slotted fused == compact fused == unfused"""
    base = ["--cells", "100,100,100", "--model", "jello", "--grid", "256", "--steps", "3", "--warmup", "0", "--no-cpu-baseline", "--checksum",
            "--no-at-rest", "--drift", "0,-0.5,0", "--lift", "8"]  # (lift: see the 24-step test)
    a = _bench(base)
    b = _bench(base + ["--compact"])
    # (with --checksum the fused variants run one more step that materialises v, C and the stress of every particle)
    c = _bench([x if x != "3" else "4" for x in base] + ["--compact", "--unfused"])
    assert a["config"]["particles"] == 8_000_000 and a["hip_error"] == 0 and "slotted" in a["config"]["storage"]
    _same_state(a["checksum"], b["checksum"], 8_000_000, 2e-5, 1e-4)
    _same_state(a["checksum"], c["checksum"], 8_000_000, 2e-5, 1e-4)


def test_config4_sand_64m_fused_equals_unfused():
    """BASELINE config 4 at N = 1 (64 Mi-particle DruckerPrager column, dx = 1/512) falling at 0.05 cell per step: after three steps the
    slotted fused step, the compact fused step and the unfused P2G / G2P kernels hold the same particle state (channel sums and sums of
    squares); the slotted run delivered every mover it sent and lost no particle"""
    base = ["--steps", "3", "--warmup", "0", "--no-cpu-baseline", "--checksum", "--no-at-rest", "--lift", "8"]  # (lift: see the 24-step test)
    a = _bench(base)
    b = _bench(base + ["--compact"])
    c = _bench([x if x != "3" else "4" for x in base] + ["--compact", "--unfused"])
    n = 67_108_864
    assert a["config"]["particles"] == n and a["hip_error"] == 0 and a["config"]["movers_per_step_rank0"] > 1e6
    _same_state(a["checksum"], b["checksum"], n, 2e-5, 1e-4)
    _same_state(a["checksum"], c["checksum"], n, 2e-5, 1e-4)
    # mass channel: sum == n * m exactly in float64 (every particle still there, once)
    m = 1000.0 * (1.0 / 512) ** 3 / 8
    assert abs(a["checksum"][0] - n * np.float32(m)) <= 1e-9 * n * m


def test_config4_sand_64m_slotted_24_moving_steps_equal_compact_with_rebins():
    """24 steps of the falling 64 Mi-particle column (1.3 cells of travel: a third of the particles change cell, every bin's rounds
    have become uneven): the slotted step -- packed producers, movers through the outboxes, no re-bin -- against the compact storage
    with the re-bin controller; same particle state, every mover delivered, nobody lost."""
    # (--lift 8: the column stands one block above y = 0, where the reference's arena has no local position that rounds to 1.5 -- on y = 0
    # one foot particle is weighted a cell off in ~3 % of the compact-storage runs, profiles/r03_compact_outliers.md; two runs then differ)
    base = ["--steps", "24", "--warmup", "0", "--no-cpu-baseline", "--checksum", "--no-at-rest", "--lift", "8"]
    a = _bench(base + ["--slot-stats"])
    b = _bench(base + ["--compact", "--rebin-check", "2"])
    n = 67_108_864
    assert a["config"]["particles"] == n and a["hip_error"] == 0 and b["hip_error"] == 0
    assert a["config"]["rebins"] == 0 and b["config"]["rebins"] > 0
    assert a["slot_stats"]["mean_rounds"] > a["slot_stats"]["mean_particles_per_bin_div64"] + 1.0  # the regime the packing is for
    # the trimmed sums (bench.py: particles with a velocity-gradient entry beyond 8 rms are left out: what a hit of the arena's rounding
    # case leaves behind, and the two edge particles of the column that carry such entries in every run) must agree, and few may be trimmed
    ta, tb = a["checksum_trimmed"], b["checksum_trimmed"]
    # bound tied to measurements: 11 (slotted) and 76 (compact) particles were trimmed in the r03 runs, of 67 M; a defect that touches more
    # than a couple of hundred particles must not hide behind the filter
    assert ta["trimmed_particles"] <= 200 and tb["trimmed_particles"] <= 200, (ta["trimmed_particles"], tb["trimmed_particles"])
    _same_state(ta["sums"], tb["sums"], n, 1e-4, 3e-4)
    m = 1000.0 * (1.0 / 512) ** 3 / 8
    assert abs(a["checksum"][0] - n * np.float32(m)) <= 1e-9 * n * m


def test_config4_sand_64m_on_the_floor_two_storages_agree_outside_the_foot_layer():
    """BASELINE's geometry proper: the column stands ON y = 0 (--lift 0).  There the reference's arena has local positions that round
    to exactly 1.5 next to the origin; a particle that hits the case is weighted a cell off by the reference and by us alike, and what it
    leaves behind differs between two runs only in the column's foot layer.  12 moving steps, slotted against compact storage: the
    trimmed sums agree, few particles are trimmed, and every trimmed particle lies within the lowest three cell layers."""
    base = ["--steps", "12", "--warmup", "0", "--no-cpu-baseline", "--checksum", "--no-at-rest", "--lift", "0"]
    a = _bench(base)
    b = _bench(base + ["--compact", "--rebin-check", "2"])
    n = 67_108_864
    assert a["config"]["particles"] == n and a["hip_error"] == 0 and b["hip_error"] == 0
    ta, tb = a["checksum_trimmed"], b["checksum_trimmed"]
    print("un-lifted column: trimmed", ta["trimmed_particles"], tb["trimmed_particles"], "highest trimmed particle (cells above y = 0)",
          ta["trimmed_max_y_cells"], tb["trimmed_max_y_cells"])
    assert ta["trimmed_particles"] <= 200 and tb["trimmed_particles"] <= 200
    for t in (ta, tb):
        assert t["trimmed_particles"] == 0 or t["trimmed_max_y_cells"] <= 3.0 or t["trimmed_edge_particles"] == t["trimmed_particles"], t
    _same_state(ta["sums"], tb["sums"], n, 1e-4, 3e-4)
    m = 1000.0 * (1.0 / 512) ** 3 / 8
    assert abs(a["checksum"][0] - n * np.float32(m)) <= 1e-9 * n * m


# ------------------------------------------------------------------------------------------------ full-size runs anchored to the ORACLE
def _id_box_step(pol, oracle, model, grid_n, cells, drift, box_lo, steps_before, K=24, outbox_cap=128):
    """The full-size column of bench.py on slotted storage, moved for `steps_before` fused steps; then ONE more fused step whose inputs
    (particle state of a 32^3-cell sub-box, node velocities of the enclosing grid blocks) are handed to the CPU oracle
    (oracle/mpm.c: G2P, simulation/transfer/G2P.hpp:44-83, then P2G, P2G.hpp:51-125) and whose outputs are compared with it particle
    for particle (identity = a unique mass given to the sub-box particles at t = 0) and node for node (interior nodes of the box).
    Returns the dict of measured deviations / scales."""
    import bench
    from zpc_amd.mpm import MpmTransfer
    from util import OracleMpm
    dx, dt, side = 1.0 / grid_n, 1e-4, 8
    glo = [(grid_n - cells[0]) // 2 // side * side, 0, (grid_n - cells[2]) // 2 // side * side]
    ghi = [glo[d] + cells[d] for d in range(3)]
    dev = torch.device("cuda", 0)
    aos = bench.generate_particles(glo, ghi, dx, 1234, dev, model)
    for k in range(3):
        aos[:, 4 + k] += drift[k]
    n = aos.shape[0]
    # identities: the particles of the 32^3-cell box get pairwise different masses m0 (1 + j 2^-20); everybody else 0.99 m0
    m0 = float(aos[0, 0].item())
    cell = torch.floor(aos[:, 1:4] / dx).to(torch.int32)
    box_hi = [box_lo[d] + 32 for d in range(3)]
    inb = torch.ones(n, dtype=torch.bool, device=dev)
    for d in range(3):
        inb &= (cell[:, d] >= box_lo[d]) & (cell[:, d] < box_hi[d])
    ids = torch.nonzero(inb).flatten()
    nid = int(ids.numel())
    assert nid == 32 ** 3 * 8
    aos[:, 0] = 0.99 * m0
    aos[ids, 0] = (m0 * (1.0 + torch.arange(nid, device=dev, dtype=torch.float64) * 2.0 ** -20)).float()
    del cell, inb
    vol = dx ** 3 / 8
    mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True)
    aos = torch.cat([aos, torch.zeros(n, mt.nchn - aos.shape[1], dtype=torch.float32, device=dev)], dim=1).contiguous()
    import zpc_amd
    zpc_amd.lib().zs_rocm_tv_from_aos_f32(pol.handle, aos.data_ptr(), n, mt.nchn, mt.L, mt.buf.data_ptr())
    pol.syncCtx()
    del aos
    g = (0.0, -9.8, 0.0)
    mt.build_partition(max(4096, n // 128), margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update(g)
    mt.slot(K=K, outbox_cap=outbox_cap)
    for _ in range(steps_before):
        mt.g2p2g()
        mt.grid_update(g)
    pol.syncCtx()
    mt.check_slots()   # folds the 8 warm-up steps into the run-level record and clears the device words

    def id_particles():
        """[nid, nchn] rows of the particles that carry an identity, sorted by it"""
        cbuf, cnt = mt._compact_copy()          # occupied slots only (a vacated slot keeps its stale record; its mask bit is clear)
        assert cnt == n
        v = cbuf.view(-1, mt.nchn, 64)
        m = v[:, 0, :]
        sel = torch.nonzero((m >= m0) & (m < 1.3 * m0))
        rows = v[sel[:, 0], :, sel[:, 1]]
        o = torch.argsort(rows[:, 0])
        return rows[o].cpu().numpy()
    a = id_particles()
    assert a.shape[0] == nid and np.unique(a[:, 0]).shape[0] == nid            # every identity exactly once after the moving steps
    keys = mt.active_keys()
    base = np.floor(a[:, 1:4] / dx - 0.5).astype(np.int64)
    klo, khi = base.min(0) // side - 1, (base.max(0) + 2) // side + 1
    selb = np.nonzero(((keys >= klo) & (keys <= khi)).all(1))[0]
    gridA = mt.grid.view(mt.nblocks, 7, side ** 3)[torch.from_numpy(selb).to(dev)].cpu().numpy()
    kw = dict(E=5e4, nu=0.4)
    om = OracleMpm(oracle, model, dx, dt, side, vol, nthreads=8, **kw)
    om.adopt_partition(keys[selb])
    om.grid[:] = gridA
    mass = np.ascontiguousarray(a[:, 0])
    pos, vel = np.ascontiguousarray(a[:, 1:4]), np.ascontiguousarray(a[:, 4:7])
    Cm, F = np.ascontiguousarray(a[:, 7:16]), np.ascontiguousarray(a[:, 16:25])
    lj = np.ascontiguousarray(a[:, 25]) if model == 1 else np.zeros(nid, np.float32)
    om.g2p(pos, vel, Cm, F)
    om.grid[:] = 0
    om.p2g(mass, pos, vel, Cm, F, lj)
    # the same step on the GPU (write_all: v, C of every particle are stored as well)
    mt.g2p2g(write_all=True)
    pol.syncCtx()
    st1 = mt.check_slots()
    b = id_particles()
    assert np.array_equal(b[:, 0], mass)                                       # nobody lost, nobody duplicated
    gridB = mt.grid.view(mt.nblocks, 7, side ** 3)[torch.from_numpy(selb).to(dev)].cpu().numpy()
    out = {"movers_in_step": st1[5], "n_id": nid}   # check_slots() returns the period since the previous call: this one step
    out["x"] = float(np.abs(b[:, 1:4] - pos).max())
    out["v"] = float(np.abs(b[:, 4:7] - vel).max() / np.abs(vel).max())
    out["C"] = float(np.abs(b[:, 7:16] - Cm).max() / np.abs(Cm).max())
    out["F"] = float(np.abs(b[:, 16:25] - F).max())
    if model == 1:
        out["logJp"] = float(np.abs(b[:, 25] - lj).max())
    # how many of the identified particles changed cell since t = 0 / in this step
    out["changed_cell_in_step"] = int((np.floor(b[:, 1:4] / dx - 0.5).astype(np.int64) != base).any(1).sum())
    # interior nodes: 3 cells inside the box faces (the box has fallen < 1 cell), so every contributor carries an identity
    kk = keys[selb]
    c = np.arange(side ** 3)
    loc = np.stack([c // (side * side), (c // side) % side, c % side], 1)
    node = kk[:, None, :] * side + loc[None, :, :]
    interior = np.ones(node.shape[:2], bool)
    for d in range(3):
        interior &= (node[:, :, d] >= box_lo[d] + 3) & (node[:, :, d] < box_hi[d] - 3)
    assert interior.sum() == 26 ** 3
    scale = np.abs(om.grid).max(axis=(0, 2)) + 1e-30
    diff = np.abs(gridB - om.grid)
    out["grid"] = [float(diff[:, ch, :][interior].max() / scale[ch]) for ch in range(7)]
    out["grid_mass_interior"] = float(om.grid[:, 0, :][interior].min())
    # in addition: every identified particle and every interior node within its own float64 bound (tests/ref64.py), from the GPU's
    # own inputs (the node velocities before the step, the state the step stored)
    import ref64
    kscale = side // mt.kstride
    wa = ref64.world_nodes(kk, gridA, side, kscale)
    r = ref64.g2p64((wa[0], wa[1][:, 1:4]), a[:, 1:4], dx, dt, F=a[:, 16:25] if model == 0 else None)
    out["ref64_particles"] = [ref64.check_particles(b[:, 1:4], r["x"], r["b_x"], "sub-box x"),
                              ref64.check_particles(b[:, 4:7], r["v"], r["b_v"], "sub-box v"),
                              ref64.check_particles(b[:, 7:16], r["C"], r["b_C"], "sub-box C")]
    if model == 0:
        out["ref64_particles"].append(ref64.check_particles(b[:, 16:25], r["F"], r["b_F"], "sub-box F"))
    del r
    ref = ref64.p2g64(b[:, 0], b[:, 1:4], b[:, 4:7], b[:, 7:16], dx, dt)
    wb = ref64.world_nodes(kk, gridB, side, kscale)
    inner = interior.ravel()
    rows = ref.lookup(wb[0][inner])
    assert (rows >= 0).all()
    out["ref64_grid"] = ref64.check_grid(ref.subset(rows), (wb[0][inner], wb[1][inner]), range(4), "sub-box interior nodes")[:4].tolist()
    return out


def test_config4_sand_64m_slotted_moving_subbox_vs_oracle(pol, oracle):
    """BASELINE config 4 at N = 1 anchored to the oracle: 64 Mi-particle DruckerPrager column falling at 0.05 cell per step on slotted
    storage; after 8 moving steps the 9th step's G2P + P2G of a 262 144-particle sub-box (32^3 cells in the middle of the column) ==
    oracle/mpm.c on exactly those particles with the GPU's node velocities as input.  Tolerances: x 1e-6, v / C 2e-4 of the channel
    maximum, F and logJp 2e-5, grid channels 2e-4 of the channel maximum (float atomics: summation order)."""
    r = _id_box_step(pol, oracle, 1, 512, (128, 512, 128), (0.0, -1.0, 0.0), (240, 256, 240), steps_before=8)
    assert r["movers_in_step"] > 1_000_000 and r["changed_cell_in_step"] > 1000, r   # the step under test moves particles between cells
    assert r["x"] <= 1e-6 and r["v"] <= 2e-4 and r["C"] <= 2e-4 and r["F"] <= 2e-5 and r["logJp"] <= 2e-5, r
    assert max(r["grid"]) <= 2e-4 and r["grid_mass_interior"] > 0, r
    assert max(r["ref64_grid"]) <= 1 and max(r["ref64_particles"]) <= 1, r   # (ref64's checks raise on their own; recorded in r)
    print("REF64 sub-box grid %s particles %s" % (r["ref64_grid"], r["ref64_particles"]))


def test_config3_jello_8m_slotted_moving_subbox_vs_oracle(pol, oracle):
    """BASELINE config 3 anchored to the oracle: the 8 M-particle FixedCorotated cube (256^3 grid) moving 0.013 cell per step; 8 slotted
    steps, then the 9th step of a 32^3-cell sub-box against oracle/mpm.c (tolerances as above)."""
    r = _id_box_step(pol, oracle, 0, 256, (100, 100, 100), (0.0, -0.5, 0.0), (112, 32, 112), steps_before=8)
    assert r["x"] <= 1e-6 and r["v"] <= 2e-4 and r["C"] <= 2e-4 and r["F"] <= 2e-5, r
    assert max(r["grid"]) <= 2e-4 and r["grid_mass_interior"] > 0, r
    assert max(r["ref64_grid"]) <= 1 and max(r["ref64_particles"]) <= 1, r   # (ref64's checks raise on their own; recorded in r)
    print("REF64 sub-box grid %s particles %s" % (r["ref64_grid"], r["ref64_particles"]))


# ------------------------------------------------------------------------------------------------ r04: conservation across re-partitions
def test_config4_sand_64m_480_steps_closed_loop_repartitions_lose_nobody():
    """The r03 soak lost 227 211 of the 67 108 864 particles over 3000 steps and 38 re-partitions without a word (a mover whose
    destination block was not in the partition was dropped, and every re-partition started a fresh status buffer).  480 steps of the
    accelerating column (30 cells of fall), re-partitioned whenever the slotted step's own status word asks for it: >= 3 re-partitions,
    particle count exact, mass sum exact to 1e-9, every mover re-homed, no flag in any period.  Reference semantics: every particle is
    written back, simulation/transfer/G2P.hpp:67-82."""
    a = _bench(["--steps", "480", "--warmup", "0", "--no-cpu-baseline", "--checksum", "--no-at-rest"])
    n = 67_108_864
    c = a["config"]
    rec = c["slot_record_rank0"]
    assert c["particles"] == n and a["hip_error"] == 0
    assert c["repartitions"] >= 3 and c["repartition_trigger"].startswith("closed loop"), (c["repartitions"], c["repartition_steps"])
    assert rec["particles_in_storage"] == n and rec["movers_sent"] == rec["movers_rehomed"] > 100_000_000, rec
    assert not any(rec["periods_with_flag"].values()) and rec["periods"] == c["repartitions"] + 1, rec
    assert rec["periods_with_edge_warning"] >= c["repartitions"], rec
    m = 1000.0 * (1.0 / 512) ** 3 / 8
    assert abs(a["checksum"][0] - n * np.float32(m)) <= 1e-9 * n * m


def test_config4_sand_64m_identities_survive_400_steps_and_repartitions(pol):
    """The same property particle by particle: the 262 144 particles of a 32^3-cell sub-box at the FOOT of the 64 Mi column (where the
    column leaves the partition first) carry pairwise different masses; after 400 closed-loop steps with >= 3 re-partitions the storage
    holds exactly those identities once each, and exactly n particles."""
    import bench
    import zpc_amd
    from zpc_amd.mpm import MpmTransfer
    grid_n, cells, model, side = 512, (128, 512, 128), 1, 8
    dx, dt = 1.0 / grid_n, 1e-4
    glo = [(grid_n - cells[0]) // 2 // side * side, 0, (grid_n - cells[2]) // 2 // side * side]
    ghi = [glo[d] + cells[d] for d in range(3)]
    dev = torch.device("cuda", 0)
    aos = bench.generate_particles(glo, ghi, dx, 1234, dev, model)
    aos[:, 5] += -1.0
    n = aos.shape[0]
    m0 = float(aos[0, 0].item())
    cell = torch.floor(aos[:, 1:4] / dx).to(torch.int32)
    box_lo = (glo[0], 0, glo[2])          # a corner of the column's foot
    inb = torch.ones(n, dtype=torch.bool, device=dev)
    for d in range(3):
        inb &= (cell[:, d] >= box_lo[d]) & (cell[:, d] < box_lo[d] + 32)
    ids = torch.nonzero(inb).flatten()
    nid = int(ids.numel())
    assert nid == 32 ** 3 * 8
    aos[:, 0] = 0.99 * m0
    want_ids = (m0 * (1.0 + torch.arange(nid, device=dev, dtype=torch.float64) * 2.0 ** -20)).float()
    aos[ids, 0] = want_ids
    del cell, inb
    vol = dx ** 3 / 8
    mt = MpmTransfer(pol, n, dx, dt, model=model, side=side, volume=vol, cache_stress=True)
    aos = torch.cat([aos, torch.zeros(n, mt.nchn - aos.shape[1], dtype=torch.float32, device=dev)], dim=1).contiguous()
    zpc_amd.lib().zs_rocm_tv_from_aos_f32(pol.handle, aos.data_ptr(), n, mt.nchn, mt.L, mt.buf.data_ptr())
    pol.syncCtx()
    del aos
    g = (0.0, -9.8, 0.0)

    def prime():
        mt.build_partition(max(4096, n // 128), margin=1)
        mt.rebin()
        mt.clear_grid()
        mt.p2g()
        mt.grid_update(g)
        mt.slot(K=24, outbox_cap=128)
    mt.build_partition(max(4096, n // 128), margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update(g)
    mt.slot(K=24, outbox_cap=128)
    reparts, pending = [], False
    for step in range(400):
        mt.g2p2g(write_all=pending)
        mt.grid_update(g)
        if pending:
            mt.unslot(strict=True)      # checks the period's flags, sent == re-homed, and the particle count
            prime()
            reparts.append(step)
            pending = False
        elif step % 2 == 1:
            pending = mt.poll_repartition()
    pol.syncCtx()
    mt.check_slots(strict=True)
    assert len(reparts) >= 3, reparts
    rec = mt.slot_record
    assert rec["sent"] == rec["homed"] > 100_000_000 and not any(rec["flags"][k] for k in (0, 1, 2, 4)), rec
    cbuf, cnt = mt._compact_copy()
    assert cnt == n
    m = cbuf.view(-1, mt.nchn, 64)[:, 0, :].reshape(-1)[:cnt]
    got = torch.sort(m[(m >= m0) & (m < 1.3 * m0)]).values
    assert got.numel() == nid and torch.equal(got, want_ids)
    assert int((m == np.float32(0.99 * m0)).sum()) == n - nid
