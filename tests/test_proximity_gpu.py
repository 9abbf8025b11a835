"""Mesh proximity pairs on the GPU (zpc_amd/csrc/mesh_proximity.hip, TriMesh.edges / TriMesh.proximity) against the float64 brute force of
tests/ref64_proximity.py: the edge list, membership and distances with per-pair bounds, features against the returned coordinates,
determinism, refit and the argument checks.  Prints one `PROX <what> ...` line per check.

The scenes (tests/ref64_proximity.py scene()), with the figures of the float64 brute force alone:
    sheets   288 vertices, 484 triangles, 770 edges; 1174 PT hits with all 7 features (fewest 83), 3391 EE hits with all 9 categories
             (fewest 71); no pair within the bound of dHat
    regular  768 PT and 2030 EE hits, 478 of the EE hits between exactly parallel edges
    torus    2736 PT and 7152 EE hits, none within the bound of dHat
    fan      387 PT hits, 48 of them at one vertex; 583 EE hits, up to 48 at one edge
    stack    40 separate triangles inside a ball smaller than dHat: 4680 PT and 7020 EE hits (all pairs of different triangles); owners
             with more than 32 hits and with fewer in the same wave, on both sides
    tiny     nt = 0, 1, 2: the trees without trunk nodes
    large    18432 vertices (the Morton-ordered path); the brute force for 512 sampled vertices and 512 sampled edges against everything.
             The hits of this scene are second-ring neighbours whose distances pile up towards dHat = h / 2, so the share of pairs within
             the bound of dHat depends on the sample: LARGE_SEED is the first seed from 0 for which the reference alone has at most 0.5 %
             on both sides (PT 0 of 134, EE 0 of 325; over the seeds 0 .. 39 the
             shares average 0.7 % and 0.9 %); the GPU result plays no part in it."""
import ctypes as C
import functools

import numpy as np
import pytest

import ref64_mesh as rm
import ref64_proximity as rp
from util import rng

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
GREY_SHARE = 0.005
LARGE_SEED = 0


@functools.lru_cache(maxsize=None)
def _reference(name):
    v, t, dhat = rp.scene(name)
    if name != "large":
        return rp.Reference(v, t, dhat)
    g = np.random.default_rng(LARGE_SEED)
    ne = len(rp.edges(t))
    sv, se = g.choice(len(v), 512, replace=False), g.choice(ne, 512, replace=False)
    R = rp.Reference(v, t, dhat, sv, se)
    R.sample_v, R.sample_e = sv, se
    return R


def _host(r):
    return {k: (None if getattr(r, k) is None else getattr(r, k).cpu().numpy()) for k in r.__slots__}


def _restrict(out, R):
    """the lists restricted to the pairs that contain a sampled primitive (the `large` scene)"""
    if not hasattr(R, "sample_v"):
        return out
    mp = np.isin(out["pt_pairs"][:, 0], R.sample_v)
    me = np.isin(out["ee_pairs"][:, 0], R.sample_e) | np.isin(out["ee_pairs"][:, 1], R.sample_e)
    return {k: (x[mp] if k.startswith("pt") else x[me]) for k, x in out.items()}


def _check_lists(name, out, R):
    """check 2 of a scene: membership up to the pairs within the bound of dHat, distances, order, exclusions; returns what it printed"""
    v, t, e = R.verts, R.tris.astype(np.int64), R.edges
    res = {}
    for which in ("pt", "ee"):
        pairs, dist2 = out[which + "_pairs"].astype(np.int64), out[which + "_dist2"]
        hits, sure, grey = R.split(which)
        got = set(map(tuple, pairs.tolist()))
        assert len(got) == len(pairs), "a pair is reported twice"
        if which == "pt":
            assert ((pairs[:, 0] >= 0) & (pairs[:, 0] < len(v)) & (pairs[:, 1] >= 0) & (pairs[:, 1] < len(t))).all()
            assert (t[pairs[:, 1]] != pairs[:, :1]).all(), "a triangle that contains the vertex"
            d, b = rp.pt_distance(v, t, pairs)[:2]
        else:
            assert ((pairs[:, 0] >= 0) & (pairs[:, 0] < pairs[:, 1]) & (pairs[:, 1] < len(e))).all()
            ei, ej = e[pairs[:, 0]], e[pairs[:, 1]]
            assert (ei[:, :, None] != ej[:, None, :]).all(), "edges that share a vertex"
            d, b = rp.ee_distance(v, e, pairs)[:2]
        ratio = np.abs(np.sqrt(dist2.astype(np.float64)) - d) / b
        missing, extra = sure - got, got - sure - grey
        print("PROX %s[%s]: %d reported, %d reference hits, %d within the bound of dHat (share %.2e), %d missing, %d extra, distance %.3f "
              "of the bound" % (which, name, len(got), len(hits), len(grey), len(grey) / max(len(hits), 1), len(missing), len(extra),
                                ratio.max() if len(ratio) else 0.0))
        assert len(grey) <= GREY_SHARE * len(hits)
        assert not missing and not extra
        assert (ratio <= 1).all() and np.isfinite(dist2).all()
        res[which] = len(got)
    return res


def _mesh(pol, name):
    from zpc_amd.mesh import TriMesh
    v, t, dhat = rp.scene(name)
    return TriMesh(pol, v, t), dhat


# ------------------------------------------------------------------------------------------------ 1: edges
@pytest.mark.parametrize("name", rp.SCENES + ("large", "degenerate"))
def test_edges_equal_the_reference_list_in_order(pol, name):
    from zpc_amd.mesh import TriMesh
    if name == "degenerate":      # repeated indices and repeated triangles, shuffled
        v, t = rm.icosphere(2, 0.31, (0.5, 0.47, 0.53))
        t = np.concatenate([t, [[0, 0, 0], [3, 4, 4], [7, 9, 7], [5, 5, 5]], t[10:14], t[20:22, [1, 2, 0]]]).astype(np.int32)
        t = t[rng(5).permutation(len(t))]
    else:
        v, t, _ = rp.scene(name)
    mesh = TriMesh(pol, v, t)
    want = rp.edges(t)
    got = mesh.edges().cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape and mesh.num_edges == len(want)
    assert np.array_equal(got, want)
    print("PROX edges[%s]: %d triangles, %d edges" % (name, len(t), len(want)))


# ------------------------------------------------------------------------------------------------ 2: membership and distance
@pytest.mark.parametrize("name", rp.SCENES + ("large",))
def test_pairs_and_distances_against_the_float64_brute_force(pol, name):
    mesh, dhat = _mesh(pol, name)
    R = _reference(name)
    out = _host(mesh.proximity(dhat))
    assert out["pt_pairs"].shape[1:] == (2,) and out["ee_pairs"].shape[1:] == (2,) and out["pt_bary"].shape[1:] == (3,) and out["ee_st"].shape[1:] == (2,)
    n = _check_lists(name, _restrict(out, R), R)
    if name == "tiny0":
        assert len(out["pt_pairs"]) == 0 and len(out["ee_pairs"]) == 0
    if name == "fan":      # more hits at one vertex / one edge than a per-leaf cache of 32 would hold
        assert np.bincount(out["pt_pairs"][:, 0]).max() >= 48 and np.bincount(out["ee_pairs"].ravel()).max() >= 48
    if name in ("sheets", "regular", "torus", "fan", "stack", "large"):
        assert n["pt"] > 100 and n["ee"] > 100


# ------------------------------------------------------------------------------------------------ 3: features
@pytest.mark.parametrize("name", ["sheets", "regular", "torus", "fan", "tiny2"])
def test_features_and_categories_name_where_the_coordinates_put_the_points(pol, name):
    mesh, dhat = _mesh(pol, name)
    R = _reference(name)
    out = _host(mesh.proximity(dhat))
    v, t, e = rp._v64(R.verts), R.tris.astype(np.int64), R.edges
    # PT: the barycentrics against the feature, and the point they give against the float64 distance
    pairs, feat, bary = out["pt_pairs"].astype(np.int64), out["pt_feature"], out["pt_bary"]
    assert ((feat >= 0) & (feat <= 6)).all() and np.isfinite(bary).all()
    on_vertex, on_edge = feat < 3, (feat >= 3) & (feat < 6)
    assert (bary[on_vertex].max(axis=1) == 1).all() and ((bary[on_edge] == 0).sum(axis=1) >= 1).all()
    for k in range(3):
        assert (bary[feat == k][:, k] == 1).all() and (bary[feat == 3 + k][:, (k + 2) % 3] == 0).all()
    d, b = rp.pt_distance(R.verts, t, pairs)[:2]
    cp = sum(bary[:, k, None].astype(np.float64) * v[t[pairs[:, 1], k]] for k in range(3))
    rcp = np.abs(np.linalg.norm(v[pairs[:, 0]] - cp, axis=1) - d) / b
    # EE: the category against (s, t), and the point pair they give
    ep, cat, st = out["ee_pairs"].astype(np.int64), out["ee_category"], out["ee_st"]
    s, tt = st[:, 0], st[:, 1]
    uc, vc = cat // 3, cat % 3
    assert ((cat >= 0) & (cat < 9)).all() and ((st >= 0) & (st <= 1)).all()
    assert np.array_equal(uc == 0, s == 0) and np.array_equal(uc == 1, s == 1) and np.array_equal(vc == 0, tt == 0) and np.array_equal(vc == 1, tt == 1)
    de, be = rp.ee_distance(R.verts, e, ep)[:2]
    a0, a1, b0, b1 = v[e[ep[:, 0], 0]], v[e[ep[:, 0], 1]], v[e[ep[:, 1], 0]], v[e[ep[:, 1], 1]]
    q = (a0 + s[:, None].astype(np.float64) * (a1 - a0)) - (b0 + tt[:, None].astype(np.float64) * (b1 - b0))
    rq = np.abs(np.linalg.norm(q, axis=1) - de) / be
    f32 = [x.astype(np.float32) for x in (a0, a1, b0, b1)]
    par = rp.ee_closest(*f32, parallel=rp.PARALLEL32)[4] if len(ep) else np.zeros(0, bool)
    print("PROX features[%s]: features %s, closest point %.3f of the bound; categories %s, point pair %.3f of the bound; %d of %d EE hits "
          "took the parallel branch" % (name, np.bincount(feat, minlength=7).tolist(), rcp.max(), np.bincount(cat, minlength=9).tolist(),
                                        rq.max(), par.sum(), len(ep)))
    assert (rcp <= 1).all() and (rq <= 1).all()
    if name == "sheets":
        assert (np.bincount(feat, minlength=7) > 0).all() and (np.bincount(cat, minlength=9) > 0).all()
    if name == "regular":
        assert par.sum() > 100


# ------------------------------------------------------------------------------------------------ 4: determinism
@pytest.mark.parametrize("name", ["sheets", "large"])
def test_two_calls_give_the_same_bytes(pol, name):
    mesh, dhat = _mesh(pol, name)
    a, b = _host(mesh.proximity(dhat)), _host(mesh.proximity(dhat))
    other, _ = _mesh(pol, name)
    c = _host(other.proximity(dhat))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() and a[k].tobytes() == c[k].tobytes(), k
    assert len(a["pt_pairs"]) and len(a["ee_pairs"])


def _fill_by_hand(pol, mesh, dhat, side, stale):
    """count -> scan -> fill through the C ABI; stale: a count pass with another dHat in between, after which the fill pass finds the hit
    cache of the count pass taken over and walks the tree for every owner"""
    from zpc_amd import lib
    L = lib()
    count, fill = getattr(L, "zs_rocm_mesh_proximity_%s_count" % side), getattr(L, "zs_rocm_mesh_proximity_%s_fill" % side)
    n = mesh.nv if side == "pt" else mesh.num_edges
    cnt = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    assert count(pol.handle, mesh.handle, dhat, cnt.data_ptr()) == 0
    if stale:
        other = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        assert count(pol.handle, mesh.handle, 0.5 * dhat, other.data_ptr()) == 0
    off = torch.cumsum(cnt, 0, dtype=torch.int32) - cnt
    pol.syncCtx()
    total = int(off[-1].item())
    w = 3 if side == "pt" else 2
    out = [torch.empty(total, 2, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.float32, device="cuda"),
           torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, w, dtype=torch.float32, device="cuda")]
    assert fill(pol.handle, mesh.handle, dhat, off.data_ptr(), *[x.data_ptr() for x in out]) == 0
    pol.syncCtx()
    return [x.cpu().numpy() for x in out], int(cnt.max().item())


@pytest.mark.parametrize("name", ["sheets", "fan", "stack", "large"])
def test_the_fill_pass_gives_the_same_bytes_from_the_hit_cache_and_from_the_walk(pol, name):
    mesh, dhat = _mesh(pol, name)
    ref = _host(mesh.proximity(dhat))
    for side, keys in (("pt", ("pt_pairs", "pt_dist2", "pt_feature", "pt_bary")), ("ee", ("ee_pairs", "ee_dist2", "ee_category", "ee_st"))):
        for stale in (False, True):
            out, most = _fill_by_hand(pol, mesh, dhat, side, stale)
            for k, x in zip(keys, out):
                assert x.tobytes() == ref[k].tobytes(), (k, stale)
        print("PROX fill[%s, %s]: %d pairs, at most %d at one owner; cached and walked fill passes agree" % (name, side, len(out[0]), most))
        if (name == "fan" and side == "pt") or name == "stack":
            assert most > 32       # an owner whose hits do not fit the cache walks again in the cached pass as well


# ------------------------------------------------------------------------------------------------ 5: refit
def test_refit_moves_the_edge_tree_with_the_mesh(pol):
    mesh, dhat = _mesh(pol, "sheets")
    v, t, _ = rp.scene("sheets")
    before = _host(mesh.proximity(dhat))       # builds the edge tree, which refit has to follow
    moved = v.copy()
    moved[len(v) // 2:, 2] -= np.float32(0.01)
    mesh.refit(moved)
    after = _host(mesh.proximity(dhat))
    n = _check_lists("sheets, upper sheet 0.01 lower", after, rp.Reference(moved, t, dhat))
    assert n["pt"] != len(before["pt_pairs"]) and n["ee"] != len(before["ee_pairs"])
    assert after["pt_dist2"].tobytes() != before["pt_dist2"].tobytes() and after["ee_dist2"].tobytes() != before["ee_dist2"].tobytes()
    from zpc_amd.mesh import TriMesh
    fresh = _host(TriMesh(pol, moved, t).proximity(dhat))
    assert set(map(tuple, fresh["pt_pairs"].tolist())) == set(map(tuple, after["pt_pairs"].tolist()))
    assert set(map(tuple, fresh["ee_pairs"].tolist())) == set(map(tuple, after["ee_pairs"].tolist()))


# ------------------------------------------------------------------------------------------------ 6: arguments
def test_arguments(pol):
    from zpc_amd import lib
    from zpc_amd.mesh import EE_CATEGORIES, FEATURES
    assert len(EE_CATEGORIES) == 9 and len(FEATURES) == 7
    mesh, dhat = _mesh(pol, "sheets")
    for bad in (0.0, -0.01, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            mesh.proximity(bad)
    L = lib()
    counts = torch.full((mesh.nv,), 7, dtype=torch.int32, device="cuda")
    for bad in (0.0, -0.01, float("inf"), float("nan")):
        assert L.zs_rocm_mesh_proximity_pt_count(pol.handle, mesh.handle, bad, counts.data_ptr()) == -1
        assert L.zs_rocm_mesh_proximity_ee_count(pol.handle, mesh.handle, bad, counts.data_ptr()) == -1
    assert L.zs_rocm_mesh_proximity_pt_count(pol.handle, None, dhat, counts.data_ptr()) == -1
    assert L.zs_rocm_mesh_proximity_ee_fill(pol.handle, None, dhat, counts.data_ptr(), None, None, None, None) == -1
    pol.syncCtx()
    assert (counts == 7).all()
    r = mesh.proximity(dhat, ee=False)
    assert r.ee_pairs is None and r.ee_dist2 is None and r.ee_category is None and r.ee_st is None and len(r.pt_pairs) == 1174
    assert L.zs_rocm_mesh_num_edges(mesh.handle) == 770 and L.zs_rocm_mesh_num_edges(None) == 0
    r = mesh.proximity(dhat, pt=False)
    assert r.pt_pairs is None and r.pt_dist2 is None and r.pt_feature is None and r.pt_bary is None and len(r.ee_pairs) == 3391
    # the optional outputs of the fill passes may be NULL
    full = _host(mesh.proximity(dhat))
    cnt = torch.zeros(mesh.nv + 1, dtype=torch.int32, device="cuda")
    assert L.zs_rocm_mesh_proximity_pt_count(pol.handle, mesh.handle, dhat, cnt.data_ptr()) == 0
    off = torch.cumsum(cnt, 0, dtype=torch.int32) - cnt
    pairs = torch.empty(len(full["pt_pairs"]), 2, dtype=torch.int32, device="cuda")
    d2 = torch.empty(len(full["pt_pairs"]), dtype=torch.float32, device="cuda")
    assert L.zs_rocm_mesh_proximity_pt_fill(pol.handle, mesh.handle, dhat, off.data_ptr(), pairs.data_ptr(), d2.data_ptr(), None, None) == 0
    pol.syncCtx()
    assert np.array_equal(pairs.cpu().numpy(), full["pt_pairs"]) and d2.cpu().numpy().tobytes() == full["pt_dist2"].tobytes()
