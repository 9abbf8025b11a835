"""Times the mesh proximity passes (TriMesh.proximity: zs_rocm_mesh_proximity_{pt,ee}_{count,fill}) next to the route a user had before
them, on two scenes:

    surface   the jittered 980 k-triangle surface of tools/bench_mesh_levelset.py (--side 700), dHat = half the mean edge
    sheets    two jittered sheets of about 1 M triangles each (--sheet 708), a gap of h / 2, dHat = h (h = the grid spacing)

Rows per scene:
    (a) edges_and_tree   TriMesh(...) without and with the first edge-edge call: edge extraction is part of the mesh build, the edge tree
                         (edge boxes + LBvh build) of the first EE query; host wall time around synchronising calls
    (b) pt               PT count + fill
    (c) ee               EE count + fill
    (d) boxes_pt / _ee   zs_rocm_lbvh_query_count + _fill with the vertex boxes dilated by dHat on the triangle tree, and
                         zs_rocm_lbvh_self_query_count + _fill on a tree over the edge boxes dilated by dHat / 2 (the self-query tests leaf
                         box against leaf box, so half the distance on either side gives the same candidates): every box overlap is
                         written, none is tested
(b), (c), (d) are bracketed by HIP events on the policy's stream with the policy not synchronising, offsets from one earlier pass (the scan
and the read-back of the total are the same on both routes and not timed), alternated b, d, c, d in every repeat of the same process.
Also: hits, leaf tests (= box overlaps) per primitive, output bytes against the candidate list's.

    python tools/bench_proximity.py [--side 700] [--sheet 708] [--reps 10] [--warmup 2] [--out profiles/mesh_proximity.json]
prints one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zpc_amd as zs  # noqa: E402
from zpc_amd.mesh import TriMesh  # noqa: E402
from zpc_amd.containers import LBvh  # noqa: E402
from zpc_amd.primitives import exclusive_scan  # noqa: E402
from bench_mesh_levelset import jittered_surface  # noqa: E402


def sheet(n, z, seed):
    g = np.random.default_rng(seed)
    h = 0.6 / (n - 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([0.2 + h * i, 0.2 + h * j, np.full(i.shape, float(z))], axis=-1).reshape(-1, 3) + 0.6 * h * (g.random((n * n, 3)) - 0.5)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).ravel()
    t = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)])
    return v.astype(np.float32), t.astype(np.int32)


def two_sheets(n):
    h = 0.6 / (n - 1)
    v0, t0 = sheet(n, 0.5, 1)
    v1, t1 = sheet(n, 0.5 + 0.5 * h, 2)
    return np.concatenate([v0, v1]), np.concatenate([t0, t1 + len(v0)]), h


def stats(ms):
    a = np.asarray(ms)
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), reps=len(ms))


def scan(pol, counts):
    offsets = torch.empty_like(counts)
    exclusive_scan(pol, counts, offsets)
    pol.syncCtx()
    return offsets, int(offsets[-1].item())


def run_scene(pol, name, v, t, dhat, reps, warmup):
    L = zs.lib()
    H = pol.handle
    t0 = time.perf_counter()
    mesh = TriMesh(pol, v, t)
    pol.syncCtx()
    build_ms = 1e3 * (time.perf_counter() - t0)
    nv, ne = mesh.nv, mesh.num_edges
    # ---- one pass of everything: offsets, totals, outputs
    cp = torch.zeros(nv + 1, dtype=torch.int32, device="cuda")
    ce = torch.zeros(ne + 1, dtype=torch.int32, device="cuda")
    assert L.zs_rocm_mesh_proximity_pt_count(H, mesh.handle, dhat, cp.data_ptr()) == 0
    pol.syncCtx()
    t0 = time.perf_counter()
    assert L.zs_rocm_mesh_proximity_ee_count(H, mesh.handle, dhat, ce.data_ptr()) == 0     # builds the edge tree
    pol.syncCtx()
    first_ee_ms = 1e3 * (time.perf_counter() - t0)
    op, npt = scan(pol, cp)
    oe, nee = scan(pol, ce)
    f32, i32 = torch.float32, torch.int32
    pt_out = [torch.empty(npt, 2, dtype=i32, device="cuda"), torch.empty(npt, dtype=f32, device="cuda"), torch.empty(npt, dtype=i32, device="cuda"),
              torch.empty(npt, 3, dtype=f32, device="cuda")]
    ee_out = [torch.empty(nee, 2, dtype=i32, device="cuda"), torch.empty(nee, dtype=f32, device="cuda"), torch.empty(nee, dtype=i32, device="cuda"),
              torch.empty(nee, 2, dtype=f32, device="cuda")]
    # ---- the route without the fused passes: box overlaps only
    vd = torch.from_numpy(v).cuda()
    qb = torch.cat([vd - dhat, vd + dhat], dim=1).contiguous()
    tri_tree = LBvh()
    vt = vd[torch.from_numpy(t.astype(np.int64)).cuda()]
    tri_tree.build(pol, torch.cat([vt.min(dim=1).values, vt.max(dim=1).values], dim=1).contiguous())
    e = mesh.edges().long()
    ev = vd[e]
    edge_tree = LBvh()
    edge_tree.build(pol, torch.cat([ev.min(dim=1).values - 0.5 * dhat, ev.max(dim=1).values + 0.5 * dhat], dim=1).contiguous())
    bp = torch.zeros(nv + 1, dtype=torch.int32, device="cuda")
    be = torch.zeros(ne + 1, dtype=torch.int32, device="cuda")
    L.zs_rocm_lbvh_query_count(H, tri_tree.handle, qb.data_ptr(), nv, bp.data_ptr())
    L.zs_rocm_lbvh_self_query_count(H, edge_tree.handle, be.data_ptr())
    obp, nbp = scan(pol, bp)
    obe, nbe = scan(pol, be)
    box_pt = torch.empty(max(nbp, 1), dtype=i32, device="cuda")
    box_ee = torch.empty(max(nbe, 1) * 2, dtype=i32, device="cuda")

    def pt():
        L.zs_rocm_mesh_proximity_pt_count(H, mesh.handle, dhat, cp.data_ptr())
        L.zs_rocm_mesh_proximity_pt_fill(H, mesh.handle, dhat, op.data_ptr(), *[x.data_ptr() for x in pt_out])

    def ee():
        L.zs_rocm_mesh_proximity_ee_count(H, mesh.handle, dhat, ce.data_ptr())
        L.zs_rocm_mesh_proximity_ee_fill(H, mesh.handle, dhat, oe.data_ptr(), *[x.data_ptr() for x in ee_out])

    def boxes_pt():
        L.zs_rocm_lbvh_query_count(H, tri_tree.handle, qb.data_ptr(), nv, bp.data_ptr())
        L.zs_rocm_lbvh_query_fill(H, tri_tree.handle, qb.data_ptr(), nv, obp.data_ptr(), box_pt.data_ptr())

    def boxes_ee():
        L.zs_rocm_lbvh_self_query_count(H, edge_tree.handle, be.data_ptr())
        L.zs_rocm_lbvh_self_query_fill(H, edge_tree.handle, obe.data_ptr(), box_ee.data_ptr())

    rows = dict(pt=pt, boxes_pt=boxes_pt, ee=ee, boxes_ee=boxes_ee)
    ms = {k: [] for k in rows}
    stream = torch.cuda.ExternalStream(pol.getStream()) if pol.getStream() else torch.cuda.default_stream()
    pol.sync(False)
    for it in range(warmup + reps):
        for k, fn in rows.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if it >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    pol.sync(True)
    pol.syncCtx()
    assert zs.lib().zs_rocm_last_error(-1) == 0
    return dict(scene=name, vertices=nv, triangles=mesh.nt, edges=ne, dhat=dhat,
                edges_and_tree=dict(mesh_build_with_edges_ms=build_ms, first_ee_count_with_tree_build_ms=first_ee_ms),
                times={k: stats(x) for k, x in ms.items()},
                pt=dict(hits=npt, leaf_tests_per_vertex=nbp / max(nv, 1), output_bytes=28 * npt, candidate_list_bytes=4 * nbp),
                ee=dict(hits=nee, leaf_tests_per_edge=nbe / max(ne, 1), output_bytes=24 * nee, candidate_list_bytes=8 * nbe))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--sheet", type=int, default=708)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    pol = zs.rocm_exec()
    out = []
    v, t = jittered_surface(a.side)
    p = v[t.astype(np.int64)].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
    out.append(run_scene(pol, "surface", v, t, float(np.float32(0.5 * mean_edge)), a.reps, a.warmup))
    v, t, h = two_sheets(a.sheet)
    out.append(run_scene(pol, "sheets", v, t, float(np.float32(h)), a.reps, a.warmup))
    doc = json.dumps(dict(bench="mesh_proximity", device=torch.cuda.get_device_name(0), scenes=out), indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
