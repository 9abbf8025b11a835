"""Times the mesh -> sparse level set conversion (SparseLevelSet.from_mesh) next to its comparator, the per-lane bulk query
zs_rocm_mesh_signed_distance, and the mesh build (block_kernel_vs_comparator: zs_rocm_mesh_levelset_blocks alone against that query on the
cell centres of the same candidate blocks; per_lane_on_kept_cells: the query on the kept blocks' cells only), on

    icosphere   radius 0.3, --level subdivisions (9: 5.2 M, 8: 1.3 M triangles), voxel = 1 / grid, band = 3 voxels
    jittered    a config-5-style surface: a height field of --side^2 x 2 triangles with jittered vertices (an open sheet: allow_open)
    floor       the bench column's floor as a slab mesh (12 triangles)
    sphere      the sphere under the column's foot as an icosphere of level 4 (5120 triangles)

mesh_build, from_mesh and per_lane_on_kept_cells are host wall time around synchronising calls (from_mesh sizes containers on the host in
between, so the whole call is what a user pays; launch and synchronise overhead, some tens of microseconds per call, is part of it).
block_kernel_vs_comparator is bracketed by HIP events on the policy's stream: device time of the launches alone.  Median / p10 / p90 of
--reps after --warmup; blocks kept, the share of candidate blocks rejected / staged / per-lane.  One JSON line.

    python tools/bench_mesh_levelset.py [--grid 512] [--level 8] [--side 700] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zpc_amd as zs  # noqa: E402
from zpc_amd.mesh import TriMesh  # noqa: E402
from zpc_amd.levelset import SparseLevelSet  # noqa: E402


def timed(pol, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        pol.syncCtx()
        t0 = time.perf_counter()
        fn()
        pol.syncCtx()
        ms.append(1e3 * (time.perf_counter() - t0))
    a = np.asarray(ms)
    return dict(median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), reps=reps)


def timed_events(pol, fn, reps, warmup):
    stream = torch.cuda.ExternalStream(pol.getStream()) if pol.getStream() else torch.cuda.default_stream()
    for _ in range(warmup):
        fn()
    pol.syncCtx()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    a = np.asarray(ms)
    return dict(median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), reps=reps)


def box_mesh(lo, hi):
    """12 triangles, outward orientation"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (i >> d) & 1 else lo)[d] for d in range(3)] for i in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = np.array([x for a, b, c, d in quads for x in ((a, b, c), (a, c, d))], np.int32)
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    flip = (n * (v[t].mean(1) - 0.5 * (lo + hi))).sum(1) < 0
    t[flip] = t[flip][:, [0, 2, 1]]
    return v.astype(np.float32), t


def icosphere(level, radius, centre):
    """20 x 4^level triangles on the sphere, outward orientation"""
    g = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
                  (-g, 0, 1)], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int64)
    for _ in range(level):   # one midpoint per edge, found by sorting the edge keys
        e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
        key = e[:, 0] * len(v) + e[:, 1]
        uniq, inv = np.unique(key, return_inverse=True)
        mid = v[uniq // len(v)] + v[uniq % len(v)]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)          # midpoints of ab, bc, ca per triangle
        v = np.concatenate([v, mid])
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        t = np.concatenate([np.stack([a, m[0], m[2]], 1), np.stack([b, m[1], m[0]], 1), np.stack([c, m[2], m[1]], 1), np.stack([m[0], m[1], m[2]], 1)])
    return (v * radius + np.asarray(centre, np.float64)).astype(np.float32), t.astype(np.int32)


def kernel_rows(pol, mesh, ls, voxel, band, reps, warmup):
    """the block kernel alone (zs_rocm_mesh_levelset_blocks over all candidate blocks) and the comparator on the same cells: the bulk
    per-lane query at the cell centres of the same candidate blocks, same cap"""
    import ctypes as C
    from zpc_amd.containers import Bht
    from zpc_amd.mesh import candidate_capacity
    L = zs.lib()
    org = (C.c_float * 3)(*ls.origin)
    pairs = L.zs_rocm_mesh_levelset_count(pol.handle, mesh.handle, org, voxel, band)
    lo, hi = mesh.total_box()
    cand = Bht(3, candidate_capacity(pairs, lo, hi, ls.origin, voxel, band), bucket=16)
    assert L.zs_rocm_mesh_levelset_candidates(pol.handle, mesh.handle, org, voxel, band, cand.handle) == 0
    pol.syncCtx()
    ncand = cand.size()
    scratch = torch.empty(ncand * 512, dtype=torch.float32, device="cuda")
    keep = torch.zeros(ncand, dtype=torch.int32, device="cuda")
    blocks = timed_events(pol, lambda: L.zs_rocm_mesh_levelset_blocks(pol.handle, mesh.handle, org, voxel, band, cand.handle, ncand, scratch.data_ptr(), 1,
                                                               keep.data_ptr(), None), reps, warmup)
    keys = np.empty((ncand, 3), np.int32)
    C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(keys.ctypes.data), C.c_void_p(cand.view().activeKeys), C.c_size_t(keys.nbytes), 2)
    cc = torch.stack(torch.meshgrid(*[torch.arange(8, device="cuda")] * 3, indexing="ij"), -1).reshape(-1, 3)
    idx = (torch.from_numpy(keys).cuda()[:, None, :] + cc[None]).reshape(-1, 3).to(torch.float32)
    pts = (torch.tensor(ls.origin, device="cuda", dtype=torch.float32) + np.float32(voxel) * idx).contiguous()
    sdf = torch.empty(pts.shape[0], dtype=torch.float32, device="cuda")
    cap = float(np.float32(band + 7 * 3 ** 0.5 * voxel))
    comp = timed_events(pol, lambda: L.zs_rocm_mesh_signed_distance(pol.handle, mesh.handle, pts.data_ptr(), pts.shape[0], cap, sdf.data_ptr(), None),
                 reps, warmup)
    return dict(candidate_blocks=int(ncand), cells=int(pts.shape[0]), block_kernel=blocks, per_lane_comparator=comp)


def jittered_surface(side, seed=0):
    g = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(side + 1), np.arange(side + 1), indexing="ij")
    x = (i + 0.3 * (g.random(i.shape) - 0.5)) / side * 0.8 + 0.1
    z = (j + 0.3 * (g.random(i.shape) - 0.5)) / side * 0.8 + 0.1
    y = 0.5 + 0.05 * np.sin(7 * x) * np.cos(5 * z) + 0.2 / side * (g.random(i.shape) - 0.5)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda a, b: a * (side + 1) + b
    a, b, c, d = idx(i[:-1, :-1], j[:-1, :-1]), idx(i[1:, :-1], j[1:, :-1]), idx(i[1:, 1:], j[1:, 1:]), idx(i[:-1, 1:], j[:-1, 1:])
    t = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([a, d, c], -1).reshape(-1, 3)]).astype(np.int32)
    return v, t   # open: an upward-facing sheet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", type=str, default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    pol = zs.rocm_exec()
    voxel = 1.0 / a.grid
    band = 3 * voxel
    dx = voxel
    shapes = {
        "icosphere": lambda: icosphere(a.level, 0.3, (0.5, 0.5, 0.5)),
        "jittered": lambda: jittered_surface(a.side),
        "floor": lambda: box_mesh((-0.05, -0.2, -0.05), (1.05, 1.5 * dx, 1.05)),
        "sphere": lambda: icosphere(4, 0.12, (0.5, 0.05, 0.5)),
    }
    out = {}
    for name, make in shapes.items():
        if a.only and name != a.only:
            continue
        v, t = make()
        dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        row = dict(triangles=int(len(t)))
        row["mesh_build"] = timed(pol, lambda: TriMesh(pol, dv, dt), max(a.reps // 2, 1), 1)
        mesh = TriMesh(pol, dv, dt)
        row["mesh_stats"] = mesh.stats()
        open_ok = not mesh.is_closed()
        holder = {}

        def build():
            holder["ls"] = SparseLevelSet.from_mesh(pol, mesh, voxel, band, allow_open=open_ok)
        row["from_mesh"] = timed(pol, build, a.reps, a.warmup)
        ls = holder["ls"]
        st = ls.build_stats
        cand = max(int(st[:3].sum()), 1)
        row.update(blocks=int(ls.nblocks), candidates=cand, rejected_share=float(st[0] / cand), staged_share=float(st[1] / cand),
                   per_lane_share=float(st[2] / cand))
        # the comparator: the per-lane walk on the cell centres of the kept blocks (the same cells, without the candidate stage)
        keys = torch.from_numpy(ls.keys).cuda()
        cc = torch.stack(torch.meshgrid(*[torch.arange(8, device="cuda")] * 3, indexing="ij"), -1).reshape(-1, 3)
        idx = (keys[:, None, :] + cc[None]).reshape(-1, 3).to(torch.float32)
        pts = (torch.tensor(ls.origin, device="cuda", dtype=torch.float32) + np.float32(voxel) * idx).contiguous()
        cap = band + 7 * 3 ** 0.5 * voxel
        row["per_lane_on_kept_cells"] = timed(pol, lambda: mesh.signed_distance(pts, cap=cap, allow_open=True), a.reps, a.warmup)
        row["cells"] = int(pts.shape[0])
        row["block_kernel_vs_comparator"] = kernel_rows(pol, mesh, ls, voxel, band, a.reps, a.warmup)
        out[name] = row
    print(json.dumps(dict(grid=a.grid, voxel=voxel, band=band, rows=out)))


if __name__ == "__main__":
    main()
