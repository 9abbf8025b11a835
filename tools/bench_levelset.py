"""Times the level-set boundary pass (zs_rocm_mpm_apply_boundary_levelset) on the partition of bench.py's default workload -- the
64 Mi-particle sand column, 8^3 blocks, dx = 1/512 -- next to the analytic colliders' zs_rocm_mpm_apply_boundary on the same grid:

    analytic plane    the bench's own floor (y = 1.5 dx, separate)
    analytic sphere   a sphere under the column's foot
    level-set floor   the same floor as a slab sampled at h = dx
    level-set sphere  the same sphere sampled at h = dx, band of 6 cells

Every launch is bracketed by HIP events; after a warm-up the median, p10 / p90, min and max of --reps launches are reported together with
the share of grid blocks the level-set kernel culled / evaluated from the staged footprint / evaluated through the direct fallback
(counted in one more launch with zs_rocm_levelset::stats set; the timed launches run without it).  One JSON line.  --analytic-only: just the first two rows (a build without level sets).  --only ROW --reps 1 --warmup 0: one launch of one row,
for a counters-only profiler run.

    python tools/bench_levelset.py [--reps 30] [--warmup 5] [--cells 128,512,128] [--grid 512]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zpc_amd as zs  # noqa: E402
from zpc_amd.mpm import MpmTransfer, make_collider, PLANE, SPHERE, SEPARATE  # noqa: E402
from bench import generate_particles  # noqa: E402


def timed(pol, fn, reps, warmup):
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
    return dict(mean_ms=float(a.mean()), median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), min_ms=float(a.min()),
                max_ms=float(a.max()), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--cells", type=str, default="128,512,128")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--analytic-only", action="store_true")
    ap.add_argument("--only", type=str, default="", help="one row: analytic_plane | analytic_sphere | levelset_floor | levelset_sphere")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    pol = zs.rocm_exec()
    pol.sync(False)
    side, dx, dt = 8, 1.0 / a.grid, 1e-4
    ext = [int(x) for x in a.cells.split(",")]
    lo = [(a.grid - ext[0]) // 2 // side * side, 0, (a.grid - ext[2]) // 2 // side * side]
    hi = [lo[d] + ext[d] for d in range(3)]
    aos = generate_particles(lo, hi, dx, 1234, device, 1)
    aos[:, 5] -= 1.0   # the default column's fall speed
    n = aos.shape[0]
    mt = MpmTransfer(pol, n, dx, dt, model=1, side=side, volume=dx ** 3 / 8, device=device, cache_stress=True)
    aos = torch.cat([aos, torch.zeros(n, mt.nchn - aos.shape[1], dtype=torch.float32, device=device)], dim=1).contiguous()
    zs.lib().zs_rocm_tv_from_aos_f32(pol.handle, aos.data_ptr(), n, mt.nchn, mt.L, mt.buf.data_ptr())
    torch.cuda.synchronize()
    del aos
    nb = mt.build_partition(max(4096, n // 128), margin=1)
    mt.rebin()
    mt.update_stress()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    pol.syncCtx()
    centre = np.array([(lo[0] + hi[0]) / 2 * dx, -8 * dx, (lo[2] + hi[2]) / 2 * dx])
    radius = 40 * dx
    res = dict(n=n, nblocks=nb, side=side, dx=dx, grid_bytes=int(mt.grid.numel() * 4))
    rows = {"analytic_plane": (make_collider(PLANE, SEPARATE, [0.0, 1.5 * dx, 0.0, 0.0, 1.0, 0.0]), None),
            "analytic_sphere": (make_collider(SPHERE, SEPARATE, list(centre) + [radius]), None)}
    if not a.analytic_only:
        from zpc_amd.levelset import SparseLevelSet
        from zpc_amd.mpm import make_levelset_collider
        col = make_levelset_collider(SEPARATE)
        pad = 8 * dx
        flo, fhi = (lo[0] * dx - pad, -16 * dx, lo[2] * dx - pad), (hi[0] * dx + pad, 24 * dx, hi[2] * dx + pad)
        rows["levelset_floor"] = (col, SparseLevelSet.from_function(pol, lambda x: x[..., 1] - 1.5 * dx, flo, fhi, dx, 6 * dx))
        rows["levelset_sphere"] = (col, SparseLevelSet.from_function(pol, lambda x: np.linalg.norm(x - centre, axis=-1) - radius,
                                                                     tuple(centre - radius - pad), tuple(centre + radius + pad), dx, 6 * dx))
    saved = mt.grid.clone()
    for name, (col, ls) in rows.items():
        if a.only and name != a.only:
            continue
        mt.grid.copy_(saved)
        if ls is not None:   # (timed without the block counters: 27 k atomics on one word cost more than the pass itself)
            fn = lambda: mt.apply_boundary(col, levelset=ls)
        else:
            fn = lambda: mt.apply_boundary(col)
        fn()
        pol.syncCtx()
        changed = int((mt.grid != saved).sum().item())
        r = timed(pol, fn, a.reps, a.warmup)
        r["values_changed_by_first_launch"] = changed
        if ls is not None:
            ls.enable_stats()
            fn()
            s = ls.read_stats()
            r.update(level_set_blocks=int(ls.nblocks), culled=float(s[0]) / nb, staged=float(s[1]) / nb, fallback=float(s[2]) / nb)
        res[name] = r
    assert zs.lib().zs_rocm_last_error(-1) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
