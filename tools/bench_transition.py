"""Times the boundary pass with a keyframed level-set collider (zs_rocm_mpm_apply_boundary_transition) on the partition of bench.py's
default workload -- the 64 Mi-particle sand column, 8^3 blocks, dx = 1/512 -- next to the single-level-set pass
(zs_rocm_mpm_apply_boundary_levelset) on the same grid, in the same process:

    levelset_floor / levelset_sphere       tools/bench_levelset.py's rows: the yardstick
    transition_floor / transition_sphere   two keyframes of the same slab / sphere one voxel apart, "v" = the displacement / stepDt,
                                           alpha = 0.5
    transition_culled                      two keyframes of a sphere far from every grid block

Every launch is bracketed by HIP events; after a warm-up the mean, median, p10 / p90 of --reps launches are reported with the share of
grid blocks culled / staged / direct and the staged ones whose "v" boxes were read directly (one more launch with the counters set;
the timed launches run without them).  One JSON line.

    python tools/bench_transition.py [--reps 30] [--warmup 5] [--cells 128,512,128] [--grid 512]
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
from zpc_amd.levelset import SparseLevelSet, LevelSetSequence  # noqa: E402
from zpc_amd.mpm import MpmTransfer, make_levelset_collider, SEPARATE  # noqa: E402
from bench import generate_particles  # noqa: E402
from bench_levelset import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--cells", type=str, default="128,512,128")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
    aos[:, 5] -= 1.0
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
    radius, pad, band = 40 * dx, 10 * dx, 6 * dx
    step_dt = 100 * dt                         # a keyframe every 100 sub-steps
    up = np.array([0.0, dx, 0.0])              # one voxel per keyframe
    vel = lambda x: np.broadcast_to(up / step_dt, x.shape)
    flo, fhi = (lo[0] * dx - pad, -16 * dx, lo[2] * dx - pad), (hi[0] * dx + pad, 24 * dx, hi[2] * dx + pad)
    far = centre + np.array([0.0, -3.0, 0.0])

    def floor(k, v):
        return SparseLevelSet.from_function(pol, lambda x: x[..., 1] - (1.5 * dx + k * dx), flo, fhi, dx, band, vel_fn=vel if v else None)

    def sphere(c, k, v):
        return SparseLevelSet.from_function(pol, lambda x: np.linalg.norm(x - (c + k * up), axis=-1) - radius, tuple(c - radius - pad),
                                            tuple(c + radius + pad), dx, band, vel_fn=vel if v else None)

    def sequence(frames):
        seq = LevelSetSequence(pol, step_dt)
        for f in frames:
            seq.push(f)
        seq.advance(0.5)
        return seq

    col = make_levelset_collider(SEPARATE)
    rows = {"levelset_floor": floor(0, False), "levelset_sphere": sphere(centre, 0, False),
            "transition_floor": sequence([floor(0, True), floor(1, True)]),
            "transition_sphere": sequence([sphere(centre, 0, True), sphere(centre, 1, True)]),
            "transition_culled": sequence([sphere(far, 0, True), sphere(far, 1, True)])}
    res = dict(n=n, nblocks=nb, side=side, dx=dx, step_dt=step_dt, alpha=0.5)
    saved = mt.grid.clone()
    for name, ls in rows.items():
        mt.grid.copy_(saved)
        fn = lambda: mt.apply_boundary(col, levelset=ls)
        fn()
        pol.syncCtx()
        changed = int((mt.grid != saved).sum().item())
        r = timed(pol, fn, a.reps, a.warmup)
        r["values_changed_by_first_launch"] = changed
        ls.enable_stats()
        fn()
        s = ls.read_stats()
        r.update(culled=float(s[0]) / nb, staged=float(s[1]) / nb, direct=float(s[2]) / nb, v_direct=float(s[3]) / nb)
        if isinstance(ls, LevelSetSequence):
            v = ls.view()
            r.update(max_speed=float(v.maxSpeed), widen_cells=int(np.ceil(v.stepDt * max(v.alpha, 1 - v.alpha) * v.maxSpeed / v.src.h)) + 1)
        res[name] = r
    assert zs.lib().zs_rocm_last_error(-1) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
