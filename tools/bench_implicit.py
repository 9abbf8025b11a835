"""Times zs_rocm_mpm_implicit_force (the reference's G2P2GTransfer) on BASELINE config 3 -- 8 M-particle jello, dx = 1/256, 8 per
cell, 8^3 blocks, FixedCorotated -- against what the library already offers on the same particles in the same process:

    implicit_force binned        the operator's hot path
    g2p + p2g (unfused, binned)  the reference-order pair without a stress cache: the same gather plus v, the same single
                                 constitutive update, 7 scatter channels instead of 3 and 96 B of particle stores on top
    implicit_force particle      the reference's own algorithm (hash query + global float atomics per node)

Every launch is bracketed by HIP events on the policy's stream; after a warm-up the median and the p10 / p90 of --reps launches are
reported, one JSON line.

    python tools/bench_implicit.py [--cells 100] [--reps 30] [--warmup 5] [--model 0]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zpc_amd as zs  # noqa: E402
from zpc_amd.mpm import MpmTransfer  # noqa: E402


def make_particles(mt, cells, dx, seed=1):
    """cells^3 cells with 8 jittered particles each, F = I + 1 % noise, straight into the AoSoA buffer"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = 2 * cells
    i = torch.arange(k, device="cuda", dtype=torch.float32)
    idx = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    n = idx.shape[0]
    h = dx / 2
    pos = 0.25 + (idx + 0.5) * h + (torch.rand(n, 3, device="cuda", generator=g) - 0.5) * h * 0.8
    aos = torch.zeros(n, mt.nchn, device="cuda")
    aos[:, 0] = 1000.0 * dx ** 3 / 8
    aos[:, 1:4] = pos
    aos[:, 4:7] = 0.5 * torch.randn(n, 3, device="cuda", generator=g)
    aos[:, 7:16] = 0.1 * torch.randn(n, 9, device="cuda", generator=g)
    aos[:, 16:25] = torch.eye(3, device="cuda").reshape(1, 9) + 0.01 * torch.randn(n, 9, device="cuda", generator=g)
    zs.lib().zs_rocm_tv_from_aos_f32(mt.pol.handle, aos.data_ptr(), n, mt.nchn, mt.L, mt.buf.data_ptr())
    mt.pol.syncCtx()


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
    return dict(median_ms=float(np.median(a)), p10_ms=float(np.percentile(a, 10)), p90_ms=float(np.percentile(a, 90)), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100, help="edge of the cube in cells (100: 8 M particles)")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--side", type=int, default=8, choices=[4, 8])
    ap.add_argument("--model", type=int, default=0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--particle-reps", type=int, default=5, help="launches of the (slow) particle-order path")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    pol = zs.rocm_exec()
    pol.sync(False)
    dx, dt = 1.0 / a.grid, 1e-4
    n = (2 * a.cells) ** 3
    mt = MpmTransfer(pol, n, dx, dt, model=a.model, side=a.side, volume=dx ** 3 / 8)
    make_particles(mt, a.cells, dx)
    nb = mt.build_partition(max(4096, 2 * (a.cells // a.side + 3) ** 3))
    mt.rebin()
    mt.clear_grid()
    mt.p2g()
    mt.grid_update((0.0, -9.8, 0.0))
    pol.syncCtx()
    # trial velocities: the grid's own node velocities as a dof vector
    v = mt.grid.reshape(nb, 7, a.side ** 3)[:, 1:4, :].permute(0, 2, 1).contiguous().reshape(-1, 3)
    out = mt.dof_vector()
    pol.syncCtx()
    res = dict(n=n, nblocks=nb, side=a.side, model=a.model, dx=dx)
    res["implicit_force_binned"] = timed(pol, lambda: mt.implicit_force(v, out, binned=True), a.reps, a.warmup)
    res["implicit_force_particle_order"] = timed(pol, lambda: mt.implicit_force(v, out, binned=False), a.particle_reps, 1)

    def pair():   # the unfused reference-order pair; positions advance by dt v per call, far below a cell over the whole run
        mt.g2p()
        mt.p2g()
    res["g2p_plus_p2g_unfused"] = timed(pol, pair, a.reps, a.warmup)
    res["ratio_force_over_pair"] = res["implicit_force_binned"]["median_ms"] / res["g2p_plus_p2g_unfused"]["median_ms"]
    # algorithmic bytes per particle: x 12 + F 36 read, nothing written; grid traffic per particle (3 + 3 floats per node, 8 particles
    # per cell)
    res["bytes_per_particle"] = dict(implicit_force=48 + 24 / 8.0, g2p_plus_p2g=48 + 96 + 100 + (12 + 28) / 8.0)
    assert zs.lib().zs_rocm_last_error(-1) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
