#!/usr/bin/env python3
"""CPU model of the rounds a 4^3 bin of the slotted storage needs while the default bench's column falls (profiles/block_list.md).

The cloud is bench.py's generate_particles -- 8 particles per cell on a jittered 2 x 2 x 2 lattice, velocity 0.05 N(0, 1) per axis plus
the drift -- in free fall: x(k) = x0 + v k dt + g (k dt)^2 / 2.  A particle's cell is its base node floor(x / dx - 0.5); a bin has as many
rounds as its fullest cell (compact storage: round r of a bin holds the cells with more than r particles).  Printed per step: the mean
rounds of the bins that are full (all 64 cells occupied, i.e. not at the column's surface), the lane occupancy particles / (64 rounds),
and how many rounds of a bin hold at most T occupied cells, with the particles in them.

    python tools/block_rounds_model.py [--cells 32,64,32] [--steps 8,16,24] [--thresholds 4,8,12]
"""
import argparse

import numpy as np

M64 = (1 << 64) - 1


def hash_uniform(gid, stream):
    """bench.py's _hash_uniform on uint64 (the same low 64 bits as its wrapped int64 arithmetic)"""
    x = gid.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(((stream + 1) * 0x632BE59BD9B4E019) & M64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def hash_normal(gid, stream):
    u1 = np.maximum(hash_uniform(gid, 2 * stream), 1e-12)
    u2 = hash_uniform(gid, 2 * stream + 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def cloud(ext, dx, seed=0):
    """positions and velocities (float64) of the particles of the cells [0, ext) -- the column's interior"""
    n = ext[0] * ext[1] * ext[2] * 8
    pid = np.arange(n, dtype=np.int64)
    cell, sub = pid // 8, pid % 8
    c = [cell // (ext[1] * ext[2]), (cell // ext[2]) % ext[1], cell % ext[2]]
    gid = ((((c[0] + 4096) * 8192 + (c[1] + 4096)) * 8192 + (c[2] + 4096)) * 8 + sub + seed * 7919).astype(np.uint64)
    s = [sub // 4, (sub // 2) % 2, sub % 2]
    h = dx / 2
    x = np.stack([((c[d] * 2 + s[d]) + 0.5 + (hash_uniform(gid, d) - 0.5) * 0.8).astype(np.float32) * np.float32(h) for d in range(3)], 1)
    v = np.stack([(0.05 * hash_normal(gid, 3 + d)).astype(np.float32) for d in range(3)], 1)
    return x.astype(np.float64), v.astype(np.float64)


def bin_rounds(x, dx, ext):
    """per 4^3 bin inside the box: particles per cell [bins, 64]"""
    c = np.floor(x / dx - 0.5).astype(np.int64)
    ok = ((c >= 0) & (c < np.asarray(ext))).all(1)
    c = c[ok]
    nb = [e // 4 for e in ext]
    b = ((c[:, 0] >> 2) * nb[1] + (c[:, 1] >> 2)) * nb[2] + (c[:, 2] >> 2)
    lane = ((c[:, 0] & 3) * 4 + (c[:, 1] & 3)) * 4 + (c[:, 2] & 3)
    cnt = np.zeros((nb[0] * nb[1] * nb[2], 64), np.int64)
    np.add.at(cnt, (b, lane), 1)
    return cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="32,64,32")
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--dt", type=float, default=1e-4)
    ap.add_argument("--drift", default="0,-1.0,0")
    ap.add_argument("--steps", default="0,8,16,24")
    ap.add_argument("--thresholds", default="4,8,12")
    a = ap.parse_args()
    ext = [int(t) for t in a.cells.split(",")]
    dx = 1.0 / a.grid
    drift = np.array([float(t) for t in a.drift.split(",")])
    ths = [int(t) for t in a.thresholds.split(",")]
    x0, v = cloud(ext, dx)
    v = v + drift
    print("step  rounds/full bin  occupancy  " + "  ".join("rounds<=%d cells (particles)" % t for t in ths))
    for k in [int(t) for t in a.steps.split(",")]:
        t = k * a.dt
        x = x0 + v * t
        x[:, 1] -= 0.5 * 9.8 * t * t
        cnt = bin_rounds(x, dx, ext)
        # the box stands for the column's interior: its outermost bins lose particles to the outside and get none back, leave them out
        cnt = cnt.reshape(ext[0] // 4, ext[1] // 4, ext[2] // 4, 64)[1:-1, 1:-1, 1:-1].reshape(-1, 64)
        cnt = cnt[(cnt > 0).all(1)]
        rounds = cnt.max(1)
        occ = cnt.sum() / (64.0 * rounds.sum())
        cols = []
        for T in ths:
            # round r of a bin holds the cells with more than r particles
            rr = np.arange(cnt.max())[None, :, None]
            cells_in_round = (cnt[:, None, :] > rr).sum(2)                      # [bins, rounds]
            sparse = (cells_in_round > 0) & (cells_in_round <= T)
            cols.append("%.2f (%.1f)" % (sparse.sum(1).mean(), (cells_in_round * sparse).sum(1).mean()))
        print("%4d  %15.1f  %9.2f  %s" % (k, rounds.mean(), occ, "  ".join("%-27s" % c for c in cols)))


if __name__ == "__main__":
    main()
