"""Times the conservative step bound of a mesh (TriMesh.step_candidates, TriMesh.max_step: zs_rocm_mesh_ccd) next to the same additive
CCD written in torch on the GPU (a masked loop over the pairs that are still running, amin at the end) on the two scenes of
tools/bench_barrier.py:

    surface   the jittered 980 k-triangle surface (--side 700), dHat = half the mean edge; direction `random`: seeded, uniform in
              [-a dHat, a dHat]^3 with a = --amplitude (0.25: the candidate radius 2 max|direction| comes to about dHat)
    sheets    two jittered sheets of about 1 M triangles each (--sheet 708), a gap of h / 2, dHat = h; the same seeded direction, and
              `approach`: that plus --approach (0.6) x dHat downwards on the upper sheet, so the sheets would pass through each other

Rows per scene and direction, medians over --reps repetitions after --warmup, bracketed by HIP events on the policy's stream with the
policy not synchronising, library and torch alternating inside every repetition of the same process:
    step_candidates    TriMesh.step_candidates: the proximity pass at the inflated radius (with its host read-backs)
    max_step           zs_rocm_mesh_ccd on those lists
    barrier_energy     zs_rocm_mesh_barrier_energy on the same lists with dHat = the radius: one distance evaluation per pair, the floor of
                       max_step's first phase
    torch_max_step     the torch restatement
Also: the distribution of distance evaluations per pair and the share of pairs that leave at the early out (from the torch loop), the
two step bounds next to each other (a sanity check, not a test), pair counts.

    python tools/bench_ccd.py [--side 700] [--sheet 708] [--reps 20] [--warmup 3] [--cases surface:random,sheets:random,sheets:approach]
                              [--rows max_step,..] [--out profiles/mesh_ccd.json]
prints one JSON document."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zpc_amd as zs  # noqa: E402
from zpc_amd.mesh import TriMesh  # noqa: E402
from bench_barrier import dot, seg  # noqa: E402
from bench_mesh_levelset import jittered_surface  # noqa: E402
from bench_proximity import two_sheets, stats  # noqa: E402

SLACK, T_MAX, MAX_ITER = 0.1, 1.0, 256


def dist_pt(Y):
    p, a, b, c = (Y[:, k] for k in range(4))
    ab, ac, pa = b - a, c - a, p - a
    n = torch.linalg.cross(ab, ac)
    nn = dot(n, n)
    ok = nn > 1e-13 * dot(ab, ab) * dot(ac, ac)
    nn1 = torch.where(ok, nn, torch.ones_like(nn))
    b1, b2 = dot(n, torch.linalg.cross(pa, ac)) / nn1, dot(n, torch.linalg.cross(ab, pa)) / nn1
    face = ok & (1 - b1 - b2 >= 0) & (b1 >= 0) & (b2 >= 0)
    h = dot(n, pa)
    de = torch.minimum(torch.minimum(seg(p, a, b)[0], seg(p, b, c)[0]), seg(p, c, a)[0])
    return torch.sqrt(torch.where(face, h * h / nn1, de))


def dist_ee(Y):
    a0, a1, b0, b1 = (Y[:, k] for k in range(4))
    u, v, w = a1 - a0, b1 - b0, a0 - b0
    n = torch.linalg.cross(u, v)
    nn = dot(n, n)
    ok = nn > 1e-13 * dot(u, u) * dot(v, v)
    nn1 = torch.where(ok, nn, torch.ones_like(nn))
    s, t = dot(torch.linalg.cross(v, w), n) / nn1, dot(torch.linalg.cross(u, w), n) / nn1
    inter = ok & (s > 0) & (s < 1) & (t > 0) & (t < 1)
    q = w + s[:, None] * u - t[:, None] * v
    d2 = torch.where(inter, dot(q, q), torch.full_like(nn, float("inf")))
    for pt, q0, q1 in ((a0, b0, b1), (a1, b0, b1), (b0, a0, a1), (b1, a0, a1)):
        d2 = torch.minimum(d2, seg(pt, q0, q1)[0])
    return torch.sqrt(d2)


def torch_accd(x, p, ids, ee):
    """(t [n], evaluations [n]) of the pairs with vertex numbers ids [n, 4]: ccd_device.hpp vectorised, the loop over the live pairs only"""
    dist = dist_ee if ee else dist_pt
    X, P = x[ids], p[ids]
    q = P - P.mean(dim=1, keepdim=True)
    nq = torch.linalg.vector_norm(q, dim=2)
    lp = (torch.maximum(nq[:, 0], nq[:, 1]) + torch.maximum(nq[:, 2], nq[:, 3])) if ee else (nq[:, 0] + nq[:, 1:].amax(dim=1))
    lp = lp * (1 + 2.0 ** -21)
    d0 = dist(X)
    g = SLACK * d0
    t = torch.zeros_like(d0)
    evals = torch.zeros(len(ids), dtype=torch.int32, device=x.device)
    tl = (1 - SLACK) * d0 / torch.where(lp > 0, lp, torch.ones_like(lp))
    out = (lp == 0) | ((d0 > 0) & (tl >= T_MAX))
    t[out] = T_MAX
    live = torch.nonzero(~out & (d0 > 0))[:, 0]
    for _ in range(MAX_ITER):
        if not len(live):
            break
        tt = torch.clamp(t[live] + tl[live], max=T_MAX)
        d = dist(X[live] + tt[:, None, None] * P[live])
        evals[live] += 1
        go = ~((t[live] > 0) & (d < g[live]))
        live, tt, d = live[go], tt[go], d[go]
        t[live] = tt
        tl[live] = 0.9 * d / lp[live]
        live = live[tt < T_MAX]
    return t, evals


def run_case(pol, mesh, name, which, x, p, dhat, reps, warmup, only):
    L, H = zs.lib(), pol.handle
    i32, f32 = torch.int32, torch.float32
    cand = mesh.step_candidates(p, T_MAX)
    pt, ee = cand.pt_pairs, cand.ee_pairs
    npt, nee = len(pt), len(ee)
    radius = float(torch.sqrt(torch.maximum(cand.pt_dist2.max(), cand.ee_dist2.max())).item())   # (reported: the largest listed distance)
    tris, edges = mesh_tris[id(mesh)], mesh.edges().long()
    ids_pt = torch.cat([pt[:, :1].long(), tris[pt[:, 1].long()]], dim=1)
    ids_ee = torch.cat([edges[ee[:, 0].long()], edges[ee[:, 1].long()]], dim=1)
    pt_toi, ee_toi = torch.empty(npt, dtype=f32, device="cuda"), torch.empty(nee, dtype=f32, device="cuda")
    tmin, status = torch.empty((), dtype=f32, device="cuda"), torch.empty(4, dtype=i32, device="cuda")
    pe, ee_e = torch.empty(npt, dtype=f32, device="cuda"), torch.empty(nee, dtype=f32, device="cuda")
    total, st2 = torch.empty((), dtype=torch.float64, device="cuda"), torch.empty(2, dtype=i32, device="cuda")
    big = float(np.float32(1.0))     # every listed pair is inside dHat = 1: the energy pass evaluates all of them
    keep = {}

    def step_candidates():
        mesh.step_candidates(p, T_MAX)

    def max_step():
        assert L.zs_rocm_mesh_ccd(H, mesh.handle, None, p.data_ptr(), pt.data_ptr(), npt, ee.data_ptr(), nee, SLACK, T_MAX, MAX_ITER,
                                  pt_toi.data_ptr(), ee_toi.data_ptr(), tmin.data_ptr(), status.data_ptr()) == 0

    def barrier_energy():
        assert L.zs_rocm_mesh_barrier_energy(H, mesh.handle, None, pt.data_ptr(), npt, ee.data_ptr(), nee, big, 1.0, 0, pe.data_ptr(),
                                             ee_e.data_ptr(), total.data_ptr(), st2.data_ptr()) == 0

    def torch_max_step():
        t0, e0 = torch_accd(x, p, ids_pt, False)
        t1, e1 = torch_accd(x, p, ids_ee, True)
        keep["t"], keep["evals"] = torch.minimum(t0.amin(), t1.amin()).clamp(max=T_MAX), (e0, e1)

    rows = dict(step_candidates=step_candidates, max_step=max_step, barrier_energy=barrier_energy, torch_max_step=torch_max_step)
    rows = {k: fn for k, fn in rows.items() if not only or k in only}
    ms = {k: [] for k in rows}
    stream = torch.cuda.ExternalStream(pol.getStream()) if pol.getStream() else torch.cuda.default_stream()
    pol.sync(False)
    with torch.cuda.stream(stream):
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
    dist = {}
    for kind, ev, toi in ((("pt", keep["evals"][0], pt_toi), ("ee", keep["evals"][1], ee_toi)) if keep else ()):
        e = ev.cpu().numpy()
        hit = e[(toi < T_MAX).cpu().numpy()]
        dist[kind] = dict(pairs=int(len(e)), early_out_share=float((e == 0).mean()) if len(e) else 0.0, hits=int(len(hit)),
                          evaluations_total=int(e.sum()), histogram={str(k): int(((e >= lo) & (e <= hi)).sum()) for k, lo, hi in
                                                                     (("0", 0, 0), ("1-2", 1, 2), ("3-4", 3, 4), ("5-8", 5, 8), ("9-16", 9, 16),
                                                                      ("17-64", 17, 64), ("65-256", 65, 256))},
                          hits_p50=float(np.percentile(hit, 50)) if len(hit) else 0.0, hits_p99=float(np.percentile(hit, 99)) if len(hit) else 0.0,
                          most=int(e.max()) if len(e) else 0)
    return dict(scene=name, direction=which, vertices=mesh.nv, triangles=mesh.nt, dhat=dhat, largest_listed_distance=radius, pt_pairs=npt,
                ee_pairs=nee, times={k: stats(v) for k, v in ms.items()}, evaluations=dist,
                check=dict(t=float(tmin.item()), torch_t=float(keep["t"].item()) if keep else None, status=status.tolist()))


mesh_tris = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--sheet", type=int, default=708)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--amplitude", type=float, default=0.25, help="the seeded direction is uniform in [-amplitude dHat, amplitude dHat]^3")
    ap.add_argument("--approach", type=float, default=0.6, help="`approach` adds -approach dHat in z on the upper sheet (the gap is dHat / 2)")
    ap.add_argument("--cases", default="surface:random,sheets:random,sheets:approach")
    ap.add_argument("--rows", default=None, help="comma-separated subset of the rows (default all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = [c.split(":") for c in a.cases.split(",")]
    only = set(a.rows.split(",")) if a.rows else None
    torch.cuda.set_device(0)
    pol = zs.rocm_exec()
    out = []

    def scene(name, v, t, dhat):
        directions = [w for n, w in cases if n == name]
        if not directions:
            return
        mesh = TriMesh(pol, v, t)
        mesh_tris[id(mesh)] = torch.from_numpy(t.astype(np.int64)).cuda()
        x = torch.from_numpy(v).cuda()
        rnd = np.random.default_rng(11).uniform(-a.amplitude * dhat, a.amplitude * dhat, v.shape)
        for which in directions:
            p = rnd.copy()
            if which == "approach":
                p[len(v) // 2:, 2] -= a.approach * dhat
            out.append(run_case(pol, mesh, name, which, x, torch.from_numpy(p.astype(np.float32)).cuda(), dhat, a.reps, a.warmup, only))

    if any(n == "surface" for n, _ in cases):
        v, t = jittered_surface(a.side)
        q = v[t.astype(np.int64)].astype(np.float64)
        mean_edge = float(np.mean([np.linalg.norm(q[:, k] - q[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
        scene("surface", v, t, float(np.float32(0.5 * mean_edge)))
    if any(n == "sheets" for n, _ in cases):
        v, t, h = two_sheets(a.sheet)
        scene("sheets", v, t, float(np.float32(h)))
    doc = json.dumps(dict(bench="mesh_ccd", device=torch.cuda.get_device_name(0), slack=SLACK, t_max=T_MAX, max_iter=MAX_ITER,
                          amplitude=a.amplitude, approach=a.approach, scenes=out), indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
