"""Times the mesh incremental potential (zpc_amd.mesh_potential.MeshPotential: zs_rocm_mesh_potential_{evaluate,line_search}) against what
a user composed from the public calls before it existed, on the two scenes of the other mesh benches:

    surface   the jittered 980 k-triangle surface (--side 700)
    sheets    two jittered sheets of about 1 M triangles each (--sheet 708)

at trial positions 0.1 mean edge length from rest, with all three terms (elastic, barrier, friction; masses of DENSITY x vertex area).  Rows
per scene, medians over --reps repetitions after --warmup, a host clock around work that ends in a device synchronise, library and
comparator alternating inside every repetition of the same process:
    evaluate             MeshPotential.evaluate: energy, parts and gradient
    composed_evaluate    TriMesh.elastic + TriMesh.barrier + TriMesh.friction (gradient calls), the torch composition
                         m (x - target) + scale (ge + gb + gf), the inertia energy in torch and the host sum of the energies
    search_1 / search_4  MeshPotential.line_search over --trials trials that are all rejected (c1 so large that no trial passes) with
                         check_every 1 and 4; per trial: (that time - the time of a one-trial search) / (--trials - 1)
    composed_trial       one trial composed by the user: x + t p and u in torch, the three public energy calls, the inertia energy in torch
                         and an .item() decision on the host
The comparator is the public calls as they are, never the new code.  Also, once per scene: the relative difference of the two gradients and
of the two energies.

    python tools/bench_potential.py [--side 700] [--sheet 708] [--reps 10] [--warmup 2] [--trials 9] [--out profiles/mesh_potential.json]
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
from zpc_amd.mesh_potential import MeshPotential  # noqa: E402
from bench_mesh_levelset import jittered_surface  # noqa: E402
from bench_proximity import two_sheets, stats  # noqa: E402

DENSITY, SCALE, MU, LAM, KB, KAPPA, FRICTION_MU, EPS_V = 1e3, 1e-2, 1.3e3, 0.7e3, 2e-3, 1e3, 0.3, 1e-3


def run_scene(pol, name, v, t, dhat, a):
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    mesh.set_rest_shape()
    area = mesh.rest_shape()[3]
    prox = mesh.proximity(dhat)
    lag = mesh.friction_lag(prox, dhat, KAPPA)
    p3 = v[t.astype(np.int64)].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(p3[:, k] - p3[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
    g = np.random.default_rng(5)
    x = torch.from_numpy((v + 0.1 * mean_edge * g.standard_normal(v.shape)).astype(np.float32)).cuda()
    start = x - torch.from_numpy((0.1 * EPS_V * g.standard_normal(v.shape)).astype(np.float32)).cuda()
    target = x + torch.from_numpy((0.01 * mean_edge * g.standard_normal(v.shape)).astype(np.float32)).cuda()
    mass = (DENSITY * area).contiguous()
    P = MeshPotential(mesh, mass, SCALE, target, start, elastic=(MU, LAM, KB), barrier=(prox, dhat, KAPPA), friction=(lag, FRICTION_MU, EPS_V))
    keep = {}

    def inertia(y):
        d = y - target
        return 0.5 * (mass.double() * (d.double() ** 2).sum(dim=1)).sum()

    def evaluate():
        keep["lib"] = P.evaluate(x)

    def composed_evaluate():
        el, ba, fr = mesh.elastic(MU, LAM, KB, verts=x), mesh.barrier(prox, dhat, KAPPA, verts=x), mesh.friction(lag, x - start, FRICTION_MU, EPS_V)
        grad = mass[:, None] * (x - target) + SCALE * (el.grad + ba.grad + fr.grad)
        energy = inertia(x).item() + SCALE * (el.energy.item() + ba.energy.item() + fr.energy.item())
        keep["composed"] = (energy, grad)

    # a descent direction short enough to keep every trial far from contact: 1e-3 mean edge lengths at the vertex that moves most
    evaluate()
    grad = keep["lib"].grad
    direction = (-grad * (1e-3 * mean_edge / float(grad.abs().max().item()))).contiguous()
    never = 1e30      # c1 so large that every trial is rejected

    def search(trials, check_every):
        r = P.line_search(x, direction, 1.0, c1=never, max_trials=trials, check_every=check_every)
        assert r.flag == "max_trials" and r.trials == trials

    def composed_trial():
        tk, e0, slope = 0.5, keep["composed"][0], -1.0
        xk = x + tk * direction
        el, ba = mesh.elastic(MU, LAM, KB, verts=xk, gradient=False), mesh.barrier(prox, dhat, KAPPA, verts=xk, gradient=False)
        fr = mesh.friction(lag, xk - start, FRICTION_MU, EPS_V, gradient=False)
        ek = inertia(xk).item() + SCALE * (el.energy.item() + ba.energy.item() + fr.energy.item())
        keep["accept"] = np.isfinite(ek) and ek <= e0 + never * tk * slope

    rows = dict(evaluate=evaluate, composed_evaluate=composed_evaluate, search_1_one_trial=lambda: search(1, 1), search_1=lambda: search(a.trials, 1),
                search_4=lambda: search(a.trials, 4), composed_trial=composed_trial)
    ms = {k: [] for k in rows}
    for it in range(a.warmup + a.reps):
        for k, fn in rows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            pol.syncCtx()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    assert zs.lib().zs_rocm_last_error(-1) == 0
    times = {k: stats(x_) for k, x_ in ms.items()}
    one = times["search_1_one_trial"]["median_ms"]
    for k in ("search_1", "search_4"):
        times[k + "_per_trial_ms"] = (times[k]["median_ms"] - one) / (a.trials - 1)
    energy, cgrad = keep["composed"]
    lib = keep["lib"]
    return dict(scene=name, vertices=mesh.nv, triangles=mesh.nt, hinges=mesh.num_hinges, pt_pairs=len(prox.pt_pairs), ee_pairs=len(prox.ee_pairs),
                trials_timed=a.trials, times=times,
                evaluate_over_composed=times["evaluate"]["median_ms"] / times["composed_evaluate"]["median_ms"],
                trial_over_composed_check_every_1=times["search_1_per_trial_ms"] / times["composed_trial"]["median_ms"],
                trial_over_composed_check_every_4=times["search_4_per_trial_ms"] / times["composed_trial"]["median_ms"],
                relative_difference_of_gradients=float((lib.grad - cgrad).abs().max().item()) / float(cgrad.abs().max().item()),
                relative_difference_of_energies=abs(float(lib.energy.item()) - energy) / abs(energy))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--sheet", type=int, default=708)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trials", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_potential: no GPU (there is no CPU fallback)")
    torch.cuda.set_device(0)
    pol = zs.rocm_exec()
    out = []
    v, t = jittered_surface(a.side)
    p = v[t.astype(np.int64)].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
    out.append(run_scene(pol, "surface", v, t, float(np.float32(0.5 * mean_edge)), a))
    v, t, h = two_sheets(a.sheet)
    out.append(run_scene(pol, "sheets", v, t, float(np.float32(h)), a))
    doc = json.dumps(dict(bench="mesh_potential", device=torch.cuda.get_device_name(0), scenes=out), indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
