"""Times lagged IPC friction on a mesh (TriMesh.friction_lag / friction / friction_hessian_product: zs_rocm_mesh_friction_{lag,energy,
gradient,hessian_product}) next to the same closed forms written in torch on the GPU -- what a user had before it -- and next to
zs_rocm_mesh_barrier_gradient on the same lists, on the two scenes of tools/bench_barrier.py:

    surface   the jittered 980 k-triangle surface (--side 700), dHat = half the mean edge
    sheets    two jittered sheets of about 1 M triangles each (--sheet 708), a gap of h / 2, dHat = h

The displacement is seeded, of the size of eps_v (--epsv, default dHat / 10), so that both branches of f0 hold pairs.  Rows per scene, medians
over --reps repetitions after --warmup, bracketed by HIP events on the policy's stream with the policy not synchronising, library and torch
alternating inside every repetition of the same process:
    lag                  zs_rocm_mesh_friction_lag: one 32-byte record per pair (distances recomputed, as the barrier does)
    energy               zs_rocm_mesh_friction_energy: per-pair energies from the record and the float64 total
    energy_gradient      zs_rocm_mesh_friction_gradient: the same and the gradient through the barrier's incidence
    hessian_product      zs_rocm_mesh_friction_hessian_product for a seeded direction x
    barrier_gradient     zs_rocm_mesh_barrier_gradient on the same lists: the distance chain and the same gather
    torch_energy         gather the four rows of u per pair, the closed forms of include/zensim_rocm/friction_device.hpp on the record, float64 sum
    torch_energy_gradient    the same and index_add_ of the per-pair contributions (float atomics: not reproducible)
    torch_hessian_product    the closed form of the product and index_add_
Also: the largest differences between the two routes (a sanity check, not a test), pair counts, the share of pairs below the threshold.

    python tools/bench_friction.py [--side 700] [--sheet 708] [--reps 20] [--warmup 3] [--mu 0.4] [--out profiles/mesh_friction.json]
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
from bench_mesh_levelset import jittered_surface  # noqa: E402
from bench_proximity import two_sheets, stats  # noqa: E402

KAPPA = 1.0


def dot(a, b):
    return (a * b).sum(-1)


def torch_slip(record, rows):
    """(lambda, w, n, ut, y) of the records at the gathered rows [n, 4, 3]"""
    n, lam, w = record[:, :3], record[:, 3], record[:, 4:]
    z = (w[:, :, None] * rows).sum(dim=1)
    t = z - dot(n, z)[:, None] * n
    return lam, w, n, t, torch.sqrt(dot(t, t))


def torch_energy(record, u, ids, mu, eps, grad):
    lam, w, _, ut, y = torch_slip(record, u[ids])
    f0 = torch.where(y >= eps, y, y * y * (eps - y / 3) / (eps * eps) + eps / 3)
    e = mu * lam * f0
    if not grad:
        return e, None
    c1 = torch.where(y >= eps, 1 / torch.where(y >= eps, y, torch.ones_like(y)), (2 * eps - y) / (eps * eps))
    return e, (mu * lam * c1)[:, None, None] * w[:, :, None] * ut[:, None, :]


def torch_product(record, u, x, ids, mu, eps):
    lam, w, n, ut, y = torch_slip(record, u[ids])
    z = (w[:, :, None] * x[ids]).sum(dim=1)
    zt = z - dot(n, z)[:, None] * n
    y1 = torch.where(y > 0, y, torch.ones_like(y))
    c1 = torch.where(y >= eps, 1 / y1, (2 * eps - y) / (eps * eps))
    c2 = torch.where(y > 0, torch.where(y >= eps, -1 / y1 ** 3, -1 / (eps * eps * y1)), torch.zeros_like(y))
    m = c1[:, None] * zt + (c2 * dot(ut, zt))[:, None] * ut
    return (mu * lam)[:, None, None] * w[:, :, None] * m[:, None, :]


def run_scene(pol, name, v, t, dhat, mu, epsv, reps, warmup):
    L, H = zs.lib(), pol.handle
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    prox = mesh.proximity(dhat)
    pt, ee = prox.pt_pairs, prox.ee_pairs
    npt, nee, nv = len(pt), len(ee), mesh.nv
    epsv = float(np.float32(dhat / 10 if epsv is None else epsv))
    i32, f32 = torch.int32, torch.float32
    lag = mesh.friction_lag(prox, dhat, KAPPA)
    starts, entries, nscratch = mesh._incidence(prox, pt, ee)
    scratch = torch.empty(nscratch, dtype=f32, device="cuda")
    record = torch.empty_like(lag.record)
    pe, ee_e = torch.empty(npt, dtype=f32, device="cuda"), torch.empty(nee, dtype=f32, device="cuda")
    total, grad = torch.empty((), dtype=torch.float64, device="cuda"), torch.empty(nv, 3, dtype=f32, device="cuda")
    hx, bgrad = torch.empty(nv, 3, dtype=f32, device="cuda"), torch.empty(nv, 3, dtype=f32, device="cuda")
    status = torch.empty(2, dtype=i32, device="cuda")
    g = np.random.default_rng(5)
    u = torch.from_numpy((epsv * g.standard_normal((nv, 3))).astype(np.float32)).cuda()
    xdir = torch.from_numpy(g.standard_normal((nv, 3)).astype(np.float32)).cuda()
    tris, edges = torch.from_numpy(t.astype(np.int64)).cuda(), mesh.edges().long()
    ids = torch.cat([torch.cat([pt.long()[:, :1], tris[pt.long()[:, 1]]], dim=1), torch.cat([edges[ee.long()[:, 0]], edges[ee.long()[:, 1]]], dim=1)])
    lists = (pt.data_ptr(), npt, ee.data_ptr(), nee)
    head = (H, mesh.handle, u.data_ptr()) + lists + (lag.record.data_ptr(), mu, epsv)
    tail = (pe.data_ptr(), ee_e.data_ptr(), total.data_ptr())
    inc = (starts.data_ptr(), entries.data_ptr(), scratch.data_ptr())
    keep = {}

    def lag_():
        assert L.zs_rocm_mesh_friction_lag(H, mesh.handle, None, *lists, dhat, KAPPA, 1, record.data_ptr(), status.data_ptr()) == 0

    def energy():
        assert L.zs_rocm_mesh_friction_energy(*head, *tail, status.data_ptr()) == 0

    def energy_gradient():
        assert L.zs_rocm_mesh_friction_gradient(*head, *inc, *tail, grad.data_ptr(), status.data_ptr()) == 0

    def hessian_product():
        assert L.zs_rocm_mesh_friction_hessian_product(H, mesh.handle, u.data_ptr(), xdir.data_ptr(), *lists, lag.record.data_ptr(), mu, epsv, *inc,
                                                       hx.data_ptr(), status.data_ptr()) == 0

    def barrier_gradient():
        assert L.zs_rocm_mesh_barrier_gradient(H, mesh.handle, None, *lists, dhat, KAPPA, 1, *inc, *tail, bgrad.data_ptr(), status.data_ptr()) == 0

    def t_energy():
        keep["e"] = torch_energy(lag.record, u, ids, mu, epsv, False)[0].double().sum()

    def t_energy_gradient():
        e, terms = torch_energy(lag.record, u, ids, mu, epsv, True)
        out = torch.zeros(nv, 3, dtype=f32, device="cuda")
        out.index_add_(0, ids.reshape(-1), terms.reshape(-1, 3))
        keep["e"], keep["g"] = e.double().sum(), out

    def t_hessian_product():
        out = torch.zeros(nv, 3, dtype=f32, device="cuda")
        out.index_add_(0, ids.reshape(-1), torch_product(lag.record, u, xdir, ids, mu, epsv).reshape(-1, 3))
        keep["hx"] = out

    # (the barrier row shares the energy buffers and the status with the friction rows: one more friction call after the loop fills them for
    # the check)
    rows = dict(lag=lag_, barrier_gradient=barrier_gradient, energy=energy, torch_energy=t_energy, energy_gradient=energy_gradient,
                torch_energy_gradient=t_energy_gradient, hessian_product=hessian_product, torch_hessian_product=t_hessian_product)
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
        energy_gradient()
    pol.sync(True)
    pol.syncCtx()
    assert zs.lib().zs_rocm_last_error(-1) == 0
    y = torch_slip(lag.record, u[ids])[4]
    active = lag.record[:, 3] > 0
    return dict(scene=name, vertices=nv, triangles=mesh.nt, edges=mesh.num_edges, dhat=dhat, mu=mu, eps_v=epsv, pt_pairs=npt, ee_pairs=nee,
                active_pairs=int(active.sum().item()), below_threshold=int((active & (y < epsv)).sum().item()), incidences=4 * (npt + nee),
                times={k: stats(x_) for k, x_ in ms.items()},
                check=dict(energy=float(total.item()), torch_energy=float(keep["e"].item()), records_equal=bool(torch.equal(record, lag.record)),
                           largest_gradient=float(keep["g"].abs().max().item()),
                           largest_gradient_difference=float((grad - keep["g"]).abs().max().item()),
                           largest_product=float(keep["hx"].abs().max().item()),
                           largest_product_difference=float((hx - keep["hx"]).abs().max().item()), overflow=status.tolist(),
                           zero_distance=list(lag.zero_distance)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--sheet", type=int, default=708)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mu", type=float, default=0.4)
    ap.add_argument("--epsv", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    pol = zs.rocm_exec()
    out = []
    v, t = jittered_surface(a.side)
    p = v[t.astype(np.int64)].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
    out.append(run_scene(pol, "surface", v, t, float(np.float32(0.5 * mean_edge)), a.mu, a.epsv, a.reps, a.warmup))
    v, t, h = two_sheets(a.sheet)
    out.append(run_scene(pol, "sheets", v, t, float(np.float32(h)), a.mu, a.epsv, a.reps, a.warmup))
    doc = json.dumps(dict(bench="mesh_friction", device=torch.cuda.get_device_name(0), scenes=out), indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
