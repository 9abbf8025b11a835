"""Times the mesh barrier potential (TriMesh.barrier, TriMesh.barrier_hessian_product: zs_rocm_mesh_barrier_{incidence,energy,gradient,
hessian_product}) next to the same computation written
in torch on the GPU -- what a user had before it -- on the two scenes of tools/bench_proximity.py:

    surface   the jittered 980 k-triangle surface (--side 700), dHat = half the mean edge
    sheets    two jittered sheets of about 1 M triangles each (--sheet 708), a gap of h / 2, dHat = h

Rows per scene, medians over --reps repetitions after --warmup, bracketed by HIP events on the policy's stream with the policy not
synchronising, library and torch alternating inside every repetition of the same process:
    incidence          zs_rocm_mesh_barrier_incidence (once per constraint set)
    energy             zs_rocm_mesh_barrier_energy: per-pair energies and the float64 total
    energy_gradient    zs_rocm_mesh_barrier_gradient: the same and the gradient through the incidence
    torch_energy       gather the four vertices per pair, the closed forms of include/zensim_rocm/barrier_device.hpp vectorised (every
                       candidate of tri_closest / ee_closest evaluated, the smallest selected), float64 sum
    torch_energy_gradient   the same and index_add_ of the per-pair contributions into the gradient (float atomics: not reproducible)
    hessian_product    zs_rocm_mesh_barrier_hessian_product, psd = 0: H x for a seeded direction x through the same incidence
    hessian_product_psd     the same with psd = 1 (the positive semi-definite H+)
    torch_hessian_product   torch.autograd.functional.hvp over torch_energy (the closed forms differentiated twice on the device)
Also: the largest differences between the two routes (a sanity check, not a test), pair and incidence counts.

    python tools/bench_barrier.py [--side 700] [--sheet 708] [--reps 20] [--warmup 3] [--out profiles/mesh_barrier.json]
prints one JSON document."""
import argparse
import ctypes as C
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


def seg(p, u, v):
    e, d = v - u, p - u
    ee = dot(e, e)
    t = torch.where(ee > 0, dot(d, e) / torch.where(ee > 0, ee, torch.ones_like(ee)), torch.zeros_like(ee)).clamp(0, 1)
    r = d - t[:, None] * e
    return dot(r, r), t


def barrier(d2, dhat2):
    act = (d2 < dhat2) & (d2 > 0)
    x = torch.where(act, d2, torch.full_like(d2, 0.5 * dhat2))
    t, lg = x - dhat2, torch.log(x / dhat2)
    zero = torch.zeros_like(x)
    return torch.where(act, -KAPPA * t * t * lg, zero), torch.where(act, KAPPA * (-2 * t * lg - t * t / x), zero)


def torch_pt(x, tris, pairs, dhat2, grad):
    """(energy [n], contributions [n, 4, 3] or None, vertex ids [n, 4])"""
    ids = torch.cat([pairs[:, :1], tris[pairs[:, 1]]], dim=1)
    p, a, b, c = (x[ids[:, k]] for k in range(4))
    ab, ac, pa = b - a, c - a, p - a
    n = torch.linalg.cross(ab, ac)
    nn = dot(n, n)
    ok = nn > 1e-13 * dot(ab, ab) * dot(ac, ac)
    nn1 = torch.where(ok, nn, torch.ones_like(nn))
    b1, b2 = dot(n, torch.linalg.cross(pa, ac)) / nn1, dot(n, torch.linalg.cross(ab, pa)) / nn1
    b0 = 1 - b1 - b2
    face = ok & (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
    h = dot(n, pa)
    d0, t0 = seg(p, a, b)
    d1, t1 = seg(p, b, c)
    d2, t2 = seg(p, c, a)
    s0 = (d0 <= d1) & (d0 <= d2)
    s1 = ~s0 & (d1 <= d2)
    one, zero = torch.ones_like(t0), torch.zeros_like(t0)
    de = torch.where(s0, d0, torch.where(s1, d1, d2))
    be = torch.where(s0[:, None], torch.stack([one - t0, t0, zero], -1),
                     torch.where(s1[:, None], torch.stack([zero, one - t1, t1], -1), torch.stack([t2, zero, one - t2], -1)))
    dist2 = torch.where(face, h * h / nn1, de)
    bary = torch.where(face[:, None], torch.stack([b0, b1, b2], -1), be)
    e, bp = barrier(dist2, dhat2)
    if not grad:
        return e, None, ids
    r = p - (bary[:, 0, None] * a + bary[:, 1, None] * b + bary[:, 2, None] * c)
    w = torch.cat([torch.ones_like(bary[:, :1]), -bary], dim=1)
    return e, (2 * bp)[:, None, None] * w[:, :, None] * r[:, None, :], ids


def torch_ee(x, edges, pairs, rest, dhat2, grad):
    ids = torch.cat([edges[pairs[:, 0]], edges[pairs[:, 1]]], dim=1)
    a0, a1, b0, b1 = (x[ids[:, k]] for k in range(4))
    u, v, w = a1 - a0, b1 - b0, a0 - b0
    n = torch.linalg.cross(u, v)
    nn = dot(n, n)
    ok = nn > 1e-13 * dot(u, u) * dot(v, v)
    nn1 = torch.where(ok, nn, torch.ones_like(nn))
    s, t = dot(torch.linalg.cross(v, w), n) / nn1, dot(torch.linalg.cross(u, w), n) / nn1
    inter = ok & (s > 0) & (s < 1) & (t > 0) & (t < 1)
    q = w + s[:, None] * u - t[:, None] * v
    d2 = torch.where(inter, dot(q, q), torch.full_like(nn, float("inf")))
    s, t = torch.where(inter, s, torch.zeros_like(s)), torch.where(inter, t, torch.zeros_like(t))
    zero, one = torch.zeros_like(s), torch.ones_like(s)
    for k, (pt, q0, q1) in enumerate(((a0, b0, b1), (a1, b0, b1), (b0, a0, a1), (b1, a0, a1))):
        d, par = seg(pt, q0, q1)
        m = d < d2
        cs, ct = ((zero if k == 0 else one), par) if k < 2 else (par, (zero if k == 2 else one))
        d2, s, t = torch.where(m, d, d2), torch.where(m, cs, s), torch.where(m, ct, t)
    e, bp = barrier(d2, dhat2)
    eps = 1e-2 * rest[pairs[:, 0]] * rest[pairs[:, 1]]
    on = (eps > 0) & (nn < eps)
    e1 = torch.where(eps > 0, eps, torch.ones_like(eps))
    xx = nn / e1
    m = torch.where(on, (2 - xx) * xx, torch.ones_like(xx))
    if not grad:
        return m * e, None, ids
    mp = torch.where(on, (2 / e1) * (1 - xx), torch.zeros_like(xx))
    r = (a0 + s[:, None] * u) - (b0 + t[:, None] * v)
    wt = torch.stack([1 - s, s, -(1 - t), -t], dim=1)
    dcu, dcv = 2 * torch.linalg.cross(v, n), 2 * torch.linalg.cross(n, u)
    gc = torch.stack([-dcu, dcu, -dcv, dcv], dim=1)
    g = (mp * e)[:, None, None] * gc + (2 * m * bp)[:, None, None] * wt[:, :, None] * r[:, None, :]
    return m * e, g, ids


def run_scene(pol, name, v, t, dhat, reps, warmup):
    L, H = zs.lib(), pol.handle
    mesh = TriMesh(pol, v, t)
    mesh.set_rest()
    prox = mesh.proximity(dhat)
    pt, ee = prox.pt_pairs, prox.ee_pairs
    npt, nee, nv = len(pt), len(ee), mesh.nv
    sizes = (C.c_size_t * 3)()
    assert L.zs_rocm_mesh_barrier_sizes(mesh.handle, npt, nee, sizes) == 0
    i32, f32 = torch.int32, torch.float32
    starts, entries = torch.empty(sizes[0], dtype=i32, device="cuda"), torch.empty(sizes[1], dtype=i32, device="cuda")
    scratch = torch.empty(sizes[2], dtype=f32, device="cuda")
    pe, ee_e = torch.empty(npt, dtype=f32, device="cuda"), torch.empty(nee, dtype=f32, device="cuda")
    total, grad = torch.empty((), dtype=torch.float64, device="cuda"), torch.empty(nv, 3, dtype=f32, device="cuda")
    status = torch.empty(2, dtype=i32, device="cuda")
    x = torch.from_numpy(v).cuda()
    tris, edges, rest = torch.from_numpy(t.astype(np.int64)).cuda(), mesh.edges().long(), mesh.rest()
    ptl, eel = pt.long(), ee.long()
    dhat2 = float(np.float32(dhat) * np.float32(dhat))
    head = (H, mesh.handle, None, pt.data_ptr(), npt, ee.data_ptr(), nee, dhat, KAPPA, 1)
    tail = (pe.data_ptr(), ee_e.data_ptr(), total.data_ptr())
    keep = {}

    def incidence():
        assert L.zs_rocm_mesh_barrier_incidence(H, mesh.handle, pt.data_ptr(), npt, ee.data_ptr(), nee, starts.data_ptr(), entries.data_ptr()) == 0

    def energy():
        assert L.zs_rocm_mesh_barrier_energy(*head, *tail, status.data_ptr()) == 0

    def energy_gradient():
        assert L.zs_rocm_mesh_barrier_gradient(*head, starts.data_ptr(), entries.data_ptr(), scratch.data_ptr(), *tail, grad.data_ptr(),
                                               status.data_ptr()) == 0

    def torch_energy():
        keep["e"] = torch_pt(x, tris, ptl, dhat2, False)[0].double().sum() + torch_ee(x, edges, eel, rest, dhat2, False)[0].double().sum()

    def torch_energy_gradient():
        e0, g0, i0 = torch_pt(x, tris, ptl, dhat2, True)
        e1, g1, i1 = torch_ee(x, edges, eel, rest, dhat2, True)
        g = torch.zeros(nv, 3, dtype=f32, device="cuda")
        g.index_add_(0, i0.reshape(-1), g0.reshape(-1, 3))
        g.index_add_(0, i1.reshape(-1), g1.reshape(-1, 3))
        keep["e"], keep["g"] = e0.double().sum() + e1.double().sum(), g

    xdir = torch.from_numpy(np.random.default_rng(5).standard_normal((nv, 3)).astype(np.float32)).cuda()
    hx = torch.empty(nv, 3, dtype=f32, device="cuda")

    def product(psd):
        assert L.zs_rocm_mesh_barrier_hessian_product(*head, psd, xdir.data_ptr(), starts.data_ptr(), entries.data_ptr(), scratch.data_ptr(),
                                                      hx.data_ptr(), status.data_ptr()) == 0

    def hessian_product():
        product(0)
        keep["hx"] = hx.clone() if "hx" not in keep else keep["hx"]

    def hessian_product_psd():
        product(1)

    def torch_total(y):
        return torch_pt(y, tris, ptl, dhat2, False)[0].sum() + torch_ee(y, edges, eel, rest, dhat2, False)[0].sum()

    def torch_hessian_product():
        keep["thx"] = torch.autograd.functional.hvp(torch_total, x, xdir)[1]

    rows = dict(incidence=incidence, energy=energy, torch_energy=torch_energy, energy_gradient=energy_gradient,
                torch_energy_gradient=torch_energy_gradient, hessian_product=hessian_product, torch_hessian_product=torch_hessian_product,
                hessian_product_psd=hessian_product_psd)
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
    scale = float(keep["g"].abs().max().item())
    return dict(scene=name, vertices=nv, triangles=mesh.nt, edges=mesh.num_edges, dhat=dhat, pt_pairs=npt, ee_pairs=nee,
                incidences=4 * (npt + nee), most_incidences_at_one_vertex=int((starts[1:] - starts[:-1]).max().item()),
                times={k: stats(x_) for k, x_ in ms.items()},
                check=dict(energy=float(total.item()), torch_energy=float(keep["e"].item()), largest_gradient=scale,
                           largest_gradient_difference=float((grad - keep["g"]).abs().max().item()),
                           largest_product=float(keep["hx"].abs().max().item()),
                           largest_product_difference=float((keep["hx"] - keep["thx"]).abs().max().item()), zero_distance=status.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--sheet", type=int, default=708)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    doc = json.dumps(dict(bench="mesh_barrier", device=torch.cuda.get_device_name(0), scenes=out), indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
