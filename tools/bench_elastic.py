"""Times the mesh's internal energy (TriMesh.set_rest_shape / elastic / elastic_hessian_product: zs_rocm_mesh_set_rest_shape,
zs_rocm_mesh_elastic_{energy,gradient,hessian_product}) next to the same closed forms vectorised in torch on the GPU -- what a user had
before it -- on the two scenes of tools/bench_barrier.py:

    surface   the jittered 980 k-triangle surface (--side 700)
    sheets    two jittered sheets of about 1 M triangles each (--sheet 708)

at trial positions 0.1 mean edge length from rest.  Rows per scene, medians over --reps repetitions after --warmup, bracketed by HIP events
on the policy's stream with the policy not synchronising, library and torch alternating inside every repetition of the same process:
    rest_shape_first       zs_rocm_mesh_set_rest_shape, the first call (hinges, incidence, records; once, not a median)
    rest_shape             the same, a later call: records and vertex areas only
    energy                 zs_rocm_mesh_elastic_energy: per-element energies and the float64 total
    energy_gradient        zs_rocm_mesh_elastic_gradient: the same and the gradient through the two incidences
    hessian_product        zs_rocm_mesh_elastic_hessian_product, psd = 0
    hessian_product_psd    the same with psd = 1
    torch_energy, torch_energy_gradient, torch_hessian_product, torch_hessian_product_psd
                           gather the corners per element, the closed forms of include/zensim_rocm/elastic_device.hpp vectorised from the
                           library's own records, float64 sum, index_add_ of the per-element terms (float atomics: not reproducible)
    barrier_gradient       zs_rocm_mesh_barrier_gradient on the same mesh (dHat as in tools/bench_barrier.py), for scale
    copy                   torch copy_ of 1 GiB: the box's stream rate (read + write) the fractions below refer to
Also: the algorithmic bytes of each library row -- per element the index and position reads (a product: the direction's rows as well; a
hinge product reads no positions), the 16-byte record, the energy written and read back, the terms written and read back, the 4-byte
incidence entry per corner; per vertex two run starts and the 12-byte result -- the rate they move at and its fraction of the copy rate;
the ratio torch / library; the largest differences between the two routes (a sanity check, not a test).

    python tools/bench_elastic.py [--side 700] [--sheet 708] [--reps 20] [--warmup 3] [--out profiles/mesh_elastic.json]
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

MU, LAM, KB = 1.3, 0.7, 2e-3


def dot(a, b):
    return (a * b).sum(-1)


def torch_membrane(x, tris, rec, z, psd, grad):
    """(energy [nt], terms [nt, 3, 3] or None): the gradient terms, or with z the product terms"""
    x0, x1, x2 = (x[tris[:, k]] for k in range(3))
    B00, B01, B11, A = (rec[:, k, None] for k in range(4))
    cols = lambda y0, y1, y2: (B00 * (y1 - y0), B01 * (y1 - y0) + B11 * (y2 - y0))
    F0, F1 = cols(x0, x1, x2)
    E00, E11, E01 = 0.5 * (dot(F0, F0) - 1), 0.5 * (dot(F1, F1) - 1), 0.5 * dot(F0, F1)
    tr = E00 + E11
    S00, S11, S01 = 2 * MU * E00 + LAM * tr, 2 * MU * E11 + LAM * tr, 2 * MU * E01
    e = A[:, 0] * (MU * (E00 * E00 + E11 * E11 + 2 * E01 * E01) + 0.5 * LAM * tr * tr)
    if not grad and z is None:
        return e, None
    if z is None:
        P0, P1 = S00[:, None] * F0 + S01[:, None] * F1, S01[:, None] * F0 + S11[:, None] * F1
    else:
        T00, T01, T11 = S00, S01, S11
        if psd:
            m, hd = 0.5 * (S00 + S11), 0.5 * (S00 - S11)
            r = torch.sqrt(hd * hd + S01 * S01)
            q, lo = (m + r) / (2 * r).clamp_min(1e-30), m - r
            keep, none = m - r >= 0, m + r <= 0
            pick = lambda full, mixed: torch.where(keep, full, torch.where(none, torch.zeros_like(full), mixed))
            T00, T11, T01 = pick(S00, q * (S00 - lo)), pick(S11, q * (S11 - lo)), pick(S01, q * S01)
        dF0, dF1 = cols(*(z[tris[:, k]] for k in range(3)))
        dE00, dE11, dE01 = dot(F0, dF0), dot(F1, dF1), 0.5 * (dot(F0, dF1) + dot(F1, dF0))
        dtr = dE00 + dE11
        dS00, dS11, dS01 = 2 * MU * dE00 + LAM * dtr, 2 * MU * dE11 + LAM * dtr, 2 * MU * dE01
        P0 = T00[:, None] * dF0 + T01[:, None] * dF1 + dS00[:, None] * F0 + dS01[:, None] * F1
        P1 = T01[:, None] * dF0 + T11[:, None] * dF1 + dS01[:, None] * F0 + dS11[:, None] * F1
    t1, t2 = A * (P0 * B00 + P1 * B01), A * (P1 * B11)
    return e, torch.stack([-(t1 + t2), t1, t2], dim=1)


def torch_bending(y, hinges, k, grad):
    """(energy [nh], terms [nh, 4, 3] or None) at y (positions: the gradient; a direction: the product)"""
    w = (k[:, :, None] * y[hinges]).sum(dim=1)
    return 0.5 * KB * dot(w, w), ((KB * k)[:, :, None] * w[:, None, :] if grad else None)


def run_scene(pol, name, v, t, dhat, reps, warmup):
    L, H = zs.lib(), pol.handle
    mesh = TriMesh(pol, v, t)
    i32, f32 = torch.int32, torch.float32
    stream = torch.cuda.ExternalStream(pol.getStream()) if pol.getStream() else torch.cuda.default_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    pol.sync(False)
    with torch.cuda.stream(stream):
        first = timed(lambda: L.zs_rocm_mesh_set_rest_shape(H, mesh.handle, None))
    pol.sync(True)
    counts = mesh.set_rest_shape()
    rec, hinges, hrec, area = mesh.rest_shape()
    nt, nh, nv = mesh.nt, mesh.num_hinges, mesh.nv
    mesh.set_rest()
    prox = mesh.proximity(dhat)
    barrier = mesh.barrier(prox, dhat, 1.0)      # builds the incidence
    starts, entries, nscratch = prox._incidence
    bscratch = torch.empty(nscratch, dtype=f32, device="cuda")
    p = v[t.astype(np.int64)].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
    g = np.random.default_rng(5)
    x = torch.from_numpy((v + 0.1 * mean_edge * g.standard_normal(v.shape)).astype(np.float32)).cuda()
    z = torch.from_numpy(g.standard_normal(v.shape).astype(np.float32)).cuda()
    tris, hl = torch.from_numpy(t.astype(np.int64)).cuda(), hinges.long()
    scratch = torch.empty(9 * nt + 12 * nh, dtype=f32, device="cuda")
    te, he = torch.empty(nt, dtype=f32, device="cuda"), torch.empty(nh, dtype=f32, device="cuda")
    total, grad, hx = torch.empty((), dtype=torch.float64, device="cuda"), torch.empty(nv, 3, dtype=f32, device="cuda"), torch.empty(nv, 3, dtype=f32, device="cuda")
    status = torch.empty(2, dtype=i32, device="cuda")
    head = (H, mesh.handle, x.data_ptr(), MU, LAM, KB)
    tail = (te.data_ptr(), he.data_ptr(), total.data_ptr())
    big = torch.empty(2, 1 << 28, dtype=f32, device="cuda")
    keep = {}

    def rest_shape():
        assert L.zs_rocm_mesh_set_rest_shape(H, mesh.handle, None) == 0

    def energy():
        assert L.zs_rocm_mesh_elastic_energy(*head, *tail, status.data_ptr()) == 0

    def energy_gradient():
        assert L.zs_rocm_mesh_elastic_gradient(*head, scratch.data_ptr(), *tail, grad.data_ptr(), status.data_ptr()) == 0

    def product(psd):
        assert L.zs_rocm_mesh_elastic_hessian_product(*head, psd, z.data_ptr(), scratch.data_ptr(), hx.data_ptr(), status.data_ptr()) == 0

    def hessian_product():
        product(0)
        if "hx" not in keep:
            keep["hx"] = hx.clone()

    def hessian_product_psd():
        product(1)
        if "hpx" not in keep:
            keep["hpx"] = hx.clone()

    def torch_energy():
        keep["e"] = torch_membrane(x, tris, rec, None, False, False)[0].double().sum() + torch_bending(x, hl, hrec, False)[0].double().sum()

    def scatter(tt, ht):
        out = torch.zeros(nv, 3, dtype=f32, device="cuda")
        out.index_add_(0, tris.reshape(-1), tt.reshape(-1, 3))
        out.index_add_(0, hl.reshape(-1), ht.reshape(-1, 3))
        return out

    def torch_energy_gradient():
        e0, t0 = torch_membrane(x, tris, rec, None, False, True)
        e1, t1 = torch_bending(x, hl, hrec, True)
        keep["e"], keep["g"] = e0.double().sum() + e1.double().sum(), scatter(t0, t1)

    def torch_hessian_product():
        keep["thx"] = scatter(torch_membrane(x, tris, rec, z, False, True)[1], torch_bending(z, hl, hrec, True)[1])

    def torch_hessian_product_psd():
        keep["thpx"] = scatter(torch_membrane(x, tris, rec, z, True, True)[1], torch_bending(z, hl, hrec, True)[1])

    def barrier_gradient():
        pt, ee = prox.pt_pairs, prox.ee_pairs
        assert L.zs_rocm_mesh_barrier_gradient(H, mesh.handle, None, pt.data_ptr(), len(pt), ee.data_ptr(), len(ee), dhat, 1.0, 1, starts.data_ptr(),
                                               entries.data_ptr(), bscratch.data_ptr(), None, None, None, barrier.grad.data_ptr(), status.data_ptr()) == 0

    def copy():
        big[1].copy_(big[0])

    rows = dict(rest_shape=rest_shape, energy=energy, torch_energy=torch_energy, energy_gradient=energy_gradient,
                torch_energy_gradient=torch_energy_gradient, hessian_product=hessian_product, torch_hessian_product=torch_hessian_product,
                hessian_product_psd=hessian_product_psd, torch_hessian_product_psd=torch_hessian_product_psd, barrier_gradient=barrier_gradient,
                copy=copy)
    ms = {k: [] for k in rows}
    pol.sync(False)
    with torch.cuda.stream(stream):
        for it in range(warmup + reps):
            for k, fn in rows.items():
                dt = timed(fn)
                if it >= warmup:
                    ms[k].append(dt)
    pol.sync(True)
    pol.syncCtx()
    assert zs.lib().zs_rocm_last_error(-1) == 0
    times = {k: stats(x_) for k, x_ in ms.items()}
    med = {k: float(np.median(x_)) for k, x_ in ms.items()}
    per_vertex = 8 * nv + 8 * nv + 12 * nv      # two run starts of each incidence, the result
    corners = 4 * (3 * nt + 4 * nh)
    nbytes = dict(energy=nt * (12 + 36 + 16 + 8) + nh * (16 + 48 + 16 + 8),
                  energy_gradient=nt * (12 + 36 + 16 + 8 + 72) + nh * (16 + 48 + 16 + 8 + 96) + corners + per_vertex,
                  hessian_product=nt * (12 + 72 + 16 + 72) + nh * (16 + 48 + 16 + 96) + corners + per_vertex)
    nbytes["hessian_product_psd"] = nbytes["hessian_product"]
    copy_rate = 2 * big[0].numel() * 4 / (med["copy"] * 1e-3)
    rates = {k: dict(algorithmic_bytes=b, bytes_per_s=b / (med[k] * 1e-3), fraction_of_copy_rate=b / (med[k] * 1e-3) / copy_rate,
                     torch_over_library=med["torch_" + k] / med[k]) for k, b in nbytes.items()}
    return dict(scene=name, vertices=nv, triangles=nt, hinges=nh, counts=list(counts), rest_shape_first_ms=first, copy_bytes_per_s=copy_rate,
                times=times, rates=rates,
                check=dict(energy=float(total.item()), torch_energy=float(keep["e"].item()), largest_gradient=float(keep["g"].abs().max().item()),
                           largest_gradient_difference=float((grad - keep["g"]).abs().max().item()),
                           largest_product=float(keep["hx"].abs().max().item()),
                           largest_product_difference=float((keep["hx"] - keep["thx"]).abs().max().item()),
                           largest_psd_product_difference=float((keep["hpx"] - keep["thpx"]).abs().max().item()), overflow=status.tolist(),
                           rest_area=float(area.double().sum().item())))


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
    doc = json.dumps(dict(bench="mesh_elastic", device=torch.cuda.get_device_name(0), scenes=out), indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
