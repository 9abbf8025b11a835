"""Times the mesh Newton system (zpc_amd.mesh_solve.MeshSystem: zs_rocm_mesh_system_{blocks,multiply,solve}) on the two scenes of
tools/bench_barrier.py:

    surface   the jittered 980 k-triangle surface (--side 700)
    sheets    two jittered sheets of about 1 M triangles each (--sheet 708)

at trial positions 0.1 mean edge length from rest, with all three terms (elastic, barrier, friction; masses of DENSITY x vertex area).  Rows
per scene, medians over --reps repetitions after --warmup, bracketed by HIP events on the policy's stream with the policy not
synchronising, library and comparator alternating inside every repetition of the same process:
    blocks                 zs_rocm_mesh_system_blocks: element blocks, gathers, combine and inverse
    multiply               zs_rocm_mesh_system_multiply: the three products' element kernels and one gather
    three_products         the three existing zs_rocm_mesh_*_hessian_product calls, psd, one after the other (no combine)
    pcg_iteration_1 / _8   zs_rocm_mesh_system_solve over --iters iterations (tolerances 0, so every iteration runs) with check_every 1
                           and 8, divided by the iterations
    torch_pcg_iteration    the same block-Jacobi PCG composed in torch from the three public TriMesh.*_hessian_product calls, the library's
                           own inverse blocks and .item() scalars -- what a user had before -- over --iters iterations, divided by them
Also, once per scene: the iterations the device solve needs to rel_tol = --rel-tol with the block-Jacobi preconditioner and with the
identity in its place (plain CG), capped at --cap.

    python tools/bench_solve.py [--side 700] [--sheet 708] [--reps 10] [--warmup 2] [--iters 40] [--out profiles/mesh_solve.json]
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
from zpc_amd.mesh_solve import MeshSystem  # noqa: E402
from bench_mesh_levelset import jittered_surface  # noqa: E402
from bench_proximity import two_sheets, stats  # noqa: E402

DENSITY, SCALE, MU, LAM, KB, KAPPA, FRICTION_MU, EPS_V = 1e3, 1e-2, 1.3e3, 0.7e3, 2e-3, 1e3, 0.3, 1e-3


def run_scene(pol, name, v, t, dhat, a):
    L, H = zs.lib(), pol.handle
    mesh = TriMesh(pol, v, t)
    f32 = dict(dtype=torch.float32, device="cuda")
    stream = torch.cuda.ExternalStream(pol.getStream()) if pol.getStream() else torch.cuda.default_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    mesh.set_rest()
    mesh.set_rest_shape()
    area = mesh.rest_shape()[3]
    prox = mesh.proximity(dhat)
    lag = mesh.friction_lag(prox, dhat, KAPPA)
    nv = mesh.nv
    p = v[t.astype(np.int64)].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
    g = np.random.default_rng(5)
    x = torch.from_numpy((v + 0.1 * mean_edge * g.standard_normal(v.shape)).astype(np.float32)).cuda()
    u = torch.from_numpy((0.1 * EPS_V * g.standard_normal(v.shape)).astype(np.float32)).cuda()
    z = torch.from_numpy(g.standard_normal(v.shape).astype(np.float32)).cuda()
    b = torch.from_numpy(g.standard_normal(v.shape).astype(np.float32)).cuda()
    mass = (DENSITY * area).contiguous()
    S = MeshSystem(mesh, mass, SCALE, elastic=(MU, LAM, KB), barrier=(prox, dhat, KAPPA), friction=(lag, FRICTION_MU, EPS_V))
    counts = S.linearize(x, u)
    B = S.blocks()
    d, scratch = C.byref(S._desc), S._scratch.data_ptr()
    pt, ee = prox.pt_pairs, prox.ee_pairs
    starts, entries, nscratch = prox._incidence
    escratch, pscratch = torch.empty(mesh._elastic_scratch, **f32), torch.empty(nscratch, **f32)
    q, hx = torch.empty(nv, 3, **f32), [torch.empty(nv, 3, **f32) for _ in range(3)]
    blk = [torch.empty(nv, 6, **f32) for _ in range(5)]
    status = torch.empty(8, dtype=torch.int32, device="cuda")
    xs = torch.zeros(nv, 3, **f32)
    record = torch.empty(3 + max(a.iters, a.cap), dtype=torch.int32, device="cuda")
    keep = {}

    def blocks():
        assert L.zs_rocm_mesh_system_blocks(H, mesh.handle, d, scratch, *(t_.data_ptr() for t_ in blk), status.data_ptr()) == 0

    def multiply():
        assert L.zs_rocm_mesh_system_multiply(H, mesh.handle, d, scratch, z.data_ptr(), q.data_ptr()) == 0

    def three_products():
        assert L.zs_rocm_mesh_elastic_hessian_product(H, mesh.handle, x.data_ptr(), MU, LAM, KB, 1, z.data_ptr(), escratch.data_ptr(), hx[0].data_ptr(),
                                                      status.data_ptr()) == 0
        assert L.zs_rocm_mesh_barrier_hessian_product(H, mesh.handle, x.data_ptr(), pt.data_ptr(), len(pt), ee.data_ptr(), len(ee), dhat, KAPPA, 1, 1,
                                                      z.data_ptr(), starts.data_ptr(), entries.data_ptr(), pscratch.data_ptr(), hx[1].data_ptr(),
                                                      status.data_ptr()) == 0
        assert L.zs_rocm_mesh_friction_hessian_product(H, mesh.handle, u.data_ptr(), z.data_ptr(), pt.data_ptr(), len(pt), ee.data_ptr(), len(ee),
                                                       lag.record.data_ptr(), FRICTION_MU, EPS_V, starts.data_ptr(), entries.data_ptr(),
                                                       pscratch.data_ptr(), hx[2].data_ptr(), status.data_ptr()) == 0

    def solve(inverse, iters, rel_tol, check_every):
        xs.zero_()
        assert L.zs_rocm_mesh_system_solve(H, mesh.handle, d, scratch, inverse.data_ptr(), b.data_ptr(), xs.data_ptr(), iters, 0.0 if rel_tol == 0 else 3e38,
                                           rel_tol, check_every, record.data_ptr()) == 0

    def apply(Bi, r):
        return torch.stack([Bi[:, 0] * r[:, 0] + Bi[:, 1] * r[:, 1] + Bi[:, 2] * r[:, 2], Bi[:, 1] * r[:, 0] + Bi[:, 3] * r[:, 1] + Bi[:, 4] * r[:, 2],
                            Bi[:, 2] * r[:, 0] + Bi[:, 4] * r[:, 1] + Bi[:, 5] * r[:, 2]], dim=1)

    def torch_multiply(w):
        h = mesh.elastic_hessian_product(MU, LAM, KB, w, verts=x, psd=True).hx + mesh.barrier_hessian_product(prox, dhat, KAPPA, w, verts=x, psd=True).hx
        return mass[:, None] * w + SCALE * (h + mesh.friction_hessian_product(lag, u, FRICTION_MU, EPS_V, w).hx)

    def torch_pcg():
        xt = torch.zeros(nv, 3, **f32)
        r = b - torch_multiply(xt)
        zt = apply(B.inverse, r)
        pv = zt.clone()
        rz = (r.double() * zt.double()).sum().item()
        for _ in range(a.iters):
            qv = torch_multiply(pv)
            alpha = rz / (pv.double() * qv.double()).sum().item()
            xt += alpha * pv
            r -= alpha * qv
            zt = apply(B.inverse, r)
            rz1 = (r.double() * zt.double()).sum().item()
            pv = zt + (rz1 / rz) * pv
            rz = rz1
        keep["torch_x"] = xt

    def pcg_1():
        solve(B.inverse, a.iters, 0.0, 1)

    def pcg_8():
        solve(B.inverse, a.iters, 0.0, 8)
        keep["x"] = xs.clone()

    rows = dict(blocks=blocks, multiply=multiply, three_products=three_products, pcg_1=pcg_1, torch_pcg=torch_pcg, pcg_8=pcg_8)
    ms = {k: [] for k in rows}
    pol.sync(False)
    with torch.cuda.stream(stream):
        for it in range(a.warmup + a.reps):
            for k, fn in rows.items():
                dt = timed(fn)
                if it >= a.warmup:
                    ms[k].append(dt)
        # iterations to the tolerance, with the block-Jacobi preconditioner and with the identity in its place
        iters = {}
        identity = torch.zeros(nv, 6, **f32)
        identity[:, [0, 3, 5]] = 1
        for label, inv in (("block_jacobi", B.inverse), ("none", identity)):
            solve(inv, a.cap, a.rel_tol, 8)
            pol.syncCtx()
            rec = record.cpu().numpy()
            iters[label] = dict(iters=int(rec[0]), flag=int(rec[1]), res0=float(rec[2:3].view(np.float32)[0]),
                                res=float(rec[2 + int(rec[0]):3 + int(rec[0])].view(np.float32)[0]))
    pol.sync(True)
    pol.syncCtx()
    assert zs.lib().zs_rocm_last_error(-1) == 0
    times = {k: stats(x_) for k, x_ in ms.items()}
    for k in ("pcg_1", "pcg_8", "torch_pcg"):
        times[k + "_per_iteration_ms"] = times[k]["median_ms"] / a.iters
    diff = float((keep["x"] - keep["torch_x"]).abs().max().item()) / max(float(keep["x"].abs().max().item()), 1e-30)
    return dict(scene=name, vertices=nv, triangles=mesh.nt, hinges=mesh.num_hinges, pt_pairs=len(pt), ee_pairs=len(ee),
                counts={k: getattr(counts, k) for k in counts.__slots__}, iterations_timed=a.iters, times=times,
                multiply_over_three_products=times["multiply"]["median_ms"] / times["three_products"]["median_ms"],
                torch_over_library_per_iteration=times["torch_pcg"]["median_ms"] / times["pcg_8"]["median_ms"],
                iterations_to_rel_tol=dict(rel_tol=a.rel_tol, cap=a.cap, **iters), relative_difference_to_torch_after_timed_iterations=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--sheet", type=int, default=708)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rel-tol", type=float, default=1e-3, dest="rel_tol")
    ap.add_argument("--cap", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    pol = zs.rocm_exec()
    out = []
    v, t = jittered_surface(a.side)
    p = v[t.astype(np.int64)].astype(np.float64)
    mean_edge = float(np.mean([np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=1).mean() for k in range(3)]))
    out.append(run_scene(pol, "surface", v, t, float(np.float32(0.5 * mean_edge)), a))
    v, t, h = two_sheets(a.sheet)
    out.append(run_scene(pol, "sheets", v, t, float(np.float32(h)), a))
    doc = json.dumps(dict(bench="mesh_solve", device=torch.cuda.get_device_name(0), scenes=out), indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
