"""CPU tests (no GPU): the C-ABI library loads and exports every symbol include/zs_rocm.h declares; host-side
logic (policy object, domain decomposition, halo exchange over gloo with world_size 2)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from util import LLVM_BIN, code_object_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(hiplib):
    pp = subprocess.check_output(["gcc", "-E", "-P", os.path.join(ROOT, "include", "zs_rocm.h")]).decode()
    names = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", pp))
    names = {n for n in names if not n.startswith("__") and n != "visibility"}
    assert len(names) > 300
    missing = [n for n in sorted(names) if not hasattr(hiplib, n)]
    assert not missing, missing


def test_policy_object_defaults_and_setters(hiplib):
    import zpc_amd as zs
    p = zs.rocm_exec()
    assert p.shouldSync() is True                      # execution/ExecutionPolicy.hpp:125
    assert p.sync(False).shouldSync() is False         # fluent setters return *this&
    assert p.profile(True).device(0).stream(3).listen(-1, -1).shmem(1024).block(128) is p
    assert zs.mem_enum if hasattr(zs, "mem_enum") else True
    assert hiplib.mem_enum__host() == 0 and hiplib.mem_enum__device() == 1 and hiplib.mem_enum__um() == 2


def test_missing_library_fails_loudly(monkeypatch):
    import zpc_amd._lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libzsrocm.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.lib()


def test_domain_decomposition_boxes():
    from zpc_amd.dist import cell_box, split_dims, shared_keys
    lo, hi = (192, 0, 192), (317, 512, 317)
    for w in (1, 2, 4, 8):
        boxes = [cell_box(r, w, lo, hi, align=4) for r in range(w)]
        vol = sum(np.prod(np.array(b[1]) - np.array(b[0])) for b in boxes)
        assert vol == np.prod(np.array(hi) - np.array(lo))       # a partition of the global box
        for b in boxes:
            for d in range(3):
                assert b[0][d] == lo[d] or b[0][d] % 4 == 0       # cuts on block boundaries
        assert np.prod(split_dims(w)) == w
    a = np.array([[0, 0, 1], [5, 2, 3], [1, 1, 1], [-1, 0, 2]], np.int32)
    b = np.array([[1, 1, 1], [9, 9, 9], [-1, 0, 2]], np.int32)
    s = shared_keys(a, b)
    assert np.array_equal(s, np.array([[-1, 0, 2], [1, 1, 1]], np.int32))
    assert np.array_equal(s, shared_keys(b, a))                   # same order on both sides


def test_boundary_first_block_mask():
    """near_shared_mask: the blocks within two blocks of a block another rank also holds (they are numbered and launched
    first so that their ghost sums can travel while the interior computes); key units = block side (stride)."""
    from zpc_amd.dist import near_shared_mask
    k0 = np.array([[x, y, z] for x in range(0, 9) for y in range(3) for z in (0, 1)], np.int32)   # rank 0: x < 9, ghost layer 8
    k1 = np.array([[x, y, z] for x in range(7, 16) for y in range(3) for z in (0, 1)], np.int32)  # rank 1: x >= 7, ghost layer 7
    for stride in (1, 4, 8):
        m0 = near_shared_mask(k0 * stride, [k0 * stride, k1 * stride], 0, stride)
        m1 = near_shared_mask(k1 * stride, [k0 * stride, k1 * stride], 1, stride)
        assert sorted(set(k0[m0][:, 0].tolist())) == [5, 6, 7, 8] and sorted(set(k0[~m0][:, 0].tolist())) == [0, 1, 2, 3, 4]
        assert sorted(set(k1[m1][:, 0].tolist())) == [7, 8, 9, 10]
    assert not near_shared_mask(k0, [k0, k1 + 100], 0, 1).any()      # nothing shared -> nothing is boundary
    assert near_shared_mask(k0[:0], [k0[:0], k1], 0, 1).shape == (0,)


_WORKER = r"""
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
from zpc_amd.dist import HaloExchange
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=world)
nc, bf = 8, 7 * 8
# two ranks, overlapping block sets; grid value = f(key, channel, cell, rank)
keys = {0: np.array([[0,0,0],[1,0,0],[2,0,0],[3,0,0]], np.int32), 1: np.array([[5,0,0],[3,0,0],[2,0,0]], np.int32)}[rank]
grid = torch.zeros(len(keys), 7, nc)
for i, k in enumerate(keys):
    grid[i] = float(k[0]) * 100 + torch.arange(7).reshape(7, 1) * 10 + torch.arange(nc).reshape(1, nc) + (rank + 1) * 1000
orig = grid.clone()
def lookup(sk):
    m = {tuple(k): i for i, k in enumerate(keys)}
    return np.array([m[tuple(k)] for k in sk], np.int64)
h = HaloExchange(dist, rank, world, keys, lookup, lambda x: torch.from_numpy(x.astype(np.int64)), lambda m: torch.zeros(max(m, 1)), bf)
def pack(blocks, nb, buf): buf[: nb * bf] = grid[blocks].reshape(-1)
def unpack_add(blocks, nb, buf): grid.index_add_(0, blocks, buf[: nb * bf].reshape(nb, 7, nc))
h.exchange(pack, unpack_add)
other = 1 - rank
for i, k in enumerate(keys):
    if k[0] in (2, 3):   # shared blocks hold the two-way total
        exp = orig[i] + (orig[i] - (rank + 1) * 1000 + (other + 1) * 1000)
    else:
        exp = orig[i]
    assert torch.allclose(grid[i], exp), (rank, k)
assert len(h.peers) == 1 and h.peers[0][2] == 2 and h.total_blocks == 2 and h.bytes_per_exchange == 2 * bf * 4
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_halo_exchange_gloo_world2(tmp_path):
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % {"root": ROOT, "port": port})
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=120)
        assert p.returncode == 0, out.decode()


def test_hiprtc_compile_without_gpu(tmp_path):
    """rocm_compile_program (py_interop/cuda/Nvrtc.cpp:29-146 over hiprtc) cross-compiles gfx950 with no device present;
    a broken source reports a non-zero hiprtc result instead of writing a file."""
    from zpc_amd import jit
    out = str(tmp_path / "k.hsaco")
    src = 'extern "C" __global__ void twice(float *x, unsigned long n) { unsigned long i = blockIdx.x * (unsigned long)blockDim.x + threadIdx.x; if (i < n) x[i] *= 2.f; }'
    assert jit.compile_program(src, out, arch=950) == out
    assert os.path.getsize(out) > 1000 and open(out, "rb").read(4) == b"\x7fELF"
    bad = str(tmp_path / "bad.hsaco")
    with pytest.raises(RuntimeError):
        jit.compile_program("this is not HIP", bad, arch=950)
    assert not os.path.exists(bad)


def test_abi_struct_layouts_match_the_reference(tmp_path):
    """Every POD the C ABI hands across the boundary (by value or through a pyview__ pointer) has the byte layout of the
    reference's own struct: tests/golden/abi_layout.json is derived from the reference's py_interop headers compiled in place
    (tools/gen_abi_layout.sh -- VectorViewLite, TileVectorViewLite, TileVectorNamedViewLite, BhtViewLite dim 1-4 x B 16/32,
    aosoa_iterator_port); here the structs of include/zs_rocm.h are measured with the host compiler and compared member by member.
    A JIT kernel compiled against the reference's view headers reads these objects directly."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_layout.json")))
    ours = {
        "VectorViewLite<int>": ("zs_rocm_vector_view_lite", ["_vector"]),
        "TileVectorViewLite<float,32>": ("zs_rocm_tv_view_lite", ["_vector", "_numChannels"]),
        "TileVectorNamedViewLite<float,32>": ("zs_rocm_tv_named_view_lite", ["_vector", "_numChannels", "_tagNames", "_tagOffsets", "_tagSizes", "_N"]),
        "aosoa_iterator_port<float,1>": ("aosoa_iterator_float_1", ["base", "idx", "numTileBits", "tileMask", "numChns"]),
        "aosoa_iterator_port<float,3>": ("aosoa_iterator_float_3", ["base", "idx", "numTileBits", "tileMask", "numChns"]),
        "aosoa_iterator_port<const double,1>": ("aosoa_iterator_const_double_1", ["base", "idx", "numTileBits", "tileMask", "numChns"]),
    }
    bht_members = ["keys", "indices", "status", "activeKeys", "cnt", "success", "tableSize", "numBuckets", "hf0x", "hf0y", "hf1x", "hf1y",
                   "hf2x", "hf2y"]
    for d in (1, 2, 3, 4):
        for b in (16, 32):
            ours["BhtViewLite<int,%d,int,%d>" % (d, b)] = ("zs_rocm_bht_view_lite", bht_members)
    assert set(ours) == set(want)
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "zs_rocm.h"', 'int main(void) {']
    for ref_name, (cname, members) in ours.items():
        src.append('  printf("%s|size|%%zu|%%zu\\n", sizeof(%s), (size_t)_Alignof(%s));' % (ref_name, cname, cname))
        for m in members:
            src.append('  printf("%s|%s|%%zu|%%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (ref_name, m, cname, m, cname, m))
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        s, m, a, b = line.split("|")
        got.setdefault(s, {})[m] = [int(a), int(b)]
    for ref_name, w in want.items():
        g = got[ref_name]
        assert g["size"] == [w["size"], w["align"]], (ref_name, g["size"], w["size"], w["align"])
        for m, ob in w["members"].items():
            assert g[m] == ob, (ref_name, m, g[m], ob)
    # the ctypes mirror used by the tests / bench agrees with the header
    from zpc_amd._lib import BhtViewLite
    for m in bht_members:
        f = getattr(BhtViewLite, m)
        assert [f.offset, f.size] == want["BhtViewLite<int,3,int,16>"]["members"][m], m
    assert C.sizeof(BhtViewLite) == want["BhtViewLite<int,3,int,16>"]["size"]


def test_ctypes_mirrors_of_the_mpm_structs_match_the_header(tmp_path):
    """zpc_amd/_lib.py mirrors the PODs of the MPM path by hand (the tests and bench.py fill them through ctypes): every field of every mirror
    sits at the offset and has the size the host compiler gives the member of the same name in include/zs_rocm.h, and the structs are
    as large -- a field added to one side only (zs_rocm_mpm_step grew haloChannels and rangeSchedule in r06) fails here, on CPU."""
    from zpc_amd import _lib
    pairs = {"zs_rocm_mpm_step": _lib.MpmStep, "zs_rocm_slot_storage": _lib.SlotStorage, "zs_rocm_mpm_params": _lib.MpmParams,
             "zs_rocm_particles": _lib.Particles, "zs_rocm_collider": _lib.Collider, "aosoa_iterator_float_1": _lib.Port,
             "zs_rocm_hashtable_view": _lib.HashTableView, "zs_rocm_lbvh_view": _lib.LBvhView, "zs_rocm_index_buckets_view": _lib.IndexBucketsView}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "zs_rocm.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        src.append('  printf("%s|size|%%zu|0\\n", sizeof(%s));' % (cname, cname))
        for m, _ in cls._fields_:
            src.append('  printf("%s|%s|%%zu|%%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (cname, m, cname, m, cname, m))
    src += ['  return 0;', '}']
    c = tmp_path / "mirrors.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "mirrors"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        sname, m, a, b = line.split("|")
        got.setdefault(sname, {})[m] = [int(a), int(b)]
    for cname, cls in pairs.items():
        assert C.sizeof(cls) == got[cname]["size"][0], (cname, C.sizeof(cls), got[cname]["size"][0])
        for m, _ in cls._fields_:
            f = getattr(cls, m)
            assert [f.offset, f.size] == got[cname][m], (cname, m, [f.offset, f.size], got[cname][m])
    assert _lib.lib is not None and (_lib.MpmStep.rangeSchedule.offset > _lib.MpmStep.haloChannels.offset)
    from zpc_amd import mpm
    hdr = open(os.path.join(ROOT, "include", "zs_rocm.h")).read()
    for name, val in (("ZS_ROCM_RANGES_IN_TURN", mpm.RANGES_IN_TURN), ("ZS_ROCM_RANGES_SIDE_BY_SIDE", mpm.RANGES_SIDE_BY_SIDE), ("ZS_ROCM_RANGES_ONE_LAUNCH", mpm.RANGES_ONE_LAUNCH)):
        assert "#define %s %d\n" % (name, val) in hdr


def test_native_halo_plan_matches_the_python_plan():
    """zs_rocm_halo_plan_from_keys (host part of the native multi-GPU set-up, callable without a GPU) against the numpy construction
    HaloExchange uses: same peers, same per-peer block lists in the same (lexicographic key) order, for every rank of random
    overlapping partitions; both sides of every pair list the same keys in the same order."""
    from zpc_amd.dist import halo_plan_from_keys, shared_keys
    rng = np.random.default_rng(11)
    for world in (1, 2, 5):
        allk = []
        for r in range(world):
            k = np.unique(rng.integers(-6, 7, (int(rng.integers(0, 160)), 3)).astype(np.int32) * 8, axis=0)
            allk.append(k[rng.permutation(k.shape[0])])  # block-number order is not key order
        plans = [halo_plan_from_keys(allk, r) for r in range(world)]
        for r in range(world):
            peers, blocks = plans[r]
            want = []
            for p in range(world):
                if p == r:
                    continue
                sk = shared_keys(allk[r], allk[p])
                if sk.shape[0]:
                    want.append((p, sk))
            assert [p for p, _, _ in peers] == [p for p, _ in want]
            off = 0
            for (p, o, c), (_, sk) in zip(peers, want):
                assert o == off and c == sk.shape[0]
                assert np.array_equal(allk[r][blocks[o:o + c]], sk)  # my block numbers, in the shared (sorted) key order
                # the peer lists the same keys in the same order
                pp, pb = plans[p]
                q = [x for x in pp if x[0] == r][0]
                assert np.array_equal(allk[p][pb[q[1]:q[1] + q[2]]], sk)
                off += c
            assert blocks.shape[0] == off


def test_halo_plan_of_the_full_column_on_2x2x2_ranks():
    """BASELINE config 4's decomposition: the 128 x 512 x 128-cell column at dx = 1/512 on 8 ranks as 2 x 2 x 2.
    Every rank's partition = the blocks of its particles' base nodes, EnlargeSparsity{0, 2} (simulation/sparsity/SparsityOp.hpp:89-115), plus
    `margin` blocks of travel room.  The native plan (zs_rocm_halo_plan_from_keys) gives every rank 7 peers; the ghost-block sums of one
    exchange are 25.6 MB with the reference's partition (margin 0) and 72.5 MB with the one block of travel room the slotted storage
    runs with (bench.py --margin 1) -- the figures DESIGN 7 quotes."""
    from zpc_amd.dist import cell_box, halo_plan_from_keys, set_split_dims, split_dims
    side = 8
    glo = ((512 - 128) // 2 // side * side, 0, (512 - 128) // 2 // side * side)
    ghi = (glo[0] + 128, 512, glo[2] + 128)
    assert tuple(split_dims(8)) == (2, 2, 2)

    def keys(rank, margin):
        lo, hi = cell_box(rank, 8, glo, ghi, align=side)
        b0 = [(lo[d] - 1) // side - margin for d in range(3)]          # base nodes of the particles in cells [lo, hi): lo - 1 .. hi - 1
        b1 = [(hi[d] - 1) // side + 1 + margin for d in range(3)]
        return np.stack(np.meshgrid(*[np.arange(b0[d], b1[d] + 1) for d in range(3)], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    for margin, mb in ((0, 25.6), (1, 72.5)):
        allk = [keys(r, margin) for r in range(8)]
        for r in range(8):
            peers, blocks = halo_plan_from_keys(allk, r)
            assert len(peers) == 7 and sorted(p for p, _, _ in peers) == [q for q in range(8) if q != r]
            assert abs(blocks.shape[0] * 7 * side ** 3 * 4 / 1e6 - mb) < 0.1, (margin, r, blocks.shape[0])


def test_small_input_sort_kernels_use_no_scratch_memory(tmp_path):
    """The three kernels of the small-input radix sort must not use private (scratch) memory in any instantiation: two builds that did
    (a __noinline__ device function; spilled VGPRs) sorted correctly but made a later, unrelated kernel on the same queue return wrong
    results ("radix sort, up to 2 M 4-byte keys").  Read from the built code object's metadata."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "zpc_amd", "lib", "obj", "primitives.o")
    found = code_object_kernels(obj, tmp_path)
    if found is None:
        pytest.skip("object file or llvm tools not present")
    kernels, co = found
    seen = 0
    for name, meta, _ in kernels:
        if "radix_small" not in name:
            continue
        seen += 1
        assert int(meta[".private_segment_fixed_size"]) == 0, name
        assert meta[".uses_dynamic_stack"] == "false", name
    assert seen >= 12  # hist x 4 key types, split and finish x 4 key types x {keys, pairs} (minus duplicates the linker folds)


def test_merge_sort_kernels_of_the_cpp_face_use_no_scratch_memory(tmp_path):
    """The merge sort instantiated by the C++ face's test program -- int keys, pairs, and a 16-byte struct key with a user comparator --
    keeps its per-lane run in registers: r03 / r04 carried a "scratch trap" (a kernel with private memory followed by
    the struct-key merge kernels, 176 B of scratch per lane, returned wrong results in two builds that could not be reproduced later).
    r05 removed the private memory from the merge kernels (merge_sort.hpp: serial_merge); this keeps it removed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "zpc_amd", "lib", "test_cpp_face")
    found = code_object_kernels(exe, tmp_path)
    if found is None:
        pytest.skip("test program or llvm tools not present")
    kernels, co = found
    seen = 0
    for name, meta, _ in kernels:
        if "zs_rocm_ms" not in name:
            continue
        seen += 1
        assert int(meta[".private_segment_fixed_size"]) == 0, name
    assert seen >= 6  # tile sort, partition and merge kernels for int keys, pairs and the struct key


def test_block_kernel_of_the_fused_step_keeps_its_chunk_loop_free_of_scratch(tmp_path):
    """g2p2g_slotblk_kernel runs at 128 VGPRs (two workgroups of 8 waves per CU).  Until r05's second pass 12-14 hoisted loop invariants did
    not fit and were reloaded from scratch inside the chunk loop: on gfx9 loads and stores share vmcnt, so every such reload waited for the
    record prefetch of the next chunk and for the particle stores (profiles/r05_block_kernel.md, section 7: 6.52 -> 6.33 ms/step once they
    were gone).  The solid models' instantiations must stay at zero private memory, and the kernel's code must stay one producer body
    (the wave number is a run-time value: 54 KB, not 87-94 KB)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "zpc_amd", "lib", "obj", "mpm_slotblk.o")
    found = code_object_kernels(obj, tmp_path)
    if found is None:
        pytest.skip("object file or llvm tools not present")
    kernels, co = found
    seen = 0
    for name, meta, _ in kernels:
        m = re.search(r"g2p2g_slotblk_kernelILi(\d)ELb", name)
        if not m or int(m.group(1)) > 3:  # 0 fixed-corotated, 1 DruckerPrager, 2 von Mises, 3 NACC (4 = the fluid: not covered)
            continue
        seen += 1
        assert int(meta[".private_segment_fixed_size"]) == 0, name
        assert int(meta[".vgpr_count"]) <= 128, name
    assert seen == 8  # four models x {write everything, write the step's state only}
    sizes = [size for name, _, size in kernels if "g2p2g_slotblk_kernelILi1ELb0" in name]
    assert sizes and max(sizes) < 64 * 1024, sizes


def test_tile_kernel_of_the_standalone_p2g_keeps_its_accumulators_in_registers_and_its_requests_in_assembly(tmp_path):
    """p2g_tile_kernel (the kernel north_star's 0.60 is measured on) holds 27 x 7 node sums per lane at two waves per SIMD: one spilled
    register puts scratch traffic into the record stream.  And its tile requests must reach the object as the inline-assembly
    `global_load_lds_dwordx4`: through the builtin the compiler puts `s_waitcnt vmcnt(0)` in front of every round's first LDS read and the
    ring never holds a tile in flight (profiles/r06_p2g.md: 1.65 against 1.50 ms) -- so inside the record loop no `s_waitcnt vmcnt(0)` may sit
    directly in front of a `ds_read`."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "zpc_amd", "lib", "obj", "mpm_p2g.o")
    found = code_object_kernels(obj, tmp_path)
    if found is None:
        pytest.skip("object file or llvm tools not present")
    kernels, co = found
    seen = 0
    for name, meta, _ in kernels:
        if "p2g_tile_kernel" not in name:
            continue
        seen += 1
        assert int(meta[".private_segment_fixed_size"]) == 0, name
        assert int(meta[".vgpr_spill_count"]) == 0, name
        assert int(meta[".vgpr_count"]) <= 256, name
    assert seen >= 4  # 8^3 blocks (two bins per workgroup) and 4^3 blocks, merged and per-attribute requests
    dis = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", co], stdout=subprocess.PIPE, check=True).stdout.decode()
    m = re.search(r"<_ZN3zsrL15p2g_tile_kernelILi8ELi3ELi2ELb1E[^>]*>:\n(.*?)s_endpgm", dis, re.S)
    assert m, "p2g_tile_kernel<8, 3, 2, true> not found"
    lines = [l.split("//")[0].strip() for l in m.group(1).splitlines() if l.strip()]
    req = [i for i, l in enumerate(lines) if l.startswith("global_load_lds_dwordx4")]
    assert len(req) == 12, len(req)  # 4 + 2 requests per tile, at the head of the wave and inside the record loop
    loop = lines[req[6]:]
    first_flush = next(i for i, l in enumerate(loop) if l.startswith("ds_write_b128"))   # the arena clear: the record loop ends before it
    for i, l in enumerate(loop[:first_flush]):
        if l.startswith("ds_read"):
            prev = next(x for x in reversed(loop[:i]) if not x.startswith("s_nop"))
            assert not prev.startswith("s_waitcnt vmcnt(0)"), "a vmcnt(0) sits in front of an LDS read of the record loop"

