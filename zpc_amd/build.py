"""Build script: compiles every HIP source under zpc_amd/csrc into zpc_amd/lib/libzsrocm.so for gfx950
(hipcc cross-compiles without a GPU) and the CPU parity checker under oracle/ (test infrastructure).

    python -m zpc_amd.build [--force]
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "zpc_amd", "lib")
LIB = os.path.join(LIBDIR, "libzsrocm.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-gpu-rdc",
         "-Wno-unused-result", "-I", os.path.join(ROOT, "include")]


# per-file flags.  mpm.hip: the SLP vectoriser packs independent scalar f32 ops of the per-lane 3x3 SVD / stencil code
# into v_pk_*_f32 (same FLOP rate as two scalar ops on CDNA4) and pays ~25 % extra v_mov to form the register pairs:
# 901 -> 772 instructions and ~2390 -> ~1540 issue cycles for the SVD alone (MI355X guide, 5.6: "an anti-lever").
EXTRA_FLAGS = {"mpm_slotted.hip": ["-fno-slp-vectorize"], "mpm_slotblk.hip": ["-fno-slp-vectorize"], "mpm.hip": ["-fno-slp-vectorize"], "mpm_p2g.hip": ["-fno-slp-vectorize"], "mpm_g2p.hip": ["-fno-slp-vectorize"],
               "mpm_c2.hip": ["-fno-slp-vectorize"], "mpm_implicit.hip": ["-fno-slp-vectorize"],
               "mpm_fused.hip": ["-fno-slp-vectorize"], "mpm_fused4.hip": ["-fno-slp-vectorize"], "mpm_fused8.hip": ["-fno-slp-vectorize"],
               # morton codes must round like the reference's scalar code (no fused centre/offset arithmetic)
               "lbvh.hip": ["-ffp-contract=off"],
               # finite-difference normals of the analytic colliders (eps = 1e-6 in float) must round like the reference's
               "collider.hip": ["-ffp-contract=off"], "mpm_implicit_project.hip": ["-ffp-contract=off"],
               # the level-set normal is a float central difference at +- h / 4 (include/zensim_rocm/levelset_device.hpp)
               "levelset.hip": ["-ffp-contract=off"],
               # the transition between two level sets: the tests reproduce its float32 chain up to the displaced sample points
               "levelset_transition.hip": ["-ffp-contract=off"],
               # point-triangle distances and pseudonormal signs (include/zensim_rocm/distance_device.hpp): a float32 chain in numpy
               # reproduces the discrete decisions (region, nearest triangle, sign) only without fused multiply-adds
               "mesh.hip": ["-ffp-contract=off"],
               # tri_closest / ee_closest behind the proximity walks: the same chains, the same reason
               "mesh_proximity.hip": ["-ffp-contract=off"],
               # the barrier potential on those pairs (include/zensim_rocm/barrier_device.hpp) recomputes the same distances; friction
               # (friction_device.hpp) lags them, and its evaluation is replayed bit for bit in numpy
               "mesh_barrier.hip": ["-ffp-contract=off"],
               # additive CCD on those pairs (include/zensim_rocm/ccd_device.hpp) advances on the same distances
               "mesh_ccd.hip": ["-ffp-contract=off"],
               # membrane and bending energy (include/zensim_rocm/elastic_device.hpp): replayed bit for bit in numpy
               "mesh_elastic.hip": ["-ffp-contract=off"],
               # the gather and the total behind those terms: float32 and float64 sums that the tests replay addition by addition
               "mesh_terms.hip": ["-ffp-contract=off"],
               # the Newton system on those terms (include/zensim_rocm/solve_device.hpp): blocks, operator and solve are replayed bit for bit
               "mesh_solve.hip": ["-ffp-contract=off"],
               # the incremental potential on those terms (include/zensim_rocm/potential_device.hpp): energy, gradient and the line search's
               # decisions are replayed bit for bit
               "mesh_potential.hip": ["-ffp-contract=off"]}


def _newer(src, dst):
    return (not os.path.exists(dst)) or os.path.getmtime(src) > os.path.getmtime(dst)


def build_hip(force=False, verbose=True):
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    face = os.path.join(ROOT, "include", "zensim_rocm")
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "zs_rocm.h")] \
        + [os.path.join(face, f) for f in os.listdir(face) if f.endswith("_device.hpp")]
    objs, procs = [], []
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s[:-4] + ".o")
        objs.append(obj)
        if force or _newer(src, obj) or any(_newer(h, obj) for h in hdrs) or _newer(os.path.abspath(__file__), obj):
            cmd = [HIPCC] + FLAGS + EXTRA_FLAGS.get(s, []) + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((s, subprocess.Popen(cmd)))
    for s, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on %s" % s)
    if force or procs or not os.path.exists(LIB):
        # librccl: the multi-GPU exchange steps (csrc/dist.hip) call RCCL directly
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-L/opt/rocm/lib", "-lrccl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


# Test programs under tests/cpp, each a user translation unit written against the header-only C++ face (include/zensim_rocm) and linked
# against libzsrocm.so: name -> extra compiler flags.
#   test_cpp_face   proves that the face compiles with hipcc and links the library
#   test_ofb        the face compiled with ZS_ENABLE_OFB_ACCESS_CHECK=1 (the reference's bounds-check build option)
#   test_levelset   Collider{sparseGridView, type}.resolveCollision in a user lambda against the C ABI's level-set entries; built without
#                   FP contraction like every translation unit that evaluates a level set
#   test_mesh       TriMeshView::signed_distance / closest_point in a user lambda against the C ABI's bulk entries; built without FP
#                   contraction like every translation unit that uses the point-triangle distance
#   test_transition TransitionLevelSetView{viewA, viewB, stepDt, alpha} and Collider over it in a user lambda against the C ABI's transition
#                   entries; without FP contraction for the same reason
CPP_TESTS = {"test_cpp_face": ["-munsafe-fp-atomics"], "test_ofb": [], "test_levelset": ["-ffp-contract=off"], "test_mesh": ["-ffp-contract=off"],
             "test_transition": ["-ffp-contract=off"]}


def build_cpp_test(name, verbose=True):
    """Compile tests/cpp/<name>.hip (a key of CPP_TESTS) against the C++ face and libzsrocm.so into zpc_amd/lib/<name>; returns that path."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".hip")
    out = os.path.join(LIBDIR, name)
    face = os.path.join(ROOT, "include", "zensim_rocm")
    deps = [src, LIB] + [os.path.join(face, f) for f in os.listdir(face) if f.endswith(".hpp")]
    if os.path.exists(src) and any(_newer(d, out) for d in deps):
        cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17"] + CPP_TESTS[name] + ["-I", os.path.join(ROOT, "include"), src,
               "-L", LIBDIR, "-lzsrocm", "-Wl,-rpath,$ORIGIN", "-o", out]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


def build_cpp_tests(verbose=True):
    return [build_cpp_test(name, verbose) for name in CPP_TESTS]


def build_oracle(verbose=True):
    """CPU restatement (always) and, where /root/reference exists, the in-place build of the reference's
    header-only numerics (oracle/_ref).  Building the checker is not using it."""
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-s", "-C", odir, "libzpc_oracle.so"])
    if os.path.isdir("/root/reference/include/zensim"):
        subprocess.call(["make", "-s", "-C", odir, "ref"])


if __name__ == "__main__":
    force = "--force" in sys.argv
    print(build_hip(force=force))
    build_cpp_tests()
    build_oracle()
