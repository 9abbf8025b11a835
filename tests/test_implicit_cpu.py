"""The implicit-MPM system without a GPU: its symbols, the float64 reference's own consistency, the inputs of the GPU tests, and the
binned force kernel's private-memory use."""
import os
import re
import subprocess

import numpy as np
import pytest

import ref64
import ref64_implicit as ri
from util import OracleMpm, oracle_stress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["zs_rocm_mpm_implicit_force", "zs_rocm_mpm_implicit_multiply", "zs_rocm_mpm_implicit_project", "zs_rocm_mpm_implicit_precondition",
           "zs_rocm_mpm_implicit_solve", "zs_rocm_dof_assign", "zs_rocm_dof_fill", "zs_rocm_dof_compwise", "zs_rocm_dof_linear_combine",
           "zs_rocm_dof_dot"]
METHODS = ["dof_vector", "implicit_force", "implicit_multiply", "implicit_project", "implicit_precondition", "implicit_solve"]


def test_implicit_symbols_are_declared_exported_and_bound(hiplib):
    header = open(os.path.join(ROOT, "include", "zs_rocm.h")).read()
    from zpc_amd.mpm import MpmTransfer
    for s in SYMBOLS:
        assert re.search(r"ZS_ROCM_EXPORT\s+(int|void)\s+%s\(" % s, header), s + " is not declared in zs_rocm.h"
        assert getattr(hiplib, s) is not None
        assert getattr(hiplib, s).argtypes is not None, s + " has no ctypes signature"
    for m in METHODS:
        assert callable(getattr(MpmTransfer, m, None)), "MpmTransfer.%s is missing" % m


@pytest.mark.parametrize("cloud", ri.CLOUDS)
def test_reference_force_sums_to_zero_within_its_own_bound(cloud):
    """sum_i W_ip (x_i - x_p) = 0 for the quadratic B-spline, so each force component summed over all nodes is 0 whatever P F^T vol is:
    the float64 scatter must satisfy that within the sum of its node bounds before a GPU result is judged by them.
    The identity needs weights and offsets taken at the same local position.  The edge cloud holds the particles for which they are not:
    where X - fl rounds lpn up to 1.5 (or X - 0.5 to an integer), d0 = lpn - floor(lpn - 0.5) weights the particle one cell away on the
    unchanged corner (ref64's docstring; the reference and the kernels do the same), and since sum_k w_k(d0) k = d0 the first moment of
    such a particle is (d0 - lpn) dx instead of 0.  So the sum is compared with sum_p D_inv (P F^T vol)_p (d0 - lpn)_p dx, which is
    exactly 0 for a cloud without such particles."""
    m, x, v, Cm, F, lj = ri.implicit_case(cloud, 0)
    PF = (50.0 * ri.DX ** 3 * np.random.default_rng(7).standard_normal((x.shape[0], 9))).astype(np.float32)
    ref = ri.force64(PF, x, ri.DX)
    _, lpn, d0 = ref64.arena32(x, ri.DX)
    shift = (d0.astype(np.float64) - lpn.astype(np.float64)) * ri.DX                      # [n, 3], 0 unless the arena rounded
    want = 4.0 / ri.DX ** 2 * np.einsum("ndj,nj->d", ref64._mat(PF), shift)
    if cloud != "edge":
        assert (shift == 0).all() and (want == 0).all()
    else:
        assert (shift != 0).any()
    total = np.abs(ref.val[:, 4:7].sum(0) - want)
    budget = ref.bound()[:, 4:7].sum(0)
    print("IMPLICIT ref64 force sum %s: |sum - moment| %s, summed bound %s, moment %s, largest |f| %.3g"
          % (cloud, total, budget, want, np.abs(ref.val[:, 4:7]).max()))
    assert (ref.val[:, :4] == 0).all() and (ref.N >= 1).all()
    assert np.abs(ref.val[:, 4:7]).max() > 0
    assert (total <= budget).all()


@pytest.mark.parametrize("cloud", ri.CLOUDS)
@pytest.mark.parametrize("model", [0, 1, 2, 3, 4])
def test_oracle_stress_is_finite_on_every_trial_state(oracle, model, cloud):
    """the inputs of the GPU force test: the float64 F_trial (J_trial) of every particle, rounded to float32, has a finite oracle stress
    for all five models, so that test compares every particle (no mask); dt |C| is about a per cent"""
    m, x, v, Cm, state, lj = ri.implicit_case(cloud, model)
    nodes = ri.stencil_nodes(x)
    r = ri.trial64((nodes, ri.trial_velocity(nodes, ri.cloud_centre(x), scale=ri.TRIAL_SCALE[cloud])), x, state, model)
    dtC = ri.DT * np.abs(r["C"]).max(1)
    assert 0.0005 < np.median(dtC) and dtC.max() < 0.05   # (the edge cloud's maximum: particles whose arena rounded, see trial_velocity)
    om = OracleMpm(oracle, model, ri.DX, ri.DT, 8, ri.DX ** 3 / 8, **ri.model_kw(model))
    Ft = np.zeros((x.shape[0], 9), np.float32)
    if model == 4:
        Ft[:, 0] = r["J"].astype(np.float32)
    else:
        Ft[:] = r["F"].astype(np.float32)
    PF = oracle_stress(oracle, om, r["C"].astype(np.float32), Ft, lj if model in (1, 3) else None)
    assert np.isfinite(PF).all(), "%d particles without a finite oracle stress" % int((~np.isfinite(PF).all(1)).sum())


def test_binned_implicit_force_kernel_uses_no_scratch_memory(tmp_path):
    """implicit_block_kernel keeps its 27 x 3 node sums and the constitutive update in registers in every instantiation (5 models x 2
    sides x 3 particle layouts): read from the code object's metadata"""
    obj = os.path.join(ROOT, "zpc_amd", "lib", "obj", "mpm_implicit.o")
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(obj):  # not built yet: compile the translation unit the way zpc_amd/build.py does
        from zpc_amd import build as b
        obj = str(tmp_path / "mpm_implicit.o")
        subprocess.check_call([b.HIPCC] + b.FLAGS + b.EXTRA_FLAGS["mpm_implicit.hip"] + ["-c", os.path.join(b.CSRC, "mpm_implicit.hip"), "-o", obj])
    fat, co = str(tmp_path / "p.fat"), str(tmp_path / "p.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                           "--output=" + co, "--unbundle"])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], stdout=subprocess.PIPE, check=True).stdout.decode()
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or "implicit_block_kernel" not in name.group(1):
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name.group(1)
        assert re.search(r"\.uses_dynamic_stack:\s+(\w+)", blk).group(1) == "false", name.group(1)
    assert seen == 30
