"""Resource bounds of the fused step's block kernel with the in-block mover path (zpc_amd/csrc/mpm_slotblk.hip): the ticket counters of
all eight bins of a block live in LDS for the workgroup's whole life, and two workgroups of 512 threads must still fit one CU
(160 KiB of LDS: at most 81 920 bytes each)."""
import os
import re
import subprocess

import pytest


def _notes(tmp_path, obj_name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "zpc_amd", "lib", "obj", obj_name)
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(obj) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("object file or llvm tools not present")
    fat, co = str(tmp_path / "p.fat"), str(tmp_path / "p.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat,
                           "--output=" + co, "--unbundle"])
    return subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], stdout=subprocess.PIPE, check=True).stdout.decode()


def test_block_kernel_keeps_two_workgroups_per_cu_of_lds(tmp_path):
    notes = _notes(tmp_path, "mpm_slotblk.o")
    seen = 0
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or "g2p2g_slotblk_kernel" not in name.group(1):
            continue
        seen += 1
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert lds <= 81920, (name.group(1), lds)
        assert int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", blk).group(1)) == 512, name.group(1)
    assert seen == 10  # five models x {write everything, write the step's state only}
