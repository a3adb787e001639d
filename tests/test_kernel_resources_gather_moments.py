"""The two kernels of the gather's second wire format (csrc/k_gather.h k_gather_pack, k_gather_untile2) as the BUILD made them: registers, scratch and LDS
read from the code objects inside librpt_hip.so (tools/kernel_resources.sh).  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def gather_kernels():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB, "k_gather_"], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            name = re.sub(r"^void |\(anonymous namespace\)::", "", m.group(5).strip()).split("(")[0]
            table.setdefault(name, []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


@pytest.mark.parametrize("name", ["k_gather_pack", "k_gather_untile2"])
def test_the_gather_kernels_are_built_once_without_scratch_or_lds(gather_kernels, name):
    """one copy of each (rpt_comm.hip alone emits them), no scratch, no LDS, and the 10 VGPRs the build showed when they were written: a float4 in flight,
    an index and two addresses"""
    rows = gather_kernels.get(name, [])
    assert len(rows) == 1, (name, sorted(gather_kernels))
    vgpr, sgpr, scratch, lds = rows[0]
    print(f"{name}: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds")
    assert scratch == 0 and lds == 0 and vgpr <= 10
