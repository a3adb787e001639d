"""The completion kernel of a context with moments on (csrc/k_complete.h k_complete_moments) as the BUILD made it: registers, scratch and LDS read from
the code objects inside librpt_hip.so (tools/kernel_resources.sh), held to the limits tests/test_kernel_resources.py::test_completion_kernel holds
k_complete to.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def completion_kernels():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB, "k_complete"], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            table.setdefault(m.group(5).strip().split("(")[0], []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


def test_the_moments_completion_kernel_is_built_within_the_limits_of_k_complete(completion_kernels):
    """one wave per chunk, eight radiance rows in flight in scalars plus the four words of the moments record: at most 96 VGPRs, no scratch, no static LDS
    (the tile is dynamic)"""
    assert list(completion_kernels.get("k_complete_moments", [])) != [], sorted(completion_kernels)
    for vgpr, sgpr, scratch, lds in completion_kernels["k_complete_moments"]:
        print(f"k_complete_moments: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds")
        assert vgpr <= 96 and scratch == 0 and lds == 0


def test_the_plain_completion_kernel_keeps_its_name(completion_kernels):
    """k_complete is still a plain kernel under that name (not a template instantiation, which would print as `void k_complete<...>`), and the two are
    the only completion kernels of the library"""
    assert sorted(completion_kernels) == ["k_complete", "k_complete_moments"], sorted(completion_kernels)
    assert len(completion_kernels["k_complete"]) == 1 and len(completion_kernels["k_complete_moments"]) == 1
    for vgpr, sgpr, scratch, lds in completion_kernels["k_complete"]:
        assert vgpr <= 96 and scratch == 0 and lds == 0
