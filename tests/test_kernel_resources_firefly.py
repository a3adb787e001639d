"""The kernels of the firefly clamp (csrc/k_firefly.h k_dn_prepare_var_clamp, k_dn_temporal_clamp) as the BUILD made them: registers, scratch and LDS read from
the code objects inside librpt_hip.so (tools/kernel_resources.sh); and the kernels they stand in for, still there under their names.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def denoise_kernels():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB, "k_dn_"], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            name = re.sub(r"^void |\(anonymous namespace\)::", "", m.group(5).strip()).split("(")[0]
            table.setdefault(name, []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


@pytest.mark.parametrize("name,vgpr_max", [("k_dn_prepare_var_clamp", 29), ("k_dn_temporal_clamp", 49)])
def test_the_clamp_kernels_are_built_without_scratch(denoise_kernels, name, vgpr_max):
    """both instantiations (uniform count, own counts) of each: no scratch, no spills, the staged window's 70 x 10 entries of 8 bytes in LDS and nothing else there,
    and the VGPR count the build showed when they were written — 29 for the pre-pass, 49 for the fused temporal kernel, which is k_dn_temporal's own 49"""
    for own in ("true", "false"):
        rows = denoise_kernels.get(f"{name}<{own}>", [])
        assert len(rows) == 1, sorted(denoise_kernels)
        vgpr, sgpr, scratch, lds = rows[0]
        print(f"{name}<{own}>: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds")
        assert scratch == 0 and lds == 70 * 10 * 8 and vgpr <= vgpr_max


def test_the_kernels_they_stand_in_for_keep_their_names(denoise_kernels):
    for name in ("k_dn_prepare_var", "k_dn_temporal"):
        for own in ("true", "false"):
            rows = denoise_kernels.get(f"{name}<{own}>", [])
            assert len(rows) == 1 and rows[0][2] == 0, (name, sorted(denoise_kernels))
