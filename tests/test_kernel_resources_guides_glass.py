"""The kernels of the guides that follow glass (csrc/k_guides_glass.h) as the BUILD made them: registers, scratch and LDS read from the code objects inside
librpt_hip.so (tools/kernel_resources.sh), beside the first-hit kernel they stand beside.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# kernel -> (VGPRs, LDS bytes) as the gfx950 build gives them.  k_dn_shade_guides<true> / <false> have 54 / 38: the untextured step is in its occupancy class
# (up to 64 registers: 8 waves per SIMD), the textured one a step below (72: 7 waves) — it carries the chain and the refraction beside the two atlas lookups.
KERNELS = {"k_dn_glass_step<true>": (72, 16), "k_dn_glass_step<false>": (53, 16), "k_dn_glass_scan": (26, 1024), "k_dn_glass_scatter": (14, 16)}


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB, "k_dn_"], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            name = re.sub(r"^void ", "", m.group(5).strip()).split("(")[0]
            table.setdefault(name, []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_the_kernels_exist_without_scratch_and_with_the_measured_registers(kernels, name):
    rows = kernels.get(name, [])
    assert len(rows) == 1, sorted(kernels)
    vgpr, sgpr, scratch, lds = rows[0]
    print(f"{name}: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds")
    assert scratch == 0
    assert (vgpr, lds) == KERNELS[name]


def test_the_first_hit_kernel_is_still_there(kernels):
    for name in ("k_dn_shade_guides<true>", "k_dn_shade_guides<false>"):
        assert len(kernels.get(name, [])) == 1 and kernels[name][0][2] == 0
    assert kernels["k_dn_glass_step<false>"][0][0] <= 64
