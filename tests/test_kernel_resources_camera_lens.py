"""The kernels of the thin-lens camera (csrc/rpt_lens.hip) as the BUILD made them: registers, scratch and LDS read from the code objects inside
librpt_hip.so (tools/kernel_resources.sh).  Resources only, no instruction text.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# VGPRs as the build gives them.  The completion kernels carry lens_ray (a sqrt, a sincos, two normalisations) inside the restart loop, which costs 7
# registers over the builds they were compiled from (k_complete 86, k_complete_moments 94): k_lens_complete_moments sits above the 96 its parent is held to,
# 4 waves per SIMD instead of 5, in a one-wave-per-chunk kernel that waits on memory.
VGPRS = {"k_generate_lens": 29, "k_lens_complete": 93, "k_lens_complete_moments": 101, "k_dn_camera_rays_lens": 18, "k_lens_rays": 19}
COMPILED_FROM = {"k_generate_lens": "k_generate_first", "k_lens_complete": "k_complete", "k_lens_complete_moments": "k_complete_moments", "k_dn_camera_rays_lens": "k_dn_camera_rays"}


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            table.setdefault(m.group(5).strip().split("(")[0], []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_the_lens_kernels_exist_once_without_scratch(kernels, name):
    assert len(kernels.get(name, [])) == 1, sorted(k for k in kernels if "lens" in k)
    vgpr, sgpr, scratch, lds = kernels[name][0]
    print(f"{name}: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds")
    assert scratch == 0
    assert vgpr == VGPRS[name]


@pytest.mark.parametrize("name", sorted(COMPILED_FROM))
def test_static_lds_is_that_of_the_kernel_it_was_compiled_from(kernels, name):
    """(the completion kernels' tile is dynamic: 0 static bytes in all four)"""
    assert len(kernels[COMPILED_FROM[name]]) == 1
    assert kernels[name][0][3] == kernels[COMPILED_FROM[name]][0][3]
    assert kernels["k_lens_rays"][0][3] == 0
