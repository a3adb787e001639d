"""The kernel of the window rule (csrc/k_adaptive.h k_ad_window) as the BUILD made it: registers, scratch and LDS read from the code objects inside
librpt_hip.so (tools/kernel_resources.sh); and the kernels of the ordered compaction it feeds, still there under their names.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def adaptive_kernels():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB, "k_ad_"], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            name = re.sub(r"^void |\(anonymous namespace\)::", "", m.group(5).strip()).split("(")[0]
            table.setdefault(name, []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


def test_the_window_kernel_is_built_without_scratch(adaptive_kernels):
    """no scratch, no spills; in LDS the tile's 64 row words of 64 bits twice — the `above` mask, and its rows dilated across, which the dilation down reads —
    1024 bytes and nothing else; and the 20 VGPRs the build showed when it was written.  (A kernel that is not a template is emitted by every translation unit
    that includes the header, as k_ad_scan is: every copy is held to the same figures.)"""
    rows = adaptive_kernels.get("k_ad_window", [])
    assert rows, sorted(adaptive_kernels)
    for vgpr, sgpr, scratch, lds in rows:
        print(f"k_ad_window: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds")
        assert scratch == 0 and lds == 2 * 64 * 8 and vgpr <= 20


def test_the_compaction_kernels_keep_their_names(adaptive_kernels):
    for name in ("k_ad_count<AdMaskSel>", "k_ad_count<AdNoiseSel>", "k_ad_count<AdFlagSel>"):
        rows = adaptive_kernels.get(name, [])
        assert len(rows) == 1 and rows[0][2] == 0, (name, sorted(adaptive_kernels))
    for name in ("k_ad_scan", "k_ad_scatter", "k_ad_scatter_back"):
        rows = adaptive_kernels.get(name, [])
        assert rows and all(r[2] == 0 for r in rows), (name, sorted(adaptive_kernels))
