"""The punctual variant of the surface stage (csrc/rpt_punctual.hip k_shade_punctual, the text of k_shade with shade_slot<.., MODELS, VOLUMES, PUNCTUAL>) as the
BUILD made it: registers, scratch and LDS read from the code objects inside librpt_hip.so (tools/kernel_resources.sh), beside the volumes variant it stands
in for.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# (NEE, TEXTURED, COMPACT) -> VGPRs of k_shade_punctual as the gfx950 build gives them (k_shade_volumes': 75 125 82 132 / 74 123 82 132).  The steps of the
# occupancy are 64 / 72 / 80 / 96 / 128 / 168 (8 / 7 / 6 / 5 / 4 / 3 waves per SIMD).  Every one of the eight sits on k_shade_volumes' step for the same key:
# 77 and 75 <= 80 where 75 and 74 are, 82 <= 96, 128 and 127 <= 128 where 125 and 123 are, 136 and 138 <= 168 where 132 is.
VGPRS = {(1, False, False): 77, (1, False, True): 128, (1, True, False): 82, (1, True, True): 136,
         (2, False, False): 75, (2, False, True): 127, (2, True, False): 82, (2, True, True): 138}
STEPS = (64, 72, 80, 96, 128, 168, 256, 512)


@pytest.fixture(scope="module")
def shade_kernels():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB, "k_shade"], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            name = re.sub(r"^void ", "", m.group(5).strip()).split("(")[0]
            table.setdefault(name, []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


def _name(kernel, key):
    nee, textured, compact = key
    return f"{kernel}<{nee}, {str(textured).lower()}, {str(compact).lower()}>"


def _step(vgpr):
    return next(i for i, s in enumerate(STEPS) if vgpr <= s)


@pytest.mark.parametrize("key", sorted(VGPRS))
def test_the_punctual_variant_is_built_without_scratch(shade_kernels, key):
    rows, volumes = shade_kernels.get(_name("k_shade_punctual", key), []), shade_kernels.get(_name("k_shade_volumes", key), [])
    assert len(rows) == 1 and len(volumes) == 1, sorted(shade_kernels)
    vgpr, sgpr, scratch, lds = rows[0]
    print(f"{_name('k_shade_punctual', key)}: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds (k_shade_volumes: {volumes[0]})")
    assert scratch == 0 and volumes[0][2] == 0
    assert lds == volumes[0][3]                        # no static LDS beyond k_shade_volumes'
    assert vgpr == VGPRS[key]
    assert _step(vgpr) == _step(volumes[0][0])         # the occupancy step of k_shade_volumes for the same key


def test_there_are_eight(shade_kernels):
    """NEE modes 1 and 2 only: with nee = 0 the other variants are launched, and no k_shade_punctual<0, ..> is built"""
    assert sorted(k for k in shade_kernels if k.startswith("k_shade_punctual<")) == sorted(_name("k_shade_punctual", k) for k in VGPRS)
