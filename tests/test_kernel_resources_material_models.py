"""The models variant of the surface stage (csrc/rpt_models.hip k_shade_models, the text of k_shade with shade_slot<.., MODELS>) as the BUILD made it: registers,
scratch and LDS read from the code objects inside librpt_hip.so (tools/kernel_resources.sh), beside the plain variant it stands in for.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# (NEE, TEXTURED, COMPACT) -> VGPRs of k_shade_models as the gfx950 build gives them (k_shade's: 61 93 80 121 / 75 115 82 123 / 74 113 82 121).  The steps of
# the occupancy are 64 / 72 / 80 / 96 / 128: the unpacked variants sit on k_shade's step, the packed textured NEE ones one step above theirs (131 and 129 > 128).
VGPRS = {(0, False, False): 62, (0, False, True): 109, (0, True, False): 80, (0, True, True): 125,
         (1, False, False): 75, (1, False, True): 122, (1, True, False): 82, (1, True, True): 131,
         (2, False, False): 74, (2, False, True): 120, (2, True, False): 82, (2, True, True): 129}


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


@pytest.mark.parametrize("key", sorted(VGPRS))
def test_the_models_variant_is_built_without_scratch(shade_kernels, key):
    rows, plain = shade_kernels.get(_name("k_shade_models", key), []), shade_kernels.get(_name("k_shade", key), [])
    assert len(rows) == 1 and len(plain) == 1, sorted(shade_kernels)
    vgpr, sgpr, scratch, lds = rows[0]
    print(f"{_name('k_shade_models', key)}: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds (k_shade: {plain[0]})")
    assert scratch == 0 and plain[0][2] == 0
    assert lds <= plain[0][3]
    assert vgpr == VGPRS[key]


def test_there_are_twelve_of_each(shade_kernels):
    assert sorted(k for k in shade_kernels if k.startswith("k_shade_models<")) == sorted(_name("k_shade_models", k) for k in VGPRS)
    assert sorted(k for k in shade_kernels if k.startswith("k_shade<")) == sorted(_name("k_shade", k) for k in VGPRS)
