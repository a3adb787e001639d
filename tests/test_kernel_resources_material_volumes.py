"""The volumes variant of the surface stage (csrc/rpt_volumes.hip k_shade_volumes, the text of k_shade with shade_slot<.., MODELS, VOLUMES>) as the BUILD made
it: registers, scratch and LDS read from the code objects inside librpt_hip.so (tools/kernel_resources.sh), beside the models variant it stands in for.
No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# (NEE, TEXTURED, COMPACT) -> VGPRs of k_shade_volumes as the gfx950 build gives them (k_shade_models': 62 109 80 125 / 75 122 82 131 / 74 120 82 129: the three
# exps of vol_transmit run through rpt_math.h's f64 core).  The steps of the occupancy are 64 / 72 / 80 / 96 / 128 (8 / 7 / 6 / 5 / 4 waves per SIMD): ten of
# the twelve sit on k_shade_models' step; the two unpacked no-NEE ones go one step up — 70 > 64 (7 waves for 8) and 82 > 80 (5 for 6, where the unpacked
# textured NEE variants of k_shade_models already are).
VGPRS = {(0, False, False): 70, (0, False, True): 117, (0, True, False): 82, (0, True, True): 127,
         (1, False, False): 75, (1, False, True): 125, (1, True, False): 82, (1, True, True): 132,
         (2, False, False): 74, (2, False, True): 123, (2, True, False): 82, (2, True, True): 132}
STEPS = (64, 72, 80, 96, 128, 168, 256, 512)
STEP_UP = {(0, False, False), (0, True, False)}              # one occupancy step above k_shade_models'


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
def test_the_volumes_variant_is_built_without_scratch(shade_kernels, key):
    rows, models = shade_kernels.get(_name("k_shade_volumes", key), []), shade_kernels.get(_name("k_shade_models", key), [])
    assert len(rows) == 1 and len(models) == 1, sorted(shade_kernels)
    vgpr, sgpr, scratch, lds = rows[0]
    print(f"{_name('k_shade_volumes', key)}: {vgpr} vgpr, {sgpr} sgpr, {scratch} scratch, {lds} lds (k_shade_models: {models[0]})")
    assert scratch == 0 and models[0][2] == 0
    assert lds <= models[0][3]
    assert vgpr == VGPRS[key]
    assert _step(vgpr) - _step(models[0][0]) == (1 if key in STEP_UP else 0)


def test_there_are_twelve(shade_kernels):
    assert sorted(k for k in shade_kernels if k.startswith("k_shade_volumes<")) == sorted(_name("k_shade_volumes", k) for k in VGPRS)
