"""Static instruction counts of the streamed LDS walks after their control was flattened (k_walk.h lds_stream_walk_run), no GPU: a fresh
`-S` build of rpt_traverse.hip with the Makefile's flags goes through tools/walk_overhead_count.py, and the regions the write-up names are compared with the parent's
table kept in profiles/r22_walk_scalar_static_parent.txt.  Nothing is pinned to today's compiler: every number is read from the tool's output, and what is asserted is
the rule the change was made by — at 3.7 units per vector and 6.5 per scalar instruction (profiles/r04_valu_pipes.txt, question 3) a region's cost goes down, and so
does its scalar count."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "walk_overhead_count.py")
PARENT = os.path.join(ROOT, "profiles", "r22_walk_scalar_static_parent.txt")
KERNELS = ["k_traverse_nearest_stream<16, 1024, 0>", "k_traverse_nearest_stream<16, 1024, 1>", "k_traverse_nearest_stream<16, 1024, 2>",
           "k_traverse_shadow_stream<16, 1024, false>", "k_traverse_shadow_stream<16, 1024, true>",
           "k_traverse_shadow_stream_seg<16, 1024, false>", "k_traverse_shadow_stream_seg<16, 1024, true>"]
REGIONS = ["loop head", "inner body", "push / pop", "leaf set-up", "triangle iteration", "inner trip, total"]
VALU_UNITS, SALU_UNITS = 3.7, 6.5


def parse(text):
    """{kernel: {'fast' | 'ieee': {region: (VALU, SALU, VALU units, SALU units)}}}"""
    out, kernel, form = {}, None, None
    for line in text.splitlines():
        if line.startswith("k_traverse"):
            kernel, form = line.strip(), None
            out[kernel] = {}
        m = re.match(r"\s+walk loop \S+ \((\w+)\)", line)
        if m:
            form = m.group(1)
            out[kernel][form] = {}
        m = re.match(r"\s+(loop head|inner body|push / pop|leaf set-up|triangle iteration|inner trip, total)\s+(\d+)\s+(\d+)\s+\d+\s+\d+\s+([\d.]+)\s+([\d.]+)\s*$", line)
        if m and form:
            out[kernel][form][m.group(1)] = (int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5)))
        if line.strip().startswith("refill loop"):
            form = None
    return out


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    make = open(os.path.join(ROOT, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS := (.*?)\n(?!\s)", make, re.S | re.M).group(1).replace("\\\n", " ").split()
    asm = tmp_path_factory.mktemp("walk_static") / "rpt_traverse.s"
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", str(asm), os.path.join(ROOT, "rust-path-tracer_amd", "csrc", "rpt_traverse.hip")],
                   check=True, capture_output=True)
    new = subprocess.run([sys.executable, TOOL, str(asm)], check=True, capture_output=True, text=True).stdout
    return parse(open(PARENT).read()), parse(new)


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_regions_and_their_unit_sums(tables, kernel):
    parent, new = tables
    for table in (parent, new):
        walk = table[kernel]["fast"]
        assert sorted(walk) == sorted(REGIONS)
        for valu, salu, vu, su in walk.values():
            assert vu == pytest.approx(VALU_UNITS * valu, abs=0.06) and su == pytest.approx(SALU_UNITS * salu, abs=0.06)
        trip = [sum(walk[r][k] for r in REGIONS[:3]) for k in (0, 1)]
        assert tuple(trip) == walk["inner trip, total"][:2]


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_walk_of_the_streamed_lanes_pays_by_the_unit_costs(tables, kernel):
    parent, new = tables
    p, n = parent[kernel]["fast"], new[kernel]["fast"]
    leaf = lambda w: tuple(w["leaf set-up"][k] + w["triangle iteration"][k] for k in (0, 1))
    for name, (pv, ps), (nv, ns) in (("inner trip, total", p["inner trip, total"][:2], n["inner trip, total"][:2]), ("leaf trip", leaf(p), leaf(n))):
        print(f"{kernel} {name}: VALU {pv} -> {nv}, SALU {ps} -> {ns}, units {VALU_UNITS * pv + SALU_UNITS * ps:.1f} -> {VALU_UNITS * nv + SALU_UNITS * ns:.1f}")
        assert SALU_UNITS * (ns - ps) + VALU_UNITS * (nv - pv) < 0, name
        assert ns < ps, name
    # the scalar port is no longer the longer one on an inner trip (it was: 48 x 6.5 against 82 x 3.7)
    assert SALU_UNITS * n["inner trip, total"][1] < VALU_UNITS * n["inner trip, total"][0]
