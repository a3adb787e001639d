"""The occupancy the hot kernels were tuned for is a property of the BUILD: registers, scratch and LDS per kernel, read from the
code objects inside librpt_hip.so (tools/kernel_resources.sh).  No GPU needed.

Why these numbers: the streamed LDS walks run two 1 024-thread workgroups per CU = 8 waves per SIMD, which needs
<= 64 VGPRs and 32 KB of static LDS (+ the scene image); the plain shade stage and the streamed global-memory walks of thin-leaf
scenes ask the compiler for 8 waves per SIMD too; nothing on the hot path may spill."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def resources():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            table.setdefault(m.group(5).strip(), []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    assert len(table) > 40
    return table


def _find(table, prefix):
    hits = [v for k, vs in table.items() if k.startswith(prefix) for v in vs]
    assert hits, prefix
    return hits


@pytest.mark.parametrize("kernel", ["void k_traverse_nearest_stream<16, 1024, 0>", "void k_traverse_nearest_stream<16, 1024, 1>", "void k_traverse_nearest_stream<16, 1024, 2>", "void k_traverse_shadow_stream<16, 1024, false>", "void k_traverse_shadow_stream<16, 1024, true>"])
def test_streamed_lds_walks_fit_two_workgroups_per_cu(resources, kernel):
    for vgpr, sgpr, scratch, lds in _find(resources, kernel):
        assert vgpr <= 64 and scratch == 0
        assert sgpr <= 80                     # 82 halves the occupancy (k_walk_stream.h RPT_LDS_WALK_SGPRS): measured, not reported by the occupancy API
        assert lds <= 32 * 1024 + 64          # 16-bit stacks of 16 waves + the pool; the scene image (<= 32 KB) is dynamic


@pytest.mark.parametrize("kernel", ["void k_shade<0, false, false>", "void k_traverse_nearest_gstream<24, 16, false>",
                                    "void k_traverse_shadow_gstream<24, 16, false, false>", "void k_traverse_shadow_gstream<24, 16, false, true>", "void k_traverse_nearest_gstream<16, 16, false>",
                                    "void k_traverse_nearest_gstream<32, 21, false>", "void k_traverse_shadow_gstream<32, 21, false, false>", "void k_traverse_shadow_gstream<32, 21, false, true>"])
def test_eight_waves_per_simd_where_asked(resources, kernel):
    for vgpr, sgpr, scratch, lds in _find(resources, kernel):
        assert vgpr <= 64 and sgpr <= 80 and scratch == 0


def test_no_kernel_of_the_library_spills(resources):
    """Round 3 left two (the cooperative nearest-hit walk with 24-bit stack entries asked for 8 waves per SIMD and spilled three registers);
    they ask for 7 now.  A spill in any kernel — stage, set-up, debug — fails the build check."""
    bad = {k: v for k, vs in resources.items() for v in vs if v[2] != 0}
    assert not [k for k in resources if "rocprim" in k]                   # (rounds 4-5 carried rocPRIM's radix sort: 156 kernels, half of the library; round 6 sorts with its own three)
    assert not bad, bad


@pytest.mark.parametrize("kernel,vgpr_max", [("void k_shade<1, false, false>", 80), ("void k_shade<1, false, true>", 120), ("void k_shade<0, false, true>", 96),
                                             ("void k_shade<2, false, false>", 80), ("void k_sky<false>", 96)])
def test_registers_of_the_nee_and_packed_shade_variants_do_not_creep(resources, kernel, vgpr_max):
    """What the round-3 counters were taken on (round 5, with the last-bounce paths in: k_shade<1, false, false> 75, <1, false, true> 115, <0, false, true> 93, k_sky<false> 94 VGPRs):
    a register more can cost a wave per SIMD (the steps are 64 / 72 / 80 / 96 / 128), so the ceilings are pinned to the step each sits under."""
    for vgpr, sgpr, scratch, lds in _find(resources, kernel):
        assert vgpr <= vgpr_max and scratch == 0


@pytest.mark.parametrize("kernel,vgpr_max", [("void k_shade<0, true, false>", 96), ("void k_shade<0, true, true>", 128), ("void k_shade<1, true, false>", 96),
                                             ("void k_shade<1, true, true>", 128), ("void k_shade<2, true, false>", 96), ("void k_shade<2, true, true>", 128)])
def test_registers_of_the_textured_shade_variants(resources, kernel, vgpr_max):
    """The TEXTURED variants (BASELINE config[3] as written; round 6: first counters): 84 / 119 / 82 / 123 / 82 / 123 VGPRs, 5 and 4 waves per SIMD, no scratch,
    the packed variants' 8 KB of list + a few words of LDS."""
    for vgpr, sgpr, scratch, lds in _find(resources, kernel):
        assert vgpr <= vgpr_max and scratch == 0 and lds <= 8472


def test_completion_kernel(resources):
    """k_complete (k_path.h): one wave per chunk, its LDS tile is dynamic (0 at q_shift = 0, up to 35 KB otherwise), eight radiance rows in flight
    in scalars — an array of float4 there stays in scratch behind its 16-byte copies (found in round 6)."""
    for vgpr, sgpr, scratch, lds in _find(resources, "k_complete"):
        assert vgpr <= 96 and scratch == 0 and lds == 0


def test_no_stage_kernel_of_the_shipped_scenes_spills(resources):
    """every kernel a shipped scene (or the two stand-ins) launches: no scratch"""
    for prefix in ("void k_shade<0, false, ", "void k_shade<1, false, ", "void k_shade<2, false, ", "void k_shade<0, true, ", "void k_shade<1, true, ", "void k_shade<2, true, ", "void k_sky<", "k_generate_first", "k_complete",
                   "k_shadow_resolve", "void k_traverse_nearest_gstream<32, 16, true>", "void k_traverse_shadow_gstream<32, 16, true, "):
        for vgpr, sgpr, scratch, lds in _find(resources, prefix):
            assert scratch == 0, prefix


def test_scalar_cache_path_of_the_global_walks_survives_the_compiler(tmp_path):
    """The wave-uniform node visit of the streamed nearest-hit walk (k_walk.h children_uniform) lives on two things the optimiser undid when it
    was first written: the scalar load with scalar-operand slab tests behind it (sunk into a common tail it needs fourteen v_mov), and the vector
    loads staying on the other side of the branch (hoisted above it they are issued on every step).  Checked in the ISA of the built library: the
    kernel holds s_load_dwordx16, v_sub_f32 with a scalar first operand right behind it, and no vector load between the uniformity test and it."""
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    import shutil
    work = tmp_path / "isa"
    work.mkdir()
    shutil.copy(LIB, work / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=work, capture_output=True, check=True)
    co = [f for f in os.listdir(work) if "gfx950" in f]
    assert co
    text = "".join(subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", one], cwd=work, capture_output=True, text=True, check=True).stdout for one in sorted(co))     # (one code object per translation unit)
    m = re.search(r"<_Z26k_traverse_nearest_gstreamILi24ELi16ELb0EEv[^>]*>:\n(.*?)s_endpgm", text, re.S)
    assert m, "kernel not found in the disassembly"
    lines = [l.strip() for l in m.group(1).splitlines() if l.startswith("\t")]
    at = [i for i, l in enumerate(lines) if l.startswith("s_load_dwordx16")]
    assert len(at) >= 1                                                     # (the exact-division and the IEEE-division instantiation of the walk)
    for i in at:
        behind = lines[i + 1:i + 12]
        assert any(re.match(r"v_sub_f32_e32 v\d+, s\d+, v\d+", l) for l in behind), behind      # planes read as scalar operands, no v_mov detour
        before = lines[max(0, i - 12):i]
        assert not any(l.startswith("global_load_dwordx4") for l in before), before                # the vector loads were not hoisted above the branch
    assert any(l.startswith("s_load_dwordx8") for l in lines)               # wave-uniform leaves: triangle records through the scalar cache
