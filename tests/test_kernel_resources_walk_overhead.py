"""What the streamed LDS walks need to keep two 1 024-thread workgroups on a CU (8 waves per SIMD), read from the built library as tests/test_kernel_resources.py
does: registers, scratch and static LDS of the seven kernels, and the room the largest LDS image leaves.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
CSRC = os.path.join(ROOT, "rust-path-tracer_amd", "csrc")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

KERNELS = ["void k_traverse_nearest_stream<16, 1024, 0>", "void k_traverse_nearest_stream<16, 1024, 1>", "void k_traverse_nearest_stream<16, 1024, 2>",
           "void k_traverse_shadow_stream<16, 1024, false>", "void k_traverse_shadow_stream<16, 1024, true>",
           "void k_traverse_shadow_stream_seg<16, 1024, false>", "void k_traverse_shadow_stream_seg<16, 1024, true>"]
STATIC_LDS = 16 * 16 * 64 * 2 + 16          # sixteen waves' 16-entry columns of 16-bit entries, and the pool (a 64-bit word and the lock, padded): 32 784 bytes
CU_LDS = 160 * 1024                         # MI355X


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
    return table


def _define(name):
    text = open(os.path.join(CSRC, "k_common.h")).read()
    return int(re.search(r"#define\s+%s\s+(\w+?)u?\b" % name, text).group(1), 0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_registers_scratch_and_static_lds(resources, kernel):
    hits = [v for k, vs in resources.items() if k.startswith(kernel) for v in vs]
    assert hits, kernel
    for vgpr, sgpr, scratch, lds in hits:
        assert vgpr <= 64 and sgpr <= 80 and scratch == 0
        assert lds == STATIC_LDS                     # what it was before the stack was addressed by its LDS address: no entry added, none dropped


def test_the_largest_image_leaves_room_for_two_workgroups():
    """A workgroup holds the static LDS and the image (at most RPT_LDS_SCENE_BYTES: rpt_scene.hip upload_lds_image); the LAST launch adds the flipped copy's pair
    records only if the sum stays within half a CU's LDS (upload_last_copy measures that room on the device).  Here: the bound without the copy, and that
    a copy of the largest image's pair records can never be what pushes a workgroup over (the upload drops it instead)."""
    image = _define("RPT_LDS_SCENE_BYTES")
    assert image == 32768
    assert STATIC_LDS + image <= CU_LDS // 2
    room = CU_LDS // 2 - STATIC_LDS - image            # what a flipped copy may use
    # the record sizes the image is built from (build_lds_image): 6 plane vectors and a descriptor word per pair, 3 vectors per triangle — unchanged by the
    # interleaved triangle records and the scaled descriptors
    scene = open(os.path.join(CSRC, "rpt_scene.hip")).read()
    assert "image.assign(6 * P + desc_vecs + 3 * nt" in scene and "desc_vecs = (P + 3) / 4" in scene
    assert "flip_vecs = 6 * (size_t)s.lds_pairs + ((size_t)s.lds_pairs + 3) / 4" in scene and "((size_t)s.lds_vecs + flip_vecs) * sizeof(float4) <= lds_room" in scene
    # DarkCornell's own figures (184 triangles, 140-odd pairs: 23 KB) fit with their copy; the largest image's copy (up to 32 KB of pair records) does not, and is not made
    assert room == 16368


def test_descriptor_fields_hold_every_image_the_upload_accepts():
    """an inner descriptor is 4 x the pair index and must stay below LDS_DESC_DEAD: an image of at most RPT_LDS_SCENE_BYTES has fewer than 342 pairs
    (96 bytes of planes each), far below 4 096; leaves keep 6 bits of count and 9 of first triangle under LDS_DESC_LEAF"""
    dead, leaf, image = _define("LDS_DESC_DEAD"), _define("LDS_DESC_LEAF"), _define("RPT_LDS_SCENE_BYTES")
    assert 4 * (image // 96) < dead and dead < leaf == 0x8000
    assert (63 << 9 | 511) < leaf
