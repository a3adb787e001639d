"""The kernels' image sampler (csrc/k_shade.h sample_by_lod, the function the shade stage, the sky stage and the denoiser's guides inline) through
rpt_debug_sample_image, bit for bit against the CPU oracle's (oracle_sample_image, the one trace_pixel calls), on the extents and coordinates of
tests/test_f64_reference.py::test_oracle_sampler_against_f64, which holds that oracle function to the float64 restatement.  The device function is
hand-optimised: a mask instead of the remainder where both extents are powers of two; for any other image a coordinate below the extent passes, one
equal to it wraps to 0 and only the rest divides; a row's two RGBA8 texels come from one 8-byte load, shifted left by one in the last column, with a
second load where the footprint wraps; an image one texel wide has a path of its own.  Every rendered atlas and skybox of the other tests is a power
of two in both extents; here each branch is reached on purpose, and the test counts from the restatement's integers that its input does reach it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_ref       # noqa: E402
import scenes        # noqa: E402

pytestmark = pytest.mark.gpu


def branch_counts(width, height, coords):
    """how many coordinates take each branch of the device sampler, from f64_ref.sample_by_lod's integers (raw: floor and ceil as i32, index: the
    texels after the remainder)"""
    _, index, raw = f64_ref.sample_by_lod(scenes.sampler_image(width, height, False), width, height, coords)
    extent = np.array([width, height])
    x0, x1 = index[:, 0, 0], index[:, 3, 0]
    return {"equals_extent": int((raw == extent).any((1, 2)).sum()),                       # image_wrap: u == extent -> 0
            "below_extent": int(((raw >= 0) & (raw < extent)).all((1, 2)).sum()),          # image_wrap: u < extent
            "saturated": int(((raw == f64_ref.I32_MAX) | (raw == f64_ref.I32_MIN)).any((1, 2)).sum()),
            "negative": int((raw < 0).any((1, 2)).sum()),                                  # sign-extended: the 64-bit remainder
            "beyond_extent": int((raw > extent).any((1, 2)).sum()),                        # the 64-bit remainder, from above
            "last_column_same_texel": int(((x0 == width - 1) & (x1 == x0)).sum()),         # u8_row_pair: the pair shifted left, no second load
            "last_column_wrapping": int(((x0 == width - 1) & (x1 != x0)).sum()),           # u8_row_pair: a footprint from the last column to column 0
            "inner_pair": int(((x0 < width - 1) & (x1 == x0 + 1)).sum())}                  # u8_row_pair: both texels from the one load


@pytest.mark.parametrize("is_u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("extent", scenes.SAMPLER_EXTENTS, ids=lambda e: f"{e[0]}x{e[1]}")
def test_device_sampler_equals_oracle(renderer, oracle, extent, is_u8):
    width, height = extent
    image, coords = scenes.sampler_image(width, height, is_u8), scenes.sampler_coords(width, height)
    assert len(coords) <= 100_000
    n = branch_counts(width, height, coords)
    print(f"sampler {width}x{height} {'u8' if is_u8 else 'f32'}: {len(coords)} coordinates, {n}")
    power_of_two = (width & (width - 1)) == 0 and (height & (height - 1)) == 0
    # every extent: coordinate 1.0 (the ceiling equals the extent), saturated casts (1e10, 3e38, the infinities), negative and large coordinates.  Where
    # the image is no power of two in both extents these are image_wrap's general branches, the last three its 64-bit remainder.
    for kind in ("equals_extent", "saturated", "negative", "beyond_extent"):
        assert n[kind] > 0, kind
    assert power_of_two == (extent in ((1, 1), (2, 2), (64, 64)))
    if width >= 2:
        for kind in ("below_extent", "last_column_same_texel", "last_column_wrapping", "inner_pair"):
            assert n[kind] > 0, kind
    else:
        assert n["inner_pair"] == 0 and n["last_column_same_texel"] == len(coords)         # width == 1: every footprint is column 0 twice
    got = renderer.debug_sample_image(image, coords)
    want = oracle.sample_image(image, coords)
    nan = np.isnan(want)
    assert nan.any() and not nan.all(1).all()                                               # an infinite scaled coordinate has no fractional part
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), "the device sampler differs bitwise from the oracle's"


def test_device_sampler_hook_refuses_bad_arguments(renderer, hipmod):
    import ctypes as C
    L = hipmod.lib()
    image, coords, out = np.zeros((2, 2, 4), np.uint8), np.zeros((1, 2), np.float32), np.zeros((1, 4), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.rpt_debug_sample_image(renderer._h, 1, p(image), 0, 2, 1, p(coords), p(out)) != 0
    assert L.rpt_debug_sample_image(renderer._h, 1, p(image), 2, 0, 1, p(coords), p(out)) != 0
    assert L.rpt_debug_sample_image(renderer._h, 1, None, 2, 2, 1, p(coords), p(out)) != 0
    assert L.rpt_debug_sample_image(renderer._h, 1, p(image), 1 << 16, 1 << 15, 1, p(coords), p(out)) != 0     # more texels than 32-bit indices allow
    assert L.rpt_debug_sample_image(renderer._h, 1, p(image), 2, 2, 0, p(coords), p(out)) == 0                 # nothing to do
