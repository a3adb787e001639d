"""rptm::rcp_rn and rcp_rn_window (csrc/rpt_rcp.h) ARE the IEEE reciprocal: checked on the device for every float, not argued.  rpt_debug_rcp_sweep
enumerates the bit patterns on the device and compares with the compiler's correctly rounded `1.0f / x` word for word (NaNs too: outside its guard
rcp_rn is that division); that division is itself held to the host in test_gpu_parity / test_gpu_math_domain, and rcp_rn to numpy here on the set of
tests/rcp_domain.py."""
import numpy as np
import pytest

import rcp_domain as rd
from math_domain import bits

pytestmark = pytest.mark.gpu

WINDOW_FIRST, WINDOW_LAST = 0x00800000, 0x7e800000          # the bit patterns of 2^-126 and 2^126


def test_rcp_rn_is_the_ieee_reciprocal_of_every_float(renderer):
    """all 2^32 bit patterns: zeros, denormals, both ends of the window, infinities and every NaN"""
    bad, where = renderer.debug_rcp_sweep(0, 1 << 32)
    print(f"rcp_rn: {bad} of 2^32 arguments differ")
    assert bad == 0, (bad, [hex(int(w)) for w in where])


@pytest.mark.parametrize("sign", [0, 0x80000000])
def test_rcp_rn_window_is_the_ieee_reciprocal_on_all_of_its_window(renderer, sign):
    """the step without the guard, for callers that have established |x| in [2^-126, 2^126]: every such float"""
    bad, where = renderer.debug_rcp_sweep(sign | WINDOW_FIRST, WINDOW_LAST - WINDOW_FIRST + 1, window=True)
    print(f"rcp_rn_window, sign bit {sign >> 31}: {bad} of {WINDOW_LAST - WINDOW_FIRST + 1} arguments differ")
    assert bad == 0, (bad, [hex(int(w)) for w in where])


def test_the_sweep_sees_a_difference_where_there_is_one(renderer):
    """Outside the window the step alone is wrong (v_rcp_f32 flushes a denormal argument: the estimate is inf, the step makes it NaN) — the checker is
    not blind, and it lists what it counts."""
    bad, where = renderer.debug_rcp_sweep(1, 0x007fffff, window=True)
    assert bad == 0x007fffff and len(where) == 64 and all(1 <= int(w) <= 0x007fffff for w in where)
    bad, where = renderer.debug_rcp_sweep(WINDOW_LAST + 1, 5, window=True)           # the first five floats above 2^126
    assert bad == 5 and sorted(int(w) for w in where) == list(range(WINDOW_LAST + 1, WINDOW_LAST + 6))


def test_every_side_of_the_guard_is_reached():
    n = rd.branch_counts(rd.arguments())
    print(n)
    assert all(v > 0 for v in n.values()), [k for k, v in n.items() if v == 0]


def test_device_rcp_rn_equals_numpy_on_the_whole_domain(renderer):
    x = rd.arguments()
    with np.errstate(all="ignore"):
        want = np.float32(1) / x
    got = renderer.debug_rcp(x)
    differ = np.flatnonzero(bits(got) != bits(want))
    print(f"rcp_rn: {x.size} arguments, {differ.size} differ between the device and numpy")
    assert differ.size == 0, [f"x = 0x{bits(x)[i]:08x}: device 0x{bits(got)[i]:08x}, numpy 0x{bits(want)[i]:08x}" for i in differ[:8]]
    inside = np.abs(x) >= np.float32(rd.WINDOW_LO)
    inside &= np.abs(x) <= np.float32(rd.WINDOW_HI)
    assert np.array_equal(bits(renderer.debug_rcp(x[inside], window=True)), bits(want[inside]))
