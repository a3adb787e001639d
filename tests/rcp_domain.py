"""The argument set on which the device's rptm::rcp_rn (csrc/rpt_rcp.h) is held to numpy's float32(1) / x (tests/test_gpu_rcp_exact.py), in the manner of
tests/math_domain.py and built from its generators: every sign x every exponent field x random and special mantissas, and every bit pattern within
RADIUS of the thresholds of the guard.  The guard is a test of the RESULT (0 or NaN: take the division), so its thresholds are properties of the
argument: the least normal 2^-126 (below it v_rcp_f32 flushes the argument), 2^126 (above it the reciprocal is a denormal, which v_rcp_f32 flushes), and
0, the largest float and the infinities, whose estimates are inf, 0 and 0.  Not a test module."""
import functools

import numpy as np

import math_domain as md
from math_domain import F32, bits

WINDOW_LO, WINDOW_HI = 2.0 ** -126, 2.0 ** 126          # rcp_rn's step is taken for |x| in [WINDOW_LO, WINDOW_HI], the division outside
THRESHOLDS = (0.0, WINDOW_LO, WINDOW_HI, 1.0, 2.0 ** 127, md.FLT_MAX, np.inf)


@functools.lru_cache(maxsize=None)
def arguments():
    t = np.array(THRESHOLDS)
    x = md._unique(np.concatenate([md.base(20), md.window(t), md.window(-t), md.from_bits([md.QNAN, md.SNAN, 0xffc00000, 0xff800001])]))
    assert x.size <= md.MAX_SET
    x.setflags(write=False)
    return x


def branch_counts(x):
    """how many arguments take each side of rcp_rn's guard, and by which way: the conditions restated on numpy arrays"""
    x = np.asarray(x, F32)
    ax, nan, mant = np.abs(x), np.isnan(x), bits(x) & 0x7fffff
    inside = ~nan & (ax >= WINDOW_LO) & (ax <= WINDOW_HI)
    return md._count({"step": inside, "step_negative": inside & np.signbit(x), "step_at_2^-126": ax == F32(WINDOW_LO), "step_at_2^126": ax == F32(WINDOW_HI),
                      "step_just_below_2^126": ax == np.nextafter(F32(WINDOW_HI), F32(0)), "step_mantissa_all_ones": inside & (mant == 0x7fffff),
                      "step_power_of_two": inside & (mant == 0), "division_zero": ax == 0, "division_denormal": (ax > 0) & (ax < WINDOW_LO),
                      "division_largest_denormal": bits(ax) == 0x007fffff, "division_just_above_2^126": ax == np.nextafter(F32(WINDOW_HI), F32(np.inf)),
                      "division_denormal_reciprocal": ~nan & (ax > WINDOW_HI) & np.isfinite(x), "division_inf": np.isinf(x), "division_nan": nan,
                      "division_negative": ~inside & ~nan & np.signbit(x)})
