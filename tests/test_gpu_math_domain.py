"""csrc/rpt_math.h on the DEVICE over the whole float domain: gfx950 == the clang host build inside librpt_hip.so == the g++ build of the oracle, bit for
bit, on the sets of tests/math_domain.py — every sign and exponent field (denormals, infinities, NaNs), every float around every branch threshold, every
special-case row of powr and atan2r, the arguments where reduce_pio2's n is large or negative.  This is where the device code is another expression
than the host's: the inline-asm Horner step, v_min_f32 / v_max_f32 for fminr / fmaxr, the f32 seeds of rcp_newton and sqrt_newton (which need
-fhip-fp32-correctly-rounded-divide-sqrt), roundings into the f32 denormals (-fno-gpu-flush-denormals-to-zero), the expanded double -> int64
conversion, v_ldexp_f32.

These tests need no float64 reference of their own: tests/test_math_domain.py holds the host builds to float64 (and the helpers to their definitions)
on the SAME arrays, so "equal to the host" here is "equal to float64 rounded once" there.  One rpt_debug_math call per operation.

What a float cannot show: the rounding to float hides a difference of the last bits of the double evaluation on all but a 2^-29th of the arguments (a
device Horner step with two roundings instead of the fma passes every test above).  So the double building blocks themselves — sin_poly, cos_poly,
exp_core, log_core, asin_poly, atan01 — are read out word by word (hook ops 20 .. 31) and compared bit for bit as well."""
import numpy as np
import pytest

import math_domain as md
from math_domain import bits

pytestmark = pytest.mark.gpu

WORDS = ("f2u32_sat", "abs")                     # results that are bit patterns: no NaN rule
EITHER_ZERO = ("fmin", "fmax")                   # rpt_math.h: "the sign of a zero result is never observable on the hot path": v_min_f32 / v_max_f32


def equal(name, a, b):
    same = bits(a) == bits(b)
    if name not in WORDS:
        same |= np.isnan(a) & np.isnan(b)
    if name in EITHER_ZERO:
        same |= (a == 0) & (b == 0)
    return same


def report(name, x, y, i, dev, clang, gxx):
    arg = f"x = 0x{bits(x)[i]:08x} ({float(x[i])!r})" + ("" if y is None else f", y = 0x{bits(y)[i]:08x} ({float(y[i])!r})")
    return f"{name} at {arg}: device 0x{bits(dev)[i]:08x}, clang host 0x{bits(clang)[i]:08x}, g++ oracle 0x{bits(gxx)[i]:08x}"


@pytest.mark.parametrize("name", md.UNARY + md.PAIRS)
def test_device_equals_the_host_builds_on_the_whole_domain(renderer, hipmod, oracle, name):
    x, y = md.arguments(name)
    assert 0 < x.size <= md.MAX_SET
    op = md.OPS[name]
    dev = renderer.debug_math(op, x, y)
    clang, gxx = hipmod.debug_math_host(op, x, y), oracle.math(op, x, y)
    hosts = equal(name, clang, gxx)
    assert hosts.all(), "the host compilers disagree: " + report(name, x, y, np.flatnonzero(~hosts)[0], dev, clang, gxx)
    ok = equal(name, dev, clang)
    print(f"{name}: {x.size} arguments, {int((~ok).sum())} differ between the device and the host")
    assert ok.all(), f"{int((~ok).sum())} of {x.size} differ, first: " + report(name, x, y, np.flatnonzero(~ok)[0], dev, clang, gxx)
    if name == "slab_quotient":
        # the contract of tests/test_fastdiv.py against the IEEE quotient (op 8, the host's): equal bits, or both zero, or both NaN
        true = hipmod.debug_math_host(md.OPS["div"], x, y)
        ok = (bits(dev) == bits(true)) | ((dev == 0) & (true == 0)) | (np.isnan(dev) & np.isnan(true))
        assert ok.all(), "against x / y: " + report(name, x, y, np.flatnonzero(~ok)[0], dev, true, gxx)


@pytest.mark.parametrize("name", sorted(md.CORE_OPS))
def test_device_doubles_equal_the_host_builds_bit_for_bit(renderer, hipmod, oracle, name):
    x = md.core(name)
    assert 0 < x.size <= md.MAX_SET
    for word, op in (("low", md.CORE_OPS[name]), ("high", md.CORE_OPS[name] + 1)):
        dev, clang, gxx = renderer.debug_math(op, x), hipmod.debug_math_host(op, x), oracle.math(op, x)
        ok = (bits(dev) == bits(clang)) & (bits(clang) == bits(gxx))
        print(f"{name} {word} word: {x.size} arguments, {int((~ok).sum())} differ")
        assert ok.all(), f"{int((~ok).sum())} of {x.size} differ in the {word} word, first: " + report(name, x, None, np.flatnonzero(~ok)[0], dev, clang, gxx)
