"""csrc/rpt_math.h on the HOST over the whole float domain (tests/math_domain.py: every sign and exponent field, every neighbourhood of a branch threshold,
every special-case row): the g++ build (the oracle) and the clang build (inside librpt_hip.so) agree bit for bit, and both are the float64 value of the
function rounded once to float32 — the numpy float64 function of the widened argument, an implementation that shares nothing with the header.

Double rounding: float64 carries the function's value to ~2^-52 relative; where that value lies within 2^-48 relative of the midpoint of two neighbouring
floats the rounding of the float64 number does not decide the rounding of the true value.  Such arguments are FLAGGED; they are settled with mpmath at 200
bits where it can be imported (else either neighbour is accepted), and may be at most 1e-4 of a set.  Everything else must be equal: the bits, the sign of a
zero, which arguments give NaN, an infinity, a denormal.

tests/test_gpu_math_domain.py holds the device to these host builds on the same arrays."""
from fractions import Fraction

import numpy as np
import pytest

import math_domain as md
from math_domain import F32, F64, U32, bits

try:
    import mpmath
except ImportError:                                   # flagged arguments then accept either neighbour
    mpmath = None

FLAG_REL = 2.0 ** -48
# sqrt and division in float64 are IEEE operations, correctly rounded: the true value lies within 2^-53 relative of the float64 number, so that number
# decides unless it is within 2^-52 of the midpoint.  (Under 2^-48 the mantissas 1 and 2^23 - 1 of every exponent field — sqrt(1 + 2^-23) = 1 + 2^-24 -
# 2^-49 ... — would be flagged, 2.3e-4 of the sqrt set, though float64 settles each of them.)  Fewer flagged arguments, nothing accepted that was not.
FLAG_REL_EXACT_OPS = {"sqrt": 2.0 ** -52, "div": 2.0 ** -52}
MAX_FLAGGED_SHARE = 1e-4
ROUNDED_ONCE = ("sin", "cos", "acos", "asin", "exp", "sqrt", "atan", "atan2", "pow", "div")
HELPERS = ("fmin", "fmax", "floor", "ceil", "f2u32_sat", "powi5", "abs")


def same(a, b):
    """bit for bit, the sign of a zero included; NaN counts as equal to NaN"""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def ulps(a, b):
    """distance in float32 steps where both are numbers (an infinity is one step beyond the largest float), 0 where both are NaN, -1 where one is"""
    d = np.abs(md.ordinal(a) - md.ordinal(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, np.where(np.isnan(a) | np.isnan(b), -1, d))


@pytest.fixture(scope="module")
def host(oracle, hipmod):
    """(x, y, clang host build, g++ oracle build) of every function, evaluated once"""
    cache = {}

    def get(name):
        if name not in cache:
            x, y = md.arguments(name)
            cache[name] = (x, y, hipmod.debug_math_host(md.OPS[name], x, y), oracle.math(md.OPS[name], x, y))
        return cache[name]
    return get


def float64_value(name, x, y):
    """the function in numpy float64 on the widened arguments — and, outside sincosr's supported domain, what the header says it returns there"""
    with np.errstate(all="ignore"):
        d = x.astype(F64)                                                               # (widening a signalling NaN raises "invalid")
        e = None if y is None else y.astype(F64)
        if name in ("sin", "cos"):
            beyond = np.isfinite(d) & (np.abs(d) >= 2.0 ** 30)                          # "|x| >= 2^30 ... yields (0, 1) deterministically"
            return np.where(beyond, 0.0 if name == "sin" else 1.0, (np.sin if name == "sin" else np.cos)(np.where(beyond, 0.0, d)))
        if name in ("exp", "exp_sky"):
            return np.exp(d)
        if name == "pow":
            return np.power(d, e)
        if name == "atan2":
            return np.arctan2(d, e)
        if name == "div":
            return d / e
        return {"acos": np.arccos, "asin": np.arcsin, "sqrt": np.sqrt, "atan": np.arctan}[name](d)


def round_once(v, flag_rel=FLAG_REL):
    """float64 -> (the nearest float32, its neighbour on the other side of v, the midpoint of the two, flagged: v too close to the midpoint to decide)"""
    with np.errstate(all="ignore"):
        r = v.astype(F32)
        # beyond the largest float the next "float" is 2^128: the rounding boundary is (FLT_MAX + 2^128) / 2
        wide = lambda f, s: np.where(np.isinf(f) & np.isfinite(v), np.copysign(2.0 ** 128, s), f.astype(F64))
        r64 = wide(r, v)
        other = np.nextafter(r, np.where(v > r64, np.inf, -np.inf).astype(F32))
        o64 = wide(other, v)
        mid = 0.5 * r64 + 0.5 * o64
        flagged = np.isfinite(v) & (v != r64) & (np.abs(v - mid) <= flag_rel * np.abs(v))
    return r, other, mid, flagged


def _exact(name, x, y):
    f = mpmath.mpf
    a = f(float(x))
    if name == "pow":
        return mpmath.power(a, f(float(y)))
    if name == "atan2":
        return mpmath.atan2(a, f(float(y)))
    if name == "div":
        return a / f(float(y))
    return getattr(mpmath, name)(a)


def settle(name, x, y, want, other, mid, flagged):
    """the correctly rounded float of every flagged argument from 200-bit arithmetic: the neighbour on the exact value's side of the midpoint, the even one on a tie"""
    want = want.copy()
    with mpmath.workprec(200):
        for i in np.flatnonzero(flagged):
            exact, m = _exact(name, x[i], None if y is None else y[i]), mpmath.mpf(float(mid[i]))
            lo, hi = sorted((want[i], other[i]), key=float)
            if exact == m:
                want[i] = lo if (bits(np.array([lo]))[0] & 1) == 0 else hi
            else:
                want[i] = hi if exact > m else lo
    return want


def describe(x, y, i):
    return "x = %r (0x%08x)" % (float(x[i]), bits(x)[i]) + ("" if y is None else ", y = %r (0x%08x)" % (float(y[i]), bits(y)[i]))


@pytest.mark.parametrize("name", ROUNDED_ONCE)
def test_host_builds_agree_and_are_the_float64_value_rounded_once(host, name):
    """sin and cos: held on the whole of |x| < 2^30, beyond the 1e5 the header used to promise — measured on this set, 0 differences."""
    x, y, clang, gxx = host(name)
    differ = ~same(clang, gxx)
    assert not differ.any(), "the host compilers disagree at " + describe(x, y, np.flatnonzero(differ)[0])
    want, other, mid, flagged = round_once(float64_value(name, x, y), FLAG_REL_EXACT_OPS.get(name, FLAG_REL))
    share = flagged.mean()
    if mpmath is not None:
        want = settle(name, x, y, want, other, mid, flagged)
        ok = same(clang, want)
    else:
        ok = same(clang, want) | (flagged & same(clang, other))
    worst = ulps(clang, want)
    print(f"{name}: {x.size} arguments, {int(flagged.sum())} flagged ({share:.2e}), {int((~ok).sum())} differences, worst {int(worst.max())} ulp"
          f"{'' if worst.min() >= 0 else ', NaN against a number'}")
    assert x.size <= md.MAX_SET
    assert share <= MAX_FLAGGED_SHARE
    if not ok.all():
        i = np.flatnonzero(~ok)[0]
        raise AssertionError(f"{name}: {int((~ok).sum())} differences from float64 rounded once, first at {describe(x, y, i)}: "
                             f"got 0x{bits(clang)[i]:08x}, want 0x{bits(want)[i]:08x}{' (flagged)' if flagged[i] else ''}")
    # the classes of the result, spelled out (all implied by the equality above)
    for cls in (np.isnan, np.isinf, lambda r: r == 0, lambda r: np.signbit(r) & ~np.isnan(r), lambda r: (np.abs(r) > 0) & (np.abs(r) < 2.0 ** -126)):
        assert np.array_equal(cls(clang) & ~flagged, cls(want) & ~flagged)


def test_sky_exp_is_within_one_ulp_on_the_whole_domain(host):
    """exp_sky (float arithmetic only, not correctly rounded by design): within 1 ulp of float32(exp in float64) for every argument of the set — denormal
    results and the step from the largest float to +inf included — with the special cases of the header: NaN -> NaN, +inf above 89, +0 below -104."""
    x, _, clang, gxx = host("exp_sky")
    differ = ~same(clang, gxx)
    assert not differ.any(), "the host compilers disagree at " + describe(x, None, np.flatnonzero(differ)[0])
    want, _, _, flagged = round_once(float64_value("exp_sky", x, None))
    d = ulps(clang, want)
    print(f"exp_sky: {x.size} arguments, {int(flagged.sum())} flagged, {int((d != 0).sum())} differ from the correctly rounded value, worst {int(d.max())} ulp")
    assert d.min() >= 0 and np.array_equal(np.isnan(clang), np.isnan(x))
    assert d.max() <= 1, describe(x, None, int(d.argmax()))
    assert np.all(bits(clang[x > 89.0]) == 0x7f800000) and np.all(bits(clang[x < -104.0]) == 0)
    assert not np.signbit(clang[~np.isnan(x)]).any()


def test_slab_quotient_is_the_ieee_quotient(host):
    """op 9 against op 8 under the contract of tests/test_fastdiv.py: equal bits, or both zero, or both NaN — on both sides of every guard of rpt_fastdiv.h"""
    x, y, fast, fast_gxx = host("slab_quotient")
    _, _, true, _ = host("div")
    differ = ~same(fast, fast_gxx)
    assert not differ.any(), "the host compilers disagree at " + describe(x, y, np.flatnonzero(differ)[0])
    ok = (bits(fast) == bits(true)) | ((fast == 0) & (true == 0)) | (np.isnan(fast) & np.isnan(true))
    sign_only = (fast == 0) & (true == 0) & (bits(fast) != bits(true))
    print(f"slab_quotient: {x.size} pairs, {int((~ok).sum())} differences, {int(sign_only.sum())} zero quotients of the other sign")
    assert ok.all(), describe(x, y, np.flatnonzero(~ok)[0])
    assert np.all((x[sign_only] == 0) & np.signbit(x[sign_only]))                        # the one documented difference: the dividend -0


def round_fraction(q):
    """an exact rational -> the nearest float32, ties to even, in integer arithmetic"""
    if q == 0:
        return F32(0.0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    e -= a < Fraction(2) ** e                                                            # 2^e <= a < 2^(e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(a, ulp)
    n = int(n) + (rem * 2 > ulp or (rem * 2 == ulp and int(n) % 2 == 1))
    v = n * ulp
    r = F32(np.inf) if v >= Fraction(2) ** 128 else F32(float(v))
    return -r if q < 0 else r


def test_integer_powers_are_rounded_once_exact_ties_included(host):
    """powr on integer powers that are EXACTLY the midpoint of two floats (the even neighbour is the answer), on the powers of two that give 2^-150 (the tie
    with zero) and on each such base's neighbours: held to exact rational arithmetic.  exp(y log x), good to 1e-16, cannot decide a tie: powi_exact does.
    Before it, the whole-domain pow set had one difference: (-1.6272068e18)^2 = 0x7bfef95c.8 exactly, answered 0x7bfef95d."""
    x, y, clang, gxx = host("pow_ties")
    differ = ~same(clang, gxx)
    assert not differ.any(), "the host compilers disagree at " + describe(x, y, np.flatnonzero(differ)[0])
    want = np.array([round_fraction(Fraction(float(a)) ** int(n)) for a, n in zip(x, y)], F32)
    ok = bits(clang) == bits(want)
    print(f"pow_ties: {x.size} pairs, {md.branch_counts('pow_ties', x, y)}, {int((~ok).sum())} differences, worst {int(ulps(clang, want).max())} ulp")
    assert ok.all(), describe(x, y, np.flatnonzero(~ok)[0]) + f": got 0x{bits(clang)[np.flatnonzero(~ok)[0]]:08x}, want 0x{bits(want)[np.flatnonzero(~ok)[0]]:08x}"


CORE_FLOAT64 = {"sin_poly": np.sin, "cos_poly": np.cos, "exp_core": np.exp, "log_core": np.log, "asin_poly": np.arcsin, "atan01": np.arctan}
# where a polynomial was fitted (rpt_math_consts.h): the hook evaluates it on [-1, 1], the value is held to float64 only where its callers use it
CORE_FITTED = {"sin_poly": np.pi / 4, "cos_poly": np.pi / 4, "asin_poly": 0.5}


@pytest.mark.parametrize("name", sorted(md.CORE_OPS))
def test_double_building_blocks_agree_between_the_host_compilers(oracle, hipmod, name):
    """hook ops 20 .. 31: the DOUBLE that sin_poly ... atan01 return, both words — g++ == clang bit for bit, and the value within 4 float64 steps of
    numpy's on the block's fitted domain (the header: "internal error ~1e-16 relative"; 2^-50 = 8.9e-16 is 4 steps, numpy's own error of a step or two
    included)."""
    x = md.core(name)
    words = {}
    for build, f in (("clang", hipmod.debug_math_host), ("g++", oracle.math)):
        lo, hi = bits(f(md.CORE_OPS[name], x)), bits(f(md.CORE_OPS[name] + 1, x))
        words[build] = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    differ = words["clang"] != words["g++"]
    assert not differ.any(), describe(x, None, np.flatnonzero(differ)[0])
    got = words["clang"].view(F64)
    with np.errstate(all="ignore"):
        want = CORE_FLOAT64[name](x.astype(F64))
        rel = np.where((want == got) | (np.abs(x) > CORE_FITTED.get(name, np.inf)), 0.0, np.abs(got - want) / np.abs(want))
    print(f"{name}: {x.size} arguments, worst relative difference from float64 {rel.max():.2e}")
    assert 0 < x.size <= md.MAX_SET and np.isfinite(got).all() and len(np.unique(words["clang"])) > x.size // 4
    assert rel.max() <= 2.0 ** -50, describe(x, None, int(rel.argmax()))


def definition(name, x, y):
    """ops 12 to 19 written out in numpy -> (float32 result, equal(got, want))"""
    plain = lambda want: (want, lambda got: same(got, want))
    with np.errstate(all="ignore"):
        if name in ("fmin", "fmax"):
            # Rust f32::min / max: a NaN yields the other operand (a signalling NaN is a NaN); a result of +-0 counts as one value
            # (written out: np.fmin answers NaN to a signalling one)
            want = np.where(np.isnan(x), y, np.where(np.isnan(y), x, (np.minimum if name == "fmin" else np.maximum)(x, y)))
            return want, lambda got: same(got, want) | ((got == 0) & (want == 0))
        if name in ("floor", "ceil"):
            return plain((np.floor if name == "floor" else np.ceil)(x))
        if name == "f2u32_sat":                                                          # Rust `as u32`: NaN and negatives 0, saturating, truncating
            d = x.astype(F64)
            word = np.where(np.isnan(d) | (d <= 0), 0, np.where(d >= 2.0 ** 32, 0xffffffff, np.trunc(np.clip(np.nan_to_num(d), 0, 2.0 ** 32 - 1)))).astype(np.uint64)
            want = md.from_bits(word.astype(U32))
            return want, lambda got: bits(got) == bits(want)                             # a word: bit patterns only
        if name == "powi5":
            x2 = x * x
            return plain(x * (x2 * x2))
        if name == "abs":
            want = md.from_bits(bits(x) & U32(0x7fffffff))
            return want, lambda got: bits(got) == bits(want)
    raise KeyError(name)


@pytest.mark.parametrize("name", HELPERS + ("atan",))
def test_helpers_are_their_definitions(host, name):
    x, y, clang, gxx = host(name)
    differ = ~same(clang, gxx)
    assert not differ.any(), "the host compilers disagree at " + describe(x, y, np.flatnonzero(differ)[0])
    if name == "atan":                                                                   # op 17 is held to float64 above; here: atanr IS atan2r(x, 1)
        return
    want, equal = definition(name, x, y)
    ok = equal(clang)
    print(f"{name}: {x.size} arguments, {int((~ok).sum())} differences")
    assert ok.all(), describe(x, y, np.flatnonzero(~ok)[0]) + f": got 0x{bits(clang)[np.flatnonzero(~ok)[0]]:08x}, want 0x{bits(want)[np.flatnonzero(~ok)[0]]:08x}"


def test_atanr_is_atan2r_against_one(hipmod):
    x = md.unary("atan")
    assert same(hipmod.debug_math_host(17, x), hipmod.debug_math_host(6, x, np.ones_like(x))).all()


def test_the_hook_knows_ops_0_to_31_and_no_other(hipmod):
    x = np.ones(4, F32)
    for op in range(32):
        assert hipmod.debug_math_host(op, x, x).shape == x.shape
    for op in (-1, 32, 1 << 20):
        with pytest.raises(hipmod.RptError):
            hipmod.debug_math_host(op, x, x)


@pytest.mark.parametrize("name", md.UNARY + md.PAIRS)
def test_every_branch_is_reached(name):
    x, y = md.arguments(name)
    n = md.branch_counts(name, x, y)
    print(f"{name}: {x.size} arguments, {n}")
    assert 0 < x.size <= md.MAX_SET
    empty = [k for k, v in n.items() if v <= 0]
    assert not empty, empty


def test_the_sets_are_what_they_say():
    """every (sign, exponent field) class with the special mantissas, the thresholds' whole windows, seeded"""
    for name in md.UNARY:
        u = bits(md.unary(name))
        for m in md.SPECIAL_MANTISSAS:
            assert np.isin((np.arange(512, dtype=U32) << 23) | U32(m), u).all(), (name, m)
        cls, n = np.unique(u >> 23, return_counts=True)
        assert cls.size == 512 and n.min() >= 2048
        assert np.isin(bits(md.window(md.THRESHOLDS[name]())), u).all(), name
    for name in md.PAIRS:
        if name == "pow_ties":
            continue
        x, y = md.pairs(name)
        seen = np.zeros((512, 512), bool)
        seen[bits(x) >> 23, bits(y) >> 23] = True
        assert seen.all(), name
        s = bits(md.specials())
        both = np.isin(bits(x), s) & np.isin(bits(y), s)
        have = set(zip(bits(x)[both].tolist(), bits(y)[both].tolist()))
        assert all((int(a), int(b)) in have for a in s for b in s), name
    assert np.array_equal(bits(md.unary.__wrapped__("exp")), bits(md.unary("exp")))
    for a, b in zip(md._pow_pairs(np.random.default_rng(md._PAIR_SEED["pow"])), md.pairs("pow")):
        assert np.array_equal(bits(a), bits(b))
