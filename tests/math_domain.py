"""The argument sets on which csrc/rpt_math.h (and the quotient of rpt_fastdiv.h) is held to float64 on the host (tests/test_math_domain.py) and
the device to the host (tests/test_gpu_math_domain.py).  Not a test module: seeded generators, so that both files see the SAME arrays.

unary(name) -> x, pairs(name) -> (x, y): float32 arrays in the operand order of rpt_debug_math (for atan2 the first array is atan2's y).  Every set is

  * every sign x every one of the 256 exponent fields (denormals, infinities and NaNs among them) x random mantissas plus the mantissas 0, 1, 2, 2^22,
    2^23 - 2 and 2^23 - 1, resp. every (sign, exponent) class against every other, and
  * every bit pattern within +-RADIUS of each threshold the function's code branches on, resp. operand pairs built to land on either side of a threshold
    that is a property of the pair (|y| = |x|, lo / hi = tan(pi/8), y ln x = 89, a result next to 2^128 ...),

at most MAX_SET arguments.  The thresholds are those of rpt_math.h, rpt_math_consts.h and rpt_fastdiv.h; branch_counts(name, x[, y]) restates the branch
CONDITIONS in numpy (nothing else of the header) and the tests assert that every branch is reached."""
import functools

import numpy as np

F32, F64, U32, I64 = np.float32, np.float64, np.uint32, np.int64
MAX_SET = 1 << 21
RADIUS = 2048

OPS = {"sin": 0, "cos": 1, "acos": 2, "exp": 3, "pow": 4, "asin": 5, "atan2": 6, "sqrt": 7, "pow_ties": 4, "div": 8, "slab_quotient": 9, "exp_sky": 10,
       "fmin": 12, "fmax": 13, "floor": 14, "ceil": 15, "f2u32_sat": 16, "atan": 17, "powi5": 18, "abs": 19}
UNARY = ("sin", "cos", "acos", "asin", "exp", "exp_sky", "sqrt", "atan", "floor", "ceil", "f2u32_sat", "powi5", "abs")
PAIRS = ("pow", "pow_ties", "atan2", "div", "slab_quotient", "fmin", "fmax")

# rpt_math_consts.h
TAN_PIO8 = float.fromhex("0x1.a827999fcef32p-2")
TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
LOG2E = float.fromhex("0x1.71547652b82fep+0")
SQRT2 = 1.4142135623730951                     # log_core's cut
FLT_MAX = float(np.finfo(F32).max)
QNAN, SNAN = 0x7fc00000, 0x7f800001            # bit patterns

SPECIAL_MANTISSAS = (0, 1, 2, 1 << 22, (1 << 23) - 2, (1 << 23) - 1)
# 16777217 is no float: the float after 2^24 (16777218) stands for "the first integer beyond the odd / even test of powr"
_SPECIAL_MAGNITUDES = (0.0, 1.0, 2.0, 3.0, 0.5, 2.5, np.inf, 2.0 ** -149, FLT_MAX, 16777215.0, 16777216.0, 16777218.0)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def from_bits(u):
    return np.ascontiguousarray(u, U32).view(F32)


def ordinal(x):
    """float32 -> int64 on a line where neighbouring floats differ by one (+-0 both 0, NaNs beyond the infinities)"""
    u = bits(x).astype(I64)
    return np.where(u >> 31 != 0, -(u & 0x7fffffff), u)


def from_ordinal(o):
    o = np.clip(np.asarray(o, I64), -0x7fffffff, 0x7fffffff)
    return from_bits(np.where(o >= 0, o, 0x80000000 | -o).astype(U32))


def window(centres, radius=RADIUS):
    """every float within `radius` bit patterns of each centre (a window that holds +0 holds -0 too)"""
    c = ordinal(np.atleast_1d(np.asarray(centres, F64)).astype(F32))
    w = from_ordinal((c[:, None] + np.arange(-radius, radius + 1, dtype=I64)[None, :]).ravel())
    return np.concatenate([w, -w[w == 0]])


def _frozen(*arrays):
    for a in arrays:
        assert a.dtype == F32 and a.size <= MAX_SET, a.size
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def _unique(x):
    return from_bits(np.unique(bits(x)))


def base(seed, n_random=2048):
    """2 signs x 256 exponent fields x (n_random random mantissas + SPECIAL_MANTISSAS), sign-major"""
    rng = np.random.default_rng(seed)
    m = np.concatenate([rng.integers(0, 1 << 23, (2, 256, n_random), dtype=U32),
                        np.broadcast_to(np.array(SPECIAL_MANTISSAS, U32), (2, 256, len(SPECIAL_MANTISSAS)))], axis=2)
    s = (np.arange(2, dtype=U32) << 31)[:, None, None]
    e = (np.arange(256, dtype=U32) << 23)[None, :, None]
    return from_bits((s | e | m).ravel())


def _trig_thresholds():
    ks = np.array(sorted(set(range(1, 65)) | {1 << j for j in range(30)}), F64)
    t = np.concatenate([ks * (np.pi / 2),                                   # a reduced argument near 0: the cancellation of reduce_pio2
                        [np.pi / 4], (2 * ks + 1) * (np.pi / 4),            # ties of rint_magic: the quadrant switches
                        [0.0, 2.0 ** 30, 1e5]])                             # sincosr's branches, the header's promise
    return t[t <= 2.0 ** 30]


def _exp_thresholds():
    ln = np.log
    t = [89.0, -104.0, 0.0, ln(2.0 ** 128), ln(2.0 ** -126), ln(2.0 ** -149), ln(2.0 ** -150), 2.0 ** -25, 2.0 ** -24, 1.0]
    return np.array(t + [-v for v in t])


THRESHOLDS = {
    "sin": _trig_thresholds, "cos": _trig_thresholds, "exp": _exp_thresholds, "exp_sky": _exp_thresholds,
    "acos": lambda: np.array([0.0, 0.5, 1.0]), "asin": lambda: np.array([0.0, 0.5, 1.0]),
    "sqrt": lambda: np.array([0.0, 2.0 ** -126, 1.0, 2.0, 4.0, FLT_MAX]),                 # the denormals: the windows at 0 and below the least normal
    "atan": lambda: np.array([0.0, TAN_PIO8, 1.0, 1.0 / TAN_PIO8, FLT_MAX]),               # atanr(x) = atan2r(x, 1)
    "floor": lambda: np.array([0.0, 0.5, 1.0, 2.0 ** 23, 2.0 ** 24, FLT_MAX]), "ceil": lambda: np.array([0.0, 0.5, 1.0, 2.0 ** 23, 2.0 ** 24, FLT_MAX]),
    "f2u32_sat": lambda: np.array([0.0, 1.0, 2.0 ** 23, 2.0 ** 24, 2.0 ** 31, 2.0 ** 32, FLT_MAX]),
    "powi5": lambda: np.array([0.0, 1.0, 2.0 ** (128 / 5), 2.0 ** (-126 / 5), 2.0 ** (-149 / 5), 2.0 ** (-150 / 5), 2.0 ** 32, 2.0 ** 64, 2.0 ** -75]),
    "abs": lambda: np.array([0.0, FLT_MAX]),
}


@functools.lru_cache(maxsize=None)
def unary(name):
    """the whole-domain set of one unary function; sin and cos have ~180 thresholds, so their mirror images on the negative axis get a quarter of the radius"""
    t = THRESHOLDS[name]()
    many = len(t) > 32
    x = np.concatenate([base(OPS[name]), window(t), window(-t, RADIUS // 4 if many else RADIUS)])
    return _frozen(_unique(x))


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------------------

def specials():
    mags = np.array(_SPECIAL_MAGNITUDES, F64).astype(F32)
    return np.concatenate([mags, -mags, np.array([2.2], F32), from_bits([QNAN, SNAN])])


def _class_pairs(rng):
    """every (sign, exponent field) class against every other, 2 random mantissa pairs each: 512 x 512 x 2"""
    cls = np.arange(512, dtype=U32)
    hi = ((cls >> 8) << 31) | ((cls & 255) << 23)
    a = hi[:, None, None] | rng.integers(0, 1 << 23, (512, 512, 2), dtype=U32)
    b = hi[None, :, None] | rng.integers(0, 1 << 23, (512, 512, 2), dtype=U32)
    return from_bits(a.ravel()), from_bits(b.ravel())


def _grid(a, b):
    g = np.meshgrid(np.asarray(a, F32), np.asarray(b, F32), indexing="ij")
    return g[0].ravel().copy(), g[1].ravel().copy()


def _random_floats(rng, n, e_lo, e_hi, signed=True):
    """random mantissas, exponent FIELDS e_lo..e_hi inclusive"""
    u = (rng.integers(e_lo, e_hi + 1, n, dtype=U32) << 23) | rng.integers(0, 1 << 23, n, dtype=U32)
    if signed:
        u |= rng.integers(0, 2, n, dtype=U32) << 31
    return from_bits(u)


def _join(parts):
    x = np.ascontiguousarray(np.concatenate([np.asarray(p[0], F32) for p in parts]))
    y = np.ascontiguousarray(np.concatenate([np.asarray(p[1], F32) for p in parts]))
    assert x.shape == y.shape
    return _frozen(x, y)


def _common(rng):
    s = specials()
    return [_class_pairs(rng), _grid(s, s)]


POW_NEGATIVE_BASE_EXPONENTS = (1.0, -1.0, 3.0, -3.0, 5.0, 7.0, 16777215.0, -16777215.0, 8388607.0,                       # odd
                               2.0, -2.0, 4.0, -4.0, 16777214.0, 8388606.0,                                               # even, below 2^24
                               16777216.0, -16777216.0, 16777218.0, 2.0 ** 25, 2.0 ** 63, -(2.0 ** 64), FLT_MAX,          # >= 2^24: even, never odd
                               0.5, -0.5, 2.5, 8388607.5, -4194303.75, 2.0 ** -149, 2.2)                                  # no integer
POW_WINDOW_EXPONENTS = (2.2, 1.0 / 2.2, 0.5, 3.0, -1.5, 1e-3, 100.0, 1e7, -1e7)


def _pow_exact_ties(rng):
    """a set of its own (every argument of it would be flagged by the float64 reference: it is held to exact integer arithmetic instead): integer powers that are exactly the midpoint of two floats (powi_exact): m^n with 25 significant bits for every odd m that has one, at a few scales
    (among them the scale that puts a SHORTER odd m^n at an odd multiple of 2^-150, a tie of the denormals), and the powers of two that give 2^-150 —
    the tie with zero — and its neighbours, under positive and negative exponents; then each base's neighbours, which are no ties"""
    xs, ys = [], []
    for n in range(2, 16):
        for m in range(3, 5793, 2):
            v = m ** n
            if v >= 1 << 25:
                break
            for e in ((0, -40, 30, 127 // n - 24) if v >= 1 << 24 else ()) + ((-150 // n,) if -150 % n == 0 else ()):
                if 2.0 ** -149 <= m * 2.0 ** e <= FLT_MAX and (v >= 1 << 24 or e * n == -150):
                    xs += [m * 2.0 ** e, -m * 2.0 ** e]
                    ys += [float(n), float(n)]
    for t in (-150, -149, -151, -148, -126, -127, 127, 128, 150):
        for n in range(-255, 256):
            if abs(n) >= 2 and t % n == 0 and -149 <= t // n <= 127:
                xs += [2.0 ** (t // n), -(2.0 ** (t // n))]
                ys += [float(n), float(n)]
    x, y = np.array(xs, F64).astype(F32), np.array(ys, F32)
    assert np.array_equal(x.astype(F64), np.array(xs))
    return _join([(x, y), (from_ordinal(ordinal(x) + 1), y), (from_ordinal(ordinal(x) - 1), y)])


def _pow_pairs(rng):
    parts = _common(rng)
    mag = base(OPS["pow"])[: 256 * (2048 + len(SPECIAL_MANTISSAS))]                   # the sign-0 half: the sky's pow(|x|, 2.2) and its inverse
    assert not np.signbit(mag).any()
    for y in (2.2, 1.0 / 2.2):
        parts.append((mag, np.full(mag.size, y, F32)))
    # log_core's cut m > sqrt 2 acts on the mantissa alone: the full window at a handful of exponents, a narrow one at every other (denormals included)
    wide = (-140, -127, -126, -64, -2, -1, 0, 1, 2, 64, 126, 127)
    near = np.concatenate([window([1.0]), window([SQRT2 * 2.0 ** k for k in wide]),
                           window([SQRT2 * 2.0 ** k for k in range(-149, 128) if k not in wide], 32)])
    parts.append((near, np.resize(np.array(POW_WINDOW_EXPONENTS, F32), near.size)))
    # results on either side of 2^128 (overflow), 2^-126 (the first denormal), 2^-149 and 2^-150 (the last non-zero result) and of powr's own cuts
    # t > 89, t < -104: y = target / ln x from float64, and the 4 floats on either side of it
    x = _random_floats(rng, 2048, 1, 254, signed=False)
    x = x[x != 1.0]
    with np.errstate(over="ignore"):
        for target in (np.log(2.0 ** 128), np.log(2.0 ** -126), np.log(2.0 ** -149), np.log(2.0 ** -150), 89.0, -104.0):
            y0 = ordinal((target / np.log(x.astype(F64))).astype(F32))
            for d in range(-4, 5):
                parts.append((x, from_ordinal(y0 + d)))
    xn = -np.abs(_random_floats(rng, 8192, 0, 254))
    parts.append(_grid(xn, np.array(POW_NEGATIVE_BASE_EXPONENTS, F32)))
    return _join(parts)


def _signs(v, k):
    """v with the sign of bit k of the running index: the four sign combinations of a pair cycle through a set"""
    return np.where((np.arange(v.size) >> k) & 1, -v, v).astype(F32)


def _atan2_pairs(rng):
    parts = _common(rng)
    # |y| = |x| exactly and one pattern apart (dx > dy decides which operand is divided), every sign combination, both orders
    v = np.abs(_random_floats(rng, 8192, 0, 254))
    for d in (0, 1, -1):
        w = np.abs(from_ordinal(ordinal(v) + d))
        for sa in (1, -1):
            for sb in (1, -1):
                parts.append((sa * v, sb * w))
                if d:
                    parts.append((sa * w, sb * v))
    # lo / hi on either side of atan01's cut RPT_TAN_PIO8: under a power of two the window of lo is the window of the ratio
    for k in (-140, -126, -64, -1, 0, 1, 64, 127):
        lo = np.abs(window([TAN_PIO8 * 2.0 ** k]))
        hi = np.full(lo.size, 2.0 ** k, F32)
        parts.append((_signs(lo, 0), _signs(hi, 1)))
        parts.append((_signs(hi, 0), _signs(lo, 1)))
    hi = np.abs(_random_floats(rng, 8192, 1, 254))
    lo0 = ordinal((hi.astype(F64) * TAN_PIO8).astype(F32))
    for d in range(-2, 3):
        lo = from_ordinal(lo0 + d)
        parts.append((_signs(lo, 0), _signs(hi, 1)))
        parts.append((_signs(hi, 0), _signs(lo, 1)))
    # a denormal against the largest floats, in both orders (the scale of atan2r is 2^-127 there, lo * scale far below the floats)
    tiny = np.concatenate([from_bits([1, 2, 0x7fffff, 0x800000]), _random_floats(rng, 1020, 0, 0, signed=False)])
    huge = np.concatenate([from_bits([0x7f7fffff, 0x7f7ffffe, 0x7f000000, 0x7e800000]), _random_floats(rng, 1020, 253, 254, signed=False)])
    parts.append((_signs(tiny, 0), _signs(huge, 1)))
    parts.append((_signs(huge, 0), _signs(tiny, 1)))
    # the axes: +-0 against everything, in both orders
    every = base(OPS["atan2"], 26)
    for z in (0.0, -0.0):
        parts.append((np.full(every.size, z, F32), every))
        parts.append((every, np.full(every.size, z, F32)))
    return _join(parts)


def _div_pairs(rng):
    """IEEE division and slab_quotient(x, 0, y) share one set: the guards of rpt_fastdiv.h are |y| in [2^-40, 4) and x = 0 or |x| in [2^-60, 2^40)"""
    parts = _common(rng)
    def ok_x(n): return _random_floats(rng, n, 127 - 60, 127 + 39)
    def ok_y(n): return _random_floats(rng, n, 127 - 40, 127 + 1)
    parts.append((ok_x(1 << 18), ok_y(1 << 18)))                                        # the fast path itself
    y_edges, x_edges = [2.0 ** -40, 4.0, -(2.0 ** -40), -4.0], [2.0 ** -60, 2.0 ** 40, -(2.0 ** -60), -(2.0 ** 40), 0.0]
    wy, wx = window(y_edges), window(x_edges)
    parts.append((ok_x(wy.size), wy))                                                   # divisors on both sides of each guard
    parts.append((wx, ok_y(wx.size)))                                                   # operands on both sides of each guard and of 0
    parts.append(_grid(window(x_edges, 8), window(y_edges, 8)))
    z = np.resize(np.array([0.0, -0.0], F32), 4096)
    parts.append((z, ok_y(4096)))
    return _join(parts)


def _minmax_pairs(rng):
    parts = _common(rng)
    v = base(OPS["fmin"], 58)
    parts.append((v, v.copy()))                                                         # equal operands, NaN against itself
    parts.append((v, -v))
    near = from_ordinal(ordinal(v) + 1)
    parts.append((v, near))
    parts.append((near, v))
    return _join(parts)


_PAIR_MAKERS = {"pow": _pow_pairs, "pow_ties": _pow_exact_ties, "atan2": _atan2_pairs, "div": _div_pairs, "slab_quotient": _div_pairs, "fmin": _minmax_pairs, "fmax": _minmax_pairs}
_PAIR_SEED = {"pow": 104, "pow_ties": 105, "atan2": 106, "div": 108, "slab_quotient": 108, "fmin": 112, "fmax": 112}


@functools.lru_cache(maxsize=None)
def _pairs_of(maker, seed):
    return maker(np.random.default_rng(seed))


def pairs(name):
    return _pairs_of(_PAIR_MAKERS[name], _PAIR_SEED[name])


# ---- the double building blocks (hook ops 20 .. 31: the low word at CORE_OPS[name], the high word one above) -----------------------------------------

CORE_OPS = {"sin_poly": 20, "cos_poly": 22, "exp_core": 24, "log_core": 26, "asin_poly": 28, "atan01": 30}


@functools.lru_cache(maxsize=None)
def core(name):
    """the arguments of one building block: the part of a whole-domain set that lies in its domain, and 2^18 uniform draws where the callers' arguments lie"""
    rng = np.random.default_rng(CORE_OPS[name])
    draw = lambda lo, hi: rng.uniform(lo, hi, 1 << 18).astype(F32)
    if name in ("sin_poly", "cos_poly"):
        x = np.concatenate([unary("sin"), draw(-np.pi / 4, np.pi / 4)])
        x = x[np.abs(x) <= 1]
    elif name == "exp_core":
        x = np.concatenate([unary("exp"), draw(-104, 89), draw(-700, 700)])
        x = x[np.abs(x) <= 700]
    elif name == "log_core":
        x = np.concatenate([unary("sqrt"), pairs("pow")[0][-(1 << 18):], window([SQRT2 * 2.0 ** k for k in (-140, -126, -1, 0, 1, 127)]), draw(0, 4)])
        x = x[(x > 0) & np.isfinite(x)]
    elif name == "asin_poly":
        x = np.concatenate([unary("asin"), draw(-0.5, 0.5), draw(0, 0.7072)])        # |x| <= 1/2 directly, sqrt((1 - |x|) / 2) <= 0.7071 from the upper branch
        x = x[np.abs(x) <= 1]
    else:
        x = np.concatenate([unary("atan"), window([TAN_PIO8]), draw(0, 1)])
        x = x[(x >= 0) & (x <= 1)]
    return _frozen(_unique(x))


def arguments(name):
    """(x, y or None) of any function"""
    return (unary(name), None) if name in UNARY else pairs(name)


# ---- which branch an argument takes -----------------------------------------------------------------------------------------------------------------

def _count(d):
    return {k: int(np.count_nonzero(v)) for k, v in d.items()}


def _is_int(y):
    with np.errstate(invalid="ignore"):
        return np.isfinite(y) & (np.floor(y) == y)


def _is_odd(y):
    """powr: an integer below 2^24 in magnitude with its last bit set"""
    small = _is_int(y) & (np.abs(y) < 16777216.0)
    return small & ((np.where(small, y, 0).astype(I64) & 1) == 1)


def branch_counts(name, x, y=None):
    """how many arguments of a set take each branch of `name` in rpt_math.h / rpt_fastdiv.h: the conditions restated on numpy arrays"""
    x = np.asarray(x, F32)
    ax, nan, neg = np.abs(x), np.isnan(x), np.signbit(x)
    with np.errstate(all="ignore"):
        d = x.astype(F64)                                                               # (widening a signalling NaN raises "invalid")
        if name in ("sin", "cos"):
            inside = np.isfinite(x) & (ax < 2.0 ** 30) & (x != 0)
            n = np.rint(np.where(inside, d, 0.0) * TWO_OVER_PI)
            q = n.astype(I64) & 3
            c = {"not_finite": ~np.isfinite(x), "beyond_2^30": np.isfinite(x) & (ax >= 2.0 ** 30), "zero": x == 0, "n_zero": inside & (n == 0),
                 "n_negative": inside & (n < 0), "n_beyond_int16": inside & (np.abs(n) > 32768), "n_beyond_2^24": inside & (np.abs(n) > 2.0 ** 24),
                 "beyond_1e5": inside & (ax >= 1e5), "denormal": inside & (ax < 2.0 ** -126)}
            for k in range(4):
                c[f"quadrant_{k}"] = inside & (q == k)
                c[f"quadrant_{k}_n_negative"] = inside & (q == k) & (n < 0)
            return _count(c)
        if name in ("exp", "exp_sky"):
            core = ~nan & ~(x > 89.0) & ~(x < -104.0)
            k = np.rint(np.where(core, d, 0.0) * LOG2E)
            return _count({"nan": nan, "above_89": x > 89.0, "below_-104": x < -104.0, "plus_inf": x == np.inf, "minus_inf": x == -np.inf,
                           "core_overflows": core & (d > np.log(2.0 ** 128)), "core_normal": core & (k > -126) & (k < 127),
                           "core_denormal": core & (d < np.log(2.0 ** -126)) & (d > np.log(2.0 ** -149)), "core_rounds_to_zero": core & (d < np.log(2.0 ** -150)),
                           "result_one": core & (ax <= 2.0 ** -25), "k_negative_odd": core & (k < 0) & (k.astype(I64) & 1 == 1), "k_positive": core & (k > 0)})
        if name in ("acos", "asin"):
            upper = ~nan & (ax <= 1.0) & (ax > 0.5)
            c = {"nan": nan, "beyond_1": ax > 1.0, "lower": ax <= 0.5, "lower_negative": (ax <= 0.5) & neg, "upper_positive": upper & (x > 0),
                 "upper_negative": upper & (x < 0), "one": ax == 1.0, "next_to_one": ax == np.nextafter(F32(1), F32(0)), "half": ax == 0.5, "denormal": (ax > 0) & (ax < 2.0 ** -126)}
            if name == "asin":
                c.update({"plus_zero": (x == 0) & ~neg, "minus_zero": (x == 0) & neg})
            return _count(c)
        if name == "sqrt":
            return _count({"nan": nan, "negative": x < 0, "plus_zero": (x == 0) & ~neg, "minus_zero": (x == 0) & neg, "denormal": (x > 0) & (x < 2.0 ** -126),
                           "normal_exponent_field_odd": (x >= 2.0 ** -126) & np.isfinite(x) & (((bits(x) >> 23) & 1) == 1),
                           "normal_exponent_field_even": (x >= 2.0 ** -126) & np.isfinite(x) & (((bits(x) >> 23) & 1) == 0), "plus_inf": x == np.inf})
        if name in ("atan", "atan2"):
            yf, xf = (x, np.ones_like(x)) if name == "atan" else (x, np.asarray(y, F32))
            ok = ~np.isnan(yf) & ~np.isnan(xf)
            ay, axx, xneg, yneg = np.abs(yf), np.abs(xf), np.signbit(xf), np.signbit(yf)
            y0 = ok & (ay == 0)
            x0 = ok & ~y0 & (axx == 0)
            inf = ok & ~y0 & ~x0 & (np.isinf(axx) | np.isinf(ay))
            fin = ok & ~y0 & ~x0 & ~inf
            dy, dx = ay.astype(F64), axx.astype(F64)
            a = np.where(fin, np.minimum(dx, dy) / np.where(fin, np.maximum(dx, dy), 1.0), 0.0)
            c = {"nan": ~ok, "y_zero_x_positive": y0 & ~xneg, "y_inf": inf & np.isinf(ay) & ~np.isinf(axx),
                 "finite_below_cut": fin & (a <= TAN_PIO8), "finite_above_cut": fin & (a > TAN_PIO8), "finite_y_larger": fin & (dy > dx),
                 "finite_x_larger_or_equal": fin & ~(dy > dx), "y_negative": ok & yneg, "y_negative_zero": y0 & yneg, "denormal_operand": fin & (np.minimum(dx, dy) < 2.0 ** -126)}
            if name == "atan2":
                c.update({"y_zero_x_negative": y0 & xneg, "x_zero": x0, "both_inf_x_positive": inf & np.isinf(ay) & np.isinf(axx) & ~xneg, "both_inf_x_negative": inf & np.isinf(ay) & np.isinf(axx) & xneg,
                          "x_inf_positive": inf & ~np.isinf(ay) & ~xneg, "x_inf_negative": inf & ~np.isinf(ay) & xneg, "finite_x_negative": fin & xneg,
                          "finite_equal": fin & (dx == dy), "x_zero_negative": x0 & xneg,
                          "denormal_over_largest": fin & (np.minimum(dx, dy) < 2.0 ** -126) & (np.maximum(dx, dy) >= 2.0 ** 127)})
            return _count(c)
        if name in ("pow", "pow_ties"):
            y = np.asarray(y, F32)
            r1 = y == 0
            r2 = ~r1 & (x == 1)
            r3 = ~r1 & ~r2 & (nan | np.isnan(y))
            rest = ~r1 & ~r2 & ~r3
            odd, integer = _is_odd(y), _is_int(y)
            yinf = rest & np.isinf(y)
            x0 = rest & ~yinf & (x == 0)
            xinf = rest & ~yinf & ~x0 & np.isinf(x)
            fin = rest & ~yinf & ~x0 & ~xinf
            dom = fin & ~((x < 0) & ~integer)
            t = np.where(dom, y.astype(F64) * np.log(np.where(dom, ax, 1).astype(F64)), 0.0)
            m = np.frexp(np.where(dom, ax, 1).astype(F64))[0] * 2.0                      # [1, 2)
            small_int = dom & integer & (np.abs(y) >= 2) & (np.abs(y) <= 255)
            v = np.where(small_int, d, 1.0) ** np.where(small_int & (y > 0), y, 1.0).astype(F64)   # float64: exact where it matters here
            tie = small_int & (y > 0) & (np.abs(v) < 2.0 ** 128) & (np.abs(v) >= 2.0 ** -126) & (np.frexp(v)[0] * 2.0 ** 25 % 2 == 1)
            if name == "pow_ties":
                return _count({"exact_tie": tie, "tie_of_the_denormals": small_int & (y > 0) & (np.abs(v) < 2.0 ** -126) & (np.abs(v) * 2.0 ** 150 % 2 == 1),
                               "no_tie": small_int & (y > 0) & ~tie, "gives_2^-150": small_int & (m == 1.0) & (y.astype(F64) * np.log2(np.where(dom, ax, 1).astype(F64)) == -150),
                               "gives_2^-150_negative_exponent": small_int & (m == 1.0) & (y < 0) & (y.astype(F64) * np.log2(np.where(dom, ax, 1).astype(F64)) == -150),
                               "negative_exponent_other_base": small_int & (y < 0) & (m != 1.0), "negative_base_odd_exponent": small_int & (x < 0) & odd,
                               "overflows": small_int & (t > np.log(2.0 ** 128))})
            return _count({"y_zero": r1, "x_one": r2, "nan_operand": r3, "y_inf_x_minus_one": yinf & (ax == 1), "y_inf_gives_inf": yinf & ((ax > 1) == (y > 0)) & (ax != 1),
                           "y_inf_gives_zero": yinf & ((ax > 1) != (y > 0)) & (ax != 1), "x_zero_y_positive": x0 & (y > 0), "x_zero_y_negative": x0 & (y < 0),
                           "x_minus_zero_y_odd": x0 & neg & odd, "x_minus_zero_y_even": x0 & neg & integer & ~odd, "x_inf_y_positive": xinf & (y > 0),
                           "x_inf_y_negative": xinf & (y < 0), "x_minus_inf_y_odd": xinf & neg & odd, "x_minus_inf_y_not_odd": xinf & neg & ~odd,
                           "x_negative_y_no_integer": fin & (x < 0) & ~integer, "x_negative_y_odd": fin & (x < 0) & odd, "x_negative_y_even": fin & (x < 0) & integer & ~odd,
                           "x_negative_y_integer_from_2^24": fin & (x < 0) & integer & (np.abs(y) >= 16777216.0), "t_above_89": dom & (t > 89.0), "t_below_-104": dom & (t < -104.0),
                           "core": dom & (t <= 89.0) & (t >= -104.0), "core_overflows": dom & (t <= 89.0) & (t > np.log(2.0 ** 128)),
                           "core_denormal": dom & (t < np.log(2.0 ** -126)) & (t > np.log(2.0 ** -149)), "core_rounds_to_zero": dom & (t >= -104.0) & (t < np.log(2.0 ** -150)),
                           "integer_exponent_2_to_255": small_int, "integer_exponent_beyond_255": dom & integer & (np.abs(y) > 255),
                           "negative_integer_exponent_power_of_two": small_int & (y < 0) & (m == 1.0), "negative_integer_exponent_other_base": small_int & (y < 0) & (m != 1.0),
                           "integer_power_exact_tie": tie,
                           "mantissa_above_sqrt2": dom & (m > SQRT2), "mantissa_below_sqrt2": dom & (m <= SQRT2), "x_denormal": dom & (ax < 2.0 ** -126),
                           "sky_exponent": dom & (y == F32(2.2)), "sky_inverse_exponent": dom & (y == F32(1.0 / 2.2))})
        if name in ("div", "slab_quotient"):
            y = np.asarray(y, F32)
            ey, ex = ((bits(y) >> 23) & 0xff).astype(I64), ((bits(x) >> 23) & 0xff).astype(I64)
            y_ok = (ey >= 127 - 40) & (ey <= 127 + 1)
            x_ok = (x == 0) | ((ex >= 127 - 60) & (ex < 127 + 40))
            return _count({"fast_path": y_ok & x_ok, "fast_path_zero_dividend": y_ok & (x == 0), "fast_path_minus_zero_dividend": y_ok & (x == 0) & neg,
                           "divisor_below_guard": (ey < 127 - 40) & x_ok, "divisor_above_guard": (ey > 127 + 1) & x_ok, "divisor_just_below_2^-40": (ey == 127 - 41) & x_ok,
                           "divisor_first_above_guard": (ey == 127 + 2) & x_ok, "operand_below_guard": y_ok & (x != 0) & (ex < 127 - 60),
                           "operand_above_guard": y_ok & (ex >= 127 + 40), "operand_denormal": y_ok & (x != 0) & (ex == 0), "divisor_zero": y == 0,
                           "divisor_nan": np.isnan(y), "dividend_nan": nan, "both_inf": np.isinf(x) & np.isinf(y), "both_zero": (x == 0) & (y == 0),
                           "quotient_denormal": np.isfinite(d) & (np.abs(d / y.astype(F64)) < 2.0 ** -126) & (d != 0) & np.isfinite(y)})
        if name in ("fmin", "fmax"):
            y = np.asarray(y, F32)
            snan = lambda v: np.isnan(v) & ((bits(v) & 0x00400000) == 0)
            return _count({"first_smaller": x < y, "first_larger": x > y, "equal": (x == y) & (x != 0), "zeros_of_equal_sign": (x == 0) & (y == 0) & (neg == np.signbit(y)),
                           "plus_zero_minus_zero": (x == 0) & (y == 0) & ~neg & np.signbit(y), "minus_zero_plus_zero": (x == 0) & (y == 0) & neg & ~np.signbit(y),
                           "first_nan": nan & ~np.isnan(y), "second_nan": ~nan & np.isnan(y), "both_nan": nan & np.isnan(y), "first_signalling": snan(x) & ~np.isnan(y),
                           "second_signalling": ~nan & snan(y), "first_quiet": nan & ~snan(x) & ~np.isnan(y), "second_quiet": ~nan & np.isnan(y) & ~snan(y),
                           "infinity_against_nan": np.isinf(x) & np.isnan(y), "denormal_operand": ((ax > 0) & (ax < 2.0 ** -126)) & ~np.isnan(y)})
        if name in ("floor", "ceil"):
            return _count({"nan": nan, "inf": np.isinf(x), "integer": _is_int(x), "from_2^23": np.isfinite(x) & (ax >= 2.0 ** 23), "fraction_positive": (x > 0) & ~_is_int(x) & np.isfinite(x),
                           "fraction_negative": (x < 0) & ~_is_int(x) & np.isfinite(x), "below_one_positive": (x > 0) & (x < 1), "below_one_negative": (x < 0) & (x > -1),
                           "plus_zero": (x == 0) & ~neg, "minus_zero": (x == 0) & neg, "denormal": (ax > 0) & (ax < 2.0 ** -126)})
        if name == "f2u32_sat":
            return _count({"nan": nan, "negative": x < 0, "zero": x == 0, "saturates": x >= 4294967296.0, "below_one": (x > 0) & (x < 1), "fraction": (x > 1) & ~_is_int(x),
                           "from_2^31": (x >= 2147483648.0) & (x < 4294967296.0), "below_2^31": (x >= 1) & (x < 2147483648.0), "plus_inf": x == np.inf})
        if name == "powi5":
            p = d ** 5
            return _count({"nan": nan, "overflows": np.isfinite(x) & (np.abs(p) >= 2.0 ** 128), "square_overflows_first": np.isfinite(x) & (d * d >= 2.0 ** 128),
                           "normal": (np.abs(p) >= 2.0 ** -126) & (np.abs(p) < 2.0 ** 128), "denormal": (np.abs(p) < 2.0 ** -126) & (np.abs(p) > 2.0 ** -149),
                           "underflows": (x != 0) & (np.abs(p) < 2.0 ** -150), "square_denormal": (x != 0) & (d * d < 2.0 ** -126),
                           "negative": x < 0, "zero": x == 0, "inf": np.isinf(x)})
        if name == "abs":
            return _count({"nan_sign_set": nan & neg, "nan_sign_clear": nan & ~neg, "negative": (x < 0), "positive": x > 0, "minus_zero": (x == 0) & neg, "minus_inf": x == -np.inf})
    raise KeyError(name)
