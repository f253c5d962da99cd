"""The device math primitives on their own terms (cloudsc_dev.h, cloudsc_libm.h):
each runs element-wise on the GPU through the kernels' own functions
(cloudsc_debug_fp64_libm, cloudsc_debug_fp32_libm) and is compared bit for bit
with the host C library's exp / pow / expf / powf -- what the reference kernel
calls -- and with IEEE division and sqrt, over the argument sets of
tests/device_math_cases.py: the physics' ranges, the edges of every range
check, special values, random bit patterns, in wave layouts that make lanes
diverge, at workgroup sizes 64 (the LDS table copy loops) and 256."""
import numpy as np
import pytest

import cloudsc_amd as ca
import device_math_cases as dm
from gpu_harness import lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
needs_fma = pytest.mark.skipif(not dm.has_fma(),
                               reason="the host C library's non-FMA variant rounds differently in rare cases")
BLOCKS = (64, 256)


def run64(lib, which, block, x, y=None):
    out = np.full(x.size, 12345.0)
    ca.check(lib.cloudsc_debug_fp64_libm(0, which, block, x.ctypes.data, y.ctypes.data if y is not None else None,
                                         out.ctypes.data, x.size))
    return out


def run32(lib, which, x, y):
    out = np.full(x.size, 12345.0, np.float32)
    ca.check(lib.cloudsc_debug_fp32_libm(0, which, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size))
    return out


def assert_bits(got, want, what, *args):
    bad = dm.mismatches(got, want)
    print("%s: %d elements, %d mismatches" % (what, got.size, bad.size))
    assert bad.size == 0, what + ": " + dm.describe(bad, got, want, *args)


@needs_fma
def test_exp_bitwise_vs_host_libm(lib):
    """cl_exp_impl (hot body from LDS, range check after it, divergent branch
    to the complete function) and cl_exp_cold on every argument, against the
    host exp; the two must also agree with each other."""
    x, want = dm.exp_args(), dm.exp_reference()
    for block in BLOCKS:
        hot = run64(lib, 0, block, x)
        cold = run64(lib, 8, block, x)
        assert_bits(hot, want, "exp split, block %d" % block, x)
        assert_bits(cold, want, "exp complete, block %d" % block, x)
        assert_bits(cold, hot, "exp complete vs split, block %d" % block, x)


@needs_fma
def test_exp_pair_bitwise_vs_host_libm(lib):
    """exp_pair_split: both results, with the two arguments independently in
    and out of the hot range (whole waves and single lanes of each mix)."""
    x, y = dm.exp_pair_args()
    hx, hy = dm.exp_hot(x), dm.exp_hot(y)
    for a in (True, False):
        for b in (True, False):
            assert np.count_nonzero((hx == a) & (hy == b)) >= 1000
    want_x = dm.exp_reference()
    want_y = dm.host_exp(y)
    for block in BLOCKS:
        assert_bits(run64(lib, 2, block, x, y), want_x, "exp pair first, block %d" % block, x, y)
        assert_bits(run64(lib, 3, block, x, y), want_y, "exp pair second, block %d" % block, x, y)


@needs_fma
def test_pow_bitwise_vs_host_libm(lib):
    """cl_powr (pow_split) and cl_pow_cold on every pair, against the host pow."""
    x, y = dm.pow_args()
    want = dm.pow_reference()
    for block in BLOCKS:
        hot = run64(lib, 1, block, x, y)
        cold = run64(lib, 9, block, x, y)
        assert_bits(hot, want, "pow split, block %d" % block, x, y)
        assert_bits(cold, want, "pow complete, block %d" % block, x, y)
        assert_bits(cold, hot, "pow complete vs split, block %d" % block, x, y)


def test_division_bitwise_vs_ieee(lib):
    """cl_div, cl_div with cl_recip and the known-divisor form are the IEEE
    quotient, bit for bit, wherever operands, reciprocal, quotient and residual
    are normal (device_math_cases.div_args)."""
    n, d, _ = dm.div_args()
    want = n / d
    assert np.all(np.isfinite(want)) and np.all(np.abs(want) >= 2.0 ** -1000)
    for block in BLOCKS:
        q4 = run64(lib, 4, block, n, d)
        assert_bits(q4, want, "cl_div, block %d" % block, n, d)
        for which, name in ((5, "cl_recip"), (6, "known divisor")):
            q = run64(lib, which, block, n, d)
            assert_bits(q, want, "%s division, block %d" % (name, block), n, d)
            assert_bits(q, q4, "%s division vs cl_div, block %d" % (name, block), n, d)


# What cl_div gives for a zero numerator, by the sign combination (n, d):
# a zero of the IEEE sign except -0 / +d, which is +0 (IEEE: -0).  q = n * r
# has the IEEE sign; the residual fma(-d, q, n) of two zeros of opposite sign
# is +0, and the last fma adds (+0 * r) to q: (-0) + (+0) = +0 when r > 0.
ZERO_SIGNS_CL_DIV = {("+0", "+d"): "+0", ("+0", "-d"): "-0", ("-0", "+d"): "+0", ("-0", "-d"): "+0"}
ZERO_SIGNS_IEEE = {("+0", "+d"): "+0", ("+0", "-d"): "-0", ("-0", "+d"): "-0", ("-0", "-d"): "+0"}


def zero_signs(n, d, q):
    """{(sign of n, sign of d): the set of results seen} for zero numerators."""
    seen = {}
    for sn in (False, True):
        for sd in (False, True):
            m = (np.signbit(n) == sn) & (np.signbit(d) == sd)
            assert m.sum() >= 250
            assert np.all(q[m] == 0), q[m]
            seen["-0" if sn else "+0", "-d" if sd else "+d"] = set(np.where(np.signbit(q[m]), "-0", "+0").tolist())
    return seen


def test_division_zero_numerators(lib):
    """±0 / ±d is a zero in every form; its sign is the recorded one
    (ZERO_SIGNS_CL_DIV: not IEEE's for -0 / +d), in all three fp64 forms and
    in the fp32 cl_div.  The host form (n / d) is IEEE."""
    n, d = dm.div_zero_args()
    want = {k: {v} for k, v in ZERO_SIGNS_CL_DIV.items()}
    for which in (4, 5, 6):
        for block in BLOCKS:
            seen = zero_signs(n, d, run64(lib, which, block, n, d))
            print("fp64 which %d block %d: zero numerators %s" % (which, block, seen))
            assert seen == want, (which, block)
    nf, df = dm.div_zero_args(np.float32)
    seen = zero_signs(nf, df, run32(lib, 5, nf, df))
    print("fp32 cl_div: zero numerators %s" % seen)
    assert seen == want
    differ = [k for k in ZERO_SIGNS_IEEE if ZERO_SIGNS_IEEE[k] != ZERO_SIGNS_CL_DIV[k]]
    assert differ == [("-0", "+d")]


def test_division_out_of_range_recorded(lib):
    """Outside cl_div's domain (subnormal, zero or huge divisors, quotients
    that under- or overflow, non-finite operands) the result is not asserted
    to be IEEE's; this prints what the device gives, so that a change shows
    in the log."""
    n = np.array([p[0] for p in dm.DIV_OUT_OF_RANGE])
    d = np.array([p[1] for p in dm.DIV_OUT_OF_RANGE])
    with np.errstate(all="ignore"):
        want = n / d
    for which in (4, 5, 6):
        q = run64(lib, which, 64, n, d)
        for i in range(n.size):
            same = dm.mismatches(q[i:i + 1], want[i:i + 1]).size == 0
            print("which %d: %s / %s = %s  (IEEE %s)%s" % (which, float(n[i]).hex(), float(d[i]).hex(),
                                                          float(q[i]).hex(), float(want[i]).hex(),
                                                          "" if same else "  DIFFERS"))


def test_sqrt_bitwise_vs_ieee(lib):
    """sqrt as the exact kernels call it is correctly rounded: normal and
    subnormal arguments, exact squares, ±0, inf, negative arguments (NaN)."""
    x = dm.sqrt_args()
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    for block in BLOCKS:
        assert_bits(run64(lib, 7, block, x), want, "sqrt, block %d" % block, x)


@needs_fma
def test_fp32_exact_libm_bitwise_vs_host_libm(lib):
    """The exact single-precision forms (CLOUDSC_FP32_EXACT_LIBM: which 2, 3)
    against the host expf / powf they restate, bit for bit."""
    x = dm.expf_args()
    assert_bits(run32(lib, 2, x, x), dm.host_expf(x), "expf exact", x)
    px, py = dm.powf_args()
    assert_bits(run32(lib, 3, px, py), dm.host_powf(px, py), "powf exact", px, py)


def test_fp32_exact_division_bitwise_vs_ieee(lib):
    """The exact fp32 kernels' cl_div over its whole domain -- normal divisors
    2^-126 <= |d| < 2^126, numerators 2^-100 <= |n| <= 2^100 -- is the IEEE
    quotient wherever that is finite and normal, down to |q| = 2^-126."""
    n, d = dm.divf_args()
    with np.errstate(over="ignore", under="ignore"):
        want = (n / d).astype(np.float32)
    ok = np.isfinite(want) & (np.abs(want) >= np.finfo(np.float32).tiny)
    small = ok & (np.abs(want) < 2.0 ** -100)
    print("fp32 cl_div: %d asserted quotients, %d of them below 2^-100" % (ok.sum(), small.sum()))
    assert small.sum() >= 1000
    q = run32(lib, 5, n, d)
    assert_bits(q[ok], want[ok], "fp32 cl_div", n[ok], d[ok])
