"""The argument sets and references of tests/device_math_cases.py, checked
without a GPU: every set holds the classes it claims (the device's hot / cold
predicates restated in numpy), every wave layout pattern is present, the host
C library's exp / pow are within their documented error of the exact values,
and numpy's division of the zero-numerator set has IEEE signs."""
import ctypes as C
import os

import numpy as np
import pytest

import cloudsc_amd as ca
import device_math_cases as dm

MIN_PER_CLASS = 1000


def test_exp_set_holds_every_class():
    x = dm.exp_args()
    assert x.size % 256 != 0 and not x.flags.writeable
    for name, m in dm.exp_classes(x).items():
        assert np.count_nonzero(m) >= MIN_PER_CLASS, name
    # both sides of every threshold of the range checks, to the last bit
    for edge in (512.0, -512.0, 1024.0, -1024.0, dm.EXP_MAX, dm.EXP_MIN, 2.0 ** -54, -2.0 ** -54):
        for v in (edge, np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf)):
            assert np.any(dm.bits(x) == dm.bits(np.array([v]))[0]), float(v).hex()
    for v in (0.0, -0.0, np.inf, -np.inf, 5e-324):
        assert np.any(dm.bits(x) == dm.bits(np.array([v]))[0])
    assert np.isnan(x).sum() >= MIN_PER_CLASS


def check_layout(hot):
    """The layout section's hot mask is each pattern's, group by group."""
    assert dm.LAYOUT_LEN % dm.WAVE == 0
    for name, start, stop in dm.layout_segments():
        groups = hot[start:stop].reshape(-1, dm.WAVE)
        assert groups.shape[0] == dm.GROUPS
        assert np.array_equal(groups, np.tile(dm.pattern_mask(name), (dm.GROUPS, 1))), name
    masks = {p: dm.pattern_mask(p) for p in dm.PATTERNS}
    assert masks["hot"].all() and not masks["cold"].any()
    for lane in (0, 31, 32, 63):
        assert np.flatnonzero(~masks["cold%d" % lane]).tolist() == [lane]
    assert np.array_equal(masks["alt_even_hot"], np.arange(64) % 2 == 0)
    assert np.array_equal(masks["alt_odd_hot"], np.arange(64) % 2 == 1)


def test_exp_layout_patterns():
    check_layout(dm.exp_hot(dm.exp_args()))


def test_exp_pair_mixes():
    x, y = dm.exp_pair_args()
    assert x.size == y.size and x.size % 256 != 0
    hx, hy = dm.exp_hot(x), dm.exp_hot(y)
    for a in (True, False):
        for b in (True, False):
            assert np.count_nonzero((hx == a) & (hy == b)) >= MIN_PER_CLASS, (a, b)
    # whole waves of each mix, and waves in which single lanes differ
    n = dm.LAYOUT_LEN // dm.WAVE
    gx, gy = hx[:dm.LAYOUT_LEN].reshape(n, dm.WAVE), hy[:dm.LAYOUT_LEN].reshape(n, dm.WAVE)
    for a in (True, False):
        for b in (True, False):
            assert np.any(np.all(gx == a, axis=1) & np.all(gy == b, axis=1)), (a, b)
    either_cold = ~(gx & gy)
    assert np.any(either_cold.sum(axis=1) == 1)


def test_pow_set_holds_every_class():
    x, y = dm.pow_args()
    assert x.size == y.size and x.size % 256 != 0
    for name, m in dm.pow_classes(x, y).items():
        assert np.count_nonzero(m) >= MIN_PER_CLASS, name
    # the Cartesian product of the special values is there, pair by pair
    bx, by = dm.bits(x), dm.bits(y)
    for sx in dm.POW_SPECIAL_X:
        for sy in dm.POW_SPECIAL_Y:
            m = (bx == dm.bits(np.array([sx]))[0]) & (by == dm.bits(np.array([sy]))[0])
            assert m.any(), (sx, sy)
    # the physics' exponents on the physics' bases
    for e in dm.POW_PHYSICS_EXPONENTS:
        assert np.count_nonzero((y == e) & (x >= 1e-12) & (x <= 1e8)) >= MIN_PER_CLASS, e
    # results that overflow, underflow and are subnormal, from 2^y
    two = x == 2.0
    assert np.count_nonzero(two & (y >= 1024)) >= 100 and np.count_nonzero(two & (y < -1075)) >= 100
    assert np.count_nonzero(two & (y > -1074) & (y < -1022)) >= MIN_PER_CLASS
    with np.errstate(invalid="ignore"):
        near1 = (np.abs(x - 1.0) < 2e-15) & (x != 1.0)
    assert np.count_nonzero(near1 & (np.abs(y) > 2.0 ** 40)) >= MIN_PER_CLASS


def test_pow_layout_patterns():
    x, y = dm.pow_args()
    base_ok, y_ok, exp_ok = dm.pow_predicates(x, y)
    check_layout(base_ok & y_ok & exp_ok)


def test_division_sets():
    n, d, parts = dm.div_args()
    assert n.size == d.size and n.size % 256 != 0
    rng = np.random.default_rng(1)
    _, sel = dm.div_operands(rng, dm.N_RANDOM, 300)
    for k in range(4):
        assert np.count_nonzero(sel == k) >= MIN_PER_CLASS
    lo, hi = parts["e300"], parts["cloudsc"]
    mant = dm.bits(n[lo:hi]) & np.uint64(0xfffffffffffff)
    assert np.count_nonzero(mant == 0xfffffffffffff) >= MIN_PER_CLASS      # all ones
    assert np.count_nonzero(mant == 0) >= MIN_PER_CLASS                    # powers of two
    assert np.count_nonzero((mant >> np.uint64(20)) == 0xffffffff) >= MIN_PER_CLASS
    for a in (n, d):
        assert np.count_nonzero(a[lo:hi] < 0) >= MIN_PER_CLASS and np.count_nonzero(a[lo:hi] > 0) >= MIN_PER_CLASS
        e = np.frexp(a)[1]
        assert e.min() >= -500 and e.max() <= 502
        assert np.count_nonzero(np.abs(e) > 300) >= MIN_PER_CLASS
    # every intermediate of cl_div stays normal: quotient, reciprocal, residual (about 2^-53 n)
    q = n / d
    assert np.all(np.isfinite(q)) and np.abs(q).min() >= 2.0 ** -1001 and np.abs(q).max() <= 2.0 ** 1001
    assert np.abs(n).min() * 2.0 ** -106 >= 2.0 ** -1022


def test_zero_numerator_reference_has_ieee_signs():
    for dtype in (np.float64, np.float32):
        n, d = dm.div_zero_args(dtype)
        assert n.dtype == dtype and np.all(n == 0) and np.all(d != 0)
        q = n / d
        assert np.all(q == 0)
        assert np.array_equal(np.signbit(q), np.signbit(n) != np.signbit(d))
        for sn in (False, True):
            for sd in (False, True):
                assert np.count_nonzero((np.signbit(n) == sn) & (np.signbit(d) == sd)) >= 250


def test_sqrt_and_fp32_sets():
    x = dm.sqrt_args()
    assert x.size % 256 != 0
    sub = (x > 0) & (x < 2.0 ** -1022)
    assert np.count_nonzero(sub) >= MIN_PER_CLASS and np.count_nonzero(x < 0) >= MIN_PER_CLASS
    r = np.sqrt(np.where(x > 0, x, 1.0))
    assert np.count_nonzero((r * r == x) & (x > 0) & (r == np.floor(r)) & (r > 1)) >= MIN_PER_CLASS   # exact squares
    xf = dm.expf_args()
    assert xf.dtype == np.float32 and xf.size % 256 != 0
    assert np.count_nonzero(np.abs(xf) >= 88) >= MIN_PER_CLASS
    assert np.count_nonzero((xf > -103.98) & (xf < -87.33)) >= MIN_PER_CLASS
    px, py = dm.powf_args()
    assert px.dtype == np.float32 and px.size == py.size and px.size % 256 != 0
    nf, df = dm.divf_args()
    assert np.abs(df).min() >= 2.0 ** -126 and np.abs(df).max() < 2.0 ** 126
    assert np.abs(nf).min() >= 2.0 ** -100 and np.abs(nf).max() <= 2.0 ** 100


def ulp_error(got, exact_fn, args):
    """|got - exact| in ulps of got, the exact value from mpmath at 200 bits."""
    import mpmath
    worst = 0.0
    with mpmath.workprec(200):
        for i in range(len(got)):
            g = float(got[i])
            exact = exact_fn(*(mpmath.mpf(float(a[i])) for a in args))
            ulp = mpmath.mpf(float(np.spacing(abs(g))))
            worst = max(worst, float(abs(mpmath.mpf(g) - exact) / ulp))
    return worst


@pytest.mark.skipif(not dm.has_fma(), reason="the host C library's non-FMA variant rounds differently in rare cases")
def test_host_libm_within_one_ulp_of_exact():
    """glibc documents exp and pow below 0.52 ulp; the bound here is that
    rounded up to the next whole ulp, over 4096 arguments with finite normal
    results."""
    mpmath = pytest.importorskip("mpmath")
    rng = np.random.default_rng(3)
    x, want = dm.exp_args(), dm.exp_reference()
    ok = np.flatnonzero(np.isfinite(want) & (want >= 2.0 ** -1022) & np.isfinite(x))
    pick = rng.choice(ok, 4096, replace=False)
    e = ulp_error(want[pick], mpmath.exp, (x[pick],))
    print("host exp: worst error %.4f ulp over 4096 arguments" % e)
    assert e <= 1.0
    px, py = dm.pow_args()
    pw = dm.pow_reference()
    ok = np.flatnonzero(np.isfinite(pw) & (pw >= 2.0 ** -1022) & np.isfinite(px) & np.isfinite(py) & (px > 0))
    pick = rng.choice(ok, 4096, replace=False)
    e = ulp_error(pw[pick], mpmath.power, (px[pick], py[pick]))
    print("host pow: worst error %.4f ulp over 4096 arguments" % e)
    assert e <= 1.0


def test_references_are_the_c_library():
    """Spot values through the ctypes route, and the float forms really are
    single precision."""
    assert dm.host_exp(np.array([0.0, 1.0]))[1] == 2.718281828459045
    assert dm.host_pow(np.array([2.0, -8.0]), np.array([0.5, 1.0 / 3.0]))[0] == 1.4142135623730951
    assert np.isnan(dm.host_pow(np.array([-8.0]), np.array([1.0 / 3.0]))[0])
    ef = dm.host_expf(np.array([1.0], np.float32))
    assert ef.dtype == np.float32 and ef[0] == np.float32(2.7182817)
    got = np.array([np.nan, 0.0, -0.0, np.inf, 1.0])
    want = np.array([-np.nan, 0.0, 0.0, np.inf, np.nextafter(1.0, 2.0)])
    assert dm.mismatches(got, want).tolist() == [2, 4]           # NaN payloads ignored; signed zeros are not


def test_debug_fp64_libm_argument_checks():
    """Bad arguments are CLOUDSC_EINVAL before any HIP call: block sizes other
    than 64, 128, 256, unknown codes, null arrays, a missing y where it is read."""
    if not os.path.exists(ca.LIB_PATH):
        pytest.skip("libcloudsc_amd.so not built (__graft_entry__.build())")
    lib = C.CDLL(ca.LIB_PATH)
    lib.cloudsc_debug_fp64_libm.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_longlong]
    x = np.ones(8)
    out = np.zeros(8)
    px, po = x.ctypes.data, out.ctypes.data
    for block in (0, 1, 32, 63, 65, 192, 512, 1024, -64):
        assert lib.cloudsc_debug_fp64_libm(0, 0, block, px, px, po, 8) == ca.EINVAL, block
    for which in (-1, 10, 100):
        assert lib.cloudsc_debug_fp64_libm(0, which, 64, px, px, po, 8) == ca.EINVAL, which
    assert lib.cloudsc_debug_fp64_libm(0, 0, 64, None, px, po, 8) == ca.EINVAL
    assert lib.cloudsc_debug_fp64_libm(0, 0, 64, px, px, None, 8) == ca.EINVAL
    assert lib.cloudsc_debug_fp64_libm(0, 0, 64, px, px, po, 0) == ca.EINVAL
    for which in (1, 2, 3, 4, 5, 6, 9):
        assert lib.cloudsc_debug_fp64_libm(0, which, 64, px, None, po, 8) == ca.EINVAL, which
