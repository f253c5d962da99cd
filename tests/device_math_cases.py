"""Argument sets and references for the device math primitives
(dwarf-p-cloudsc_amd/csrc/cloudsc_dev.h, cloudsc_libm.h), shared by
tests/test_device_math_gpu.py (runs them on the device through
cloudsc_debug_fp64_libm / cloudsc_debug_fp32_libm) and
tests/test_device_math_cases_cpu.py (keeps the sets and references honest).

References: exp, pow, expf, powf are the host C library's, through ctypes --
the functions the reference kernel calls (numpy's exp differs from them by
1 ulp on random arguments).  Division and sqrt are numpy's, which are IEEE.

Layout: wave divergence is part of what is tested, so every exp / pow set
begins with a section of whole 64-lane groups (PATTERNS): all hot, all cold,
hot with one cold lane at 0, 31, 32 or 63, and strictly alternating lanes.
"hot" is the device's own predicate (the inline path), "cold" the arguments
that take the out-of-line complete function.  No set's length is a multiple
of 256, so the last workgroup is partial at every block size.

Every set is generated once per process and returned read-only."""
import ctypes
import functools

import numpy as np

WAVE = 64
GROUPS = 16                      # 64-lane groups per layout pattern
N_RANDOM = (1 << 17) + 37        # length of the large random sets
PATTERNS = ("hot", "cold", "cold0", "cold31", "cold32", "cold63", "alt_even_hot", "alt_odd_hot")
LAYOUT_LEN = len(PATTERNS) * GROUPS * WAVE

EXP_MAX = float.fromhex("0x1.62e42fefa39efp+9")      # largest x with a finite exp(x), 709.78...
EXP_MIN = float.fromhex("-0x1.74910d52d3051p+9")     # below it exp(x) rounds to 0, -745.13...
POW_PHYSICS_EXPONENTS = (0.333, 0.4, 0.5777, 0.666, 1.5, 3.0, 2.47, -1.79)


def has_fma():
    """The host C library's non-FMA variant rounds differently in rare cases
    (tests/test_libm.py): the libm comparisons need a host with FMA."""
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read()
    except OSError:
        return False


# ---------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def _libm():
    lib = ctypes.CDLL("libm.so.6")
    for name in ("exp", "pow"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_double
        fn.argtypes = [ctypes.c_double] * (2 if name == "pow" else 1)
    for name in ("expf", "powf"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float] * (2 if name == "powf" else 1)
    return lib


def _map(fn, dtype, *args):
    cols = [np.ascontiguousarray(a, dtype=dtype).tolist() for a in args]
    return np.array([fn(*v) for v in zip(*cols)], dtype=dtype)


def host_exp(x):
    return _map(_libm().exp, np.float64, x)


def host_pow(x, y):
    return _map(_libm().pow, np.float64, x, y)


def host_expf(x):
    return _map(_libm().expf, np.float32, x)


def host_powf(x, y):
    return _map(_libm().powf, np.float32, x, y)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def mismatches(got, want):
    """Indices where got is not want: raw bits (signed zeros and infinities
    included), except that where want is NaN any NaN will do (x86 and the GPU
    propagate payloads differently)."""
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), bits(got) != bits(want))
    return np.flatnonzero(bad)


def describe(idx, got, want, *args, limit=6):
    """The first few mismatches as text, for an assertion message."""
    rows = []
    for i in idx[:limit]:
        rows.append("[%d] args %s got %s want %s" % (i, tuple(float(a[i]).hex() for a in args),
                                                     float(got[i]).hex(), float(want[i]).hex()))
    return "%d mismatches: %s" % (len(idx), "; ".join(rows))


# -------------------------------------------------------------------- layout
def pattern_mask(name):
    """The hot lanes of one 64-lane group of pattern `name`."""
    m = np.ones(WAVE, bool)
    if name == "cold":
        m[:] = False
    elif name.startswith("cold"):
        m[int(name[4:])] = False
    elif name == "alt_even_hot":
        m[1::2] = False
    elif name == "alt_odd_hot":
        m[0::2] = False
    return m


def layout_mask():
    return np.concatenate([np.tile(pattern_mask(p), GROUPS) for p in PATTERNS])


def layout_segments():
    """(pattern, start, stop) of each pattern's groups in the layout section."""
    return [(p, i * GROUPS * WAVE, (i + 1) * GROUPS * WAVE) for i, p in enumerate(PATTERNS)]


def lay_out(hot, cold):
    """The layout section: rows of `hot` in the hot lanes and of `cold` in the
    cold ones, each pool taken in order (cyclically)."""
    m = layout_mask()
    out = np.empty((LAYOUT_LEN,) + hot.shape[1:], hot.dtype)
    out[m] = hot[np.arange(int(m.sum())) % len(hot)]
    out[~m] = cold[np.arange(int((~m).sum())) % len(cold)]
    return out


def neighbours(v, k=8):
    """v and its k nearest representable values on each side."""
    dt = np.dtype(type(v) if isinstance(v, np.generic) else np.float64)
    lo = hi = dt.type(v)
    out = [lo]
    with np.errstate(over="ignore"):
        for _ in range(k):
            lo = np.nextafter(lo, dt.type(-np.inf))
            hi = np.nextafter(hi, dt.type(np.inf))
            out += [lo, hi]
    return np.array(out, dt)


def random_bits(rng, n, dtype=np.float64):
    if dtype == np.float64:
        return rng.integers(0, 1 << 64, n, dtype=np.uint64).view(np.float64)
    return rng.integers(0, 1 << 32, n, dtype=np.uint32).view(np.float32)


def _f32(parts):
    return np.concatenate([np.asarray(p, np.float32) for p in parts])


def _finish(a):
    """Read-only, contiguous, and never a whole number of 256-thread workgroups."""
    if len(a) % 256 == 0:
        a = np.concatenate([a, a[:37]])
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


# ----------------------------------------------------------------------- exp
def exp_hot(x):
    """cloudsc_libm::exp_in_hot_range: the inline body's result is used."""
    return np.abs(x) < 512.0


def exp_classes(x):
    ax = np.abs(x)
    return {
        "hot": (ax >= 2.0 ** -54) & (ax < 512.0),
        "tiny": ax < 2.0 ** -54,                            # 1 + x in the complete function; hot on the device
        "large_pos": (x >= 512.0) & (x < 1024.0),           # exp_specialcase, k > 0 (overflow above EXP_MAX)
        "large_neg": (x <= -512.0) & (x > -1024.0),         # exp_specialcase, k < 0 (subnormal results, 0)
        "subnormal_result": (x >= -745.14) & (x <= -708.3),
        "huge": (ax >= 1024.0) & np.isfinite(x),
        "nonfinite": ~np.isfinite(x),
    }


@functools.lru_cache(maxsize=None)
def exp_args():
    rng = np.random.default_rng(20250301)
    u = rng.uniform
    nan_bits = (rng.integers(1, 1 << 52, 1024, dtype=np.uint64) | np.uint64(0x7ff0000000000000)
                | (rng.integers(0, 2, 1024, dtype=np.uint64) << np.uint64(63)))
    hot = np.concatenate([u(-40.0, 20.0, 4096), u(-512.0, 512.0, 4096)])
    hot = hot[np.abs(hot) < 512.0]
    cold = np.concatenate([u(512.0, EXP_MAX, 512), u(-745.14, -708.3, 512), u(-708.3, -512.0, 512),
                           u(EXP_MAX, 1024.0, 256), u(-1024.0, -745.2, 256), 10.0 ** u(3.1, 300.0, 256),
                           -10.0 ** u(3.1, 300.0, 256), [np.inf, -np.inf, np.nan] * 32])
    rng.shuffle(cold)
    tiny = np.concatenate([np.copysign(2.0 ** u(-1074.0, -54.0, 4000), u(-1, 1, 4000)),
                           [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, -2.0 ** -1022, 2.0 ** -1023],
                           neighbours(2.0 ** -54), neighbours(-2.0 ** -54)])
    x = np.concatenate([
        lay_out(hot, cold),
        u(-745.2, 709.8, N_RANDOM),
        u(-40.0, 20.0, 1 << 14),                                    # the CLOUDSC range
        tiny,
        neighbours(512.0), neighbours(-512.0), neighbours(1024.0), neighbours(-1024.0),
        neighbours(EXP_MAX), neighbours(EXP_MIN), neighbours(-708.3964185322641),   # log(2^-1022)
        u(-745.14, -708.3, 4096),                                   # subnormal results
        u(512.0, EXP_MAX, 4096),
        u(-708.3, -512.0, 2048),
        [np.inf, -np.inf, np.nan, -np.nan],
        nan_bits.view(np.float64),                                  # quiet and signaling NaNs
        random_bits(rng, 1 << 16),
    ])
    return _finish(x)


@functools.lru_cache(maxsize=None)
def exp_pair_args():
    """(x, y) for exp_pair_split: x is exp_args(); y is drawn independently
    (a permutation), except that its layout section is x's moved by half a
    pattern (and x's first all-hot groups meet all-cold ones), so whole waves
    of hot/hot, hot/cold, cold/hot and cold/cold occur beside every mixed one."""
    x = exp_args()
    rng = np.random.default_rng(20250302)
    y = x[rng.permutation(len(x))]
    half = WAVE * GROUPS // 2
    y[:LAYOUT_LEN] = np.roll(x[:LAYOUT_LEN], half)
    y[:half] = x[2 * half:3 * half]          # the first all-hot groups of x against all-cold ones
    return x, _finish(y)


@functools.lru_cache(maxsize=None)
def exp_reference():
    r = host_exp(exp_args())
    r.flags.writeable = False
    return r


# ----------------------------------------------------------------------- pow
def pow_predicates(x, y):
    """The three checks of cloudsc_libm::pow_split, restated: positive normal
    base, the exponent-field window of y (2^-65 <= |y| < 2^63), |y log x| < 512."""
    bx = bits(x).astype(np.uint64)
    base_ok = (bx - np.uint64(0x0010000000000000)) < np.uint64(0x7fe0000000000000)
    topy = ((bits(y) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    y_ok = (topy >= 0x3be) & (topy < 0x43e)
    with np.errstate(all="ignore"):
        exp_ok = np.abs(y * np.log(np.where(base_ok, x, 1.0))) < 512.0
    return base_ok, y_ok, exp_ok


def pow_classes(x, y):
    base_ok, y_ok, exp_ok = pow_predicates(x, y)
    sub = (np.abs(x) < 2.0 ** -1022) & (x != 0)
    return {
        "hot": base_ok & y_ok & exp_ok,
        "cold_base": ~base_ok,
        "cold_y": base_ok & ~y_ok,
        "cold_exp": base_ok & y_ok & ~exp_ok,               # checked after the log, before the exp body
        "subnormal_base": sub,
        "negative_base": (x < 0) & np.isfinite(x),
    }


POW_SPECIAL_X = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, float.fromhex("0x0.fffffffffffffp-1022"),
                 2.0 ** -1022, 1.7976931348623157e308, -2.0, -2.5, -3.0)
POW_SPECIAL_Y = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 0.5, 2.0, 3.0, -3.0, 1e-20, 1e20, 2.0 ** 53,
                 2.0 ** 53 + 2.0, 2.0 ** 62)


@functools.lru_cache(maxsize=None)
def pow_args():
    rng = np.random.default_rng(20250303)
    u = rng.uniform
    phys = np.array(POW_PHYSICS_EXPONENTS)

    def pairs(x, y):
        return np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], axis=1)

    hot = pairs(10.0 ** u(-12.0, 8.0, 8192), np.concatenate([rng.choice(phys, 4096), u(-3.0, 3.0, 4096)]))
    subn = (rng.integers(1, 1 << 52, 1024, dtype=np.uint64)).view(np.float64)
    cold = np.concatenate([
        pairs(subn, np.concatenate([rng.choice(phys, 512), u(-3.0, 3.0, 512)])),          # subnormal bases
        pairs(-10.0 ** u(-12.0, 8.0, 1024), rng.integers(-9, 10, 1024).astype(float)),     # negative, integer y
        pairs(-10.0 ** u(-3.0, 3.0, 256), u(-3.0, 3.0, 256)),                              # negative, NaN
        pairs(10.0 ** u(-12.0, 8.0, 512), np.copysign(2.0 ** u(-200.0, -66.0, 512), u(-1, 1, 512))),   # |y| tiny
        pairs(10.0 ** u(-12.0, 8.0, 256), np.copysign(2.0 ** u(63.0, 200.0, 256), u(-1, 1, 256))),     # |y| huge
        pairs(2.0 ** u(-1000.0, 1000.0, 1024), np.copysign(u(30.0, 3000.0, 1024), u(-1, 1, 1024))),    # exp range
        pairs([0.0, -0.0, np.inf, -np.inf, np.nan] * 32, u(-3.0, 3.0, 160)),
    ])
    base_ok, y_ok, exp_ok = pow_predicates(cold[:, 0].copy(), cold[:, 1].copy())
    cold = cold[~(base_ok & y_ok & exp_ok)]
    rng.shuffle(cold)
    sx, sy = np.meshgrid(np.array(POW_SPECIAL_X), np.array(POW_SPECIAL_Y), indexing="ij")
    near1 = np.concatenate([neighbours(1.0, 8)[1:]] * 256)
    p = np.concatenate([
        lay_out(hot, cold),
        pairs(10.0 ** u(-12.0, 8.0, (1 << 16) + 37), rng.choice(phys, (1 << 16) + 37)),
        pairs(10.0 ** u(-12.0, 8.0, 1 << 16), u(-3.0, 3.0, 1 << 16)),
        pairs(sx.ravel(), sy.ravel()),
        pairs(np.full(2048, 2.0), u(1020.0, 1025.0, 2048)),                # overflow
        pairs(np.full(2048, 2.0), u(-1080.0, -1020.0, 2048)),              # underflow, subnormal results
        pairs(np.full(172, 2.0), np.concatenate([np.arange(1019.0, 1026.0), np.arange(-1080.0, -1019.0),
                                                 neighbours(1024.0), neighbours(-1022.0), neighbours(-1074.0),
                                                 neighbours(-1075.0), [0.5] * 36])),
        pairs(near1, np.copysign(2.0 ** u(0.0, 62.0, len(near1)), u(-1, 1, len(near1)))),
        pairs(subn, u(-3.0, 3.0, 1024)),
        pairs(random_bits(rng, 1 << 16), random_bits(rng, 1 << 16)),
        pairs(np.abs(random_bits(rng, 1 << 14)), u(-3.0, 3.0, 1 << 14)),   # any positive base, ordinary y
    ])
    return _finish(p[:, 0]), _finish(p[:, 1])


@functools.lru_cache(maxsize=None)
def pow_reference():
    r = host_pow(*pow_args())
    r.flags.writeable = False
    return r


# ------------------------------------------------------------------ division
def div_operands(rng, n, e):
    """Operands as tools/div_check.hip's rnd() draws them: exponent uniform in
    [-e, e], random sign, mantissa all ones / zero / many leading ones (one in
    16 each) or random.  Returns the values and the mantissa class (0, 1, 2,
    3 = random)."""
    ex = rng.integers(-e, e + 1, n)
    mant = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    sel = rng.integers(0, 16, n)
    mant = np.where(sel == 0, np.uint64(0xfffffffffffff), mant)
    mant = np.where(sel == 1, np.uint64(0), mant)
    mant = np.where(sel == 2, mant | np.uint64(0xffffffff00000), mant)
    sign = rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63)
    b = ((ex + 1023).astype(np.uint64) << np.uint64(52)) | mant | sign
    return b.view(np.float64), np.minimum(sel, 3)


@functools.lru_cache(maxsize=None)
def div_args():
    """The asserted domain: (n, d, start of each named part).  Every operand
    and quotient is normal and far enough from the ends of the range that the
    reciprocal, the quotient and the residual of cl_div are normal too."""
    rng = np.random.default_rng(20250304)
    n300, _ = div_operands(rng, N_RANDOM, 300)
    d300, _ = div_operands(rng, N_RANDOM, 300)
    nc = 10.0 ** rng.uniform(-12.0, 5.0, 1 << 14) * rng.choice([-1.0, 1.0], 1 << 14)
    dc = 10.0 ** rng.uniform(-12.0, 5.0, 1 << 14)
    n500, _ = div_operands(rng, 1 << 16, 500)
    d500, _ = div_operands(rng, 1 << 16, 500)
    parts = {"e300": 0, "cloudsc": N_RANDOM, "e500": N_RANDOM + (1 << 14)}
    return (_finish(np.concatenate([n300, nc, n500])), _finish(np.concatenate([d300, dc, d500])), parts)


@functools.lru_cache(maxsize=None)
def div_zero_args(dtype=np.float64):
    """±0 / ±d, 256 divisors per sign combination, in the order (+0, +d),
    (+0, -d), (-0, +d), (-0, -d)."""
    rng = np.random.default_rng(20250305)
    e = 300 if dtype == np.float64 else 100
    d = np.abs(2.0 ** rng.uniform(-e, e, 256)).astype(dtype)
    z = np.zeros(256, dtype)
    return (_finish(np.concatenate([z, z, -z, -z])[:-3]), _finish(np.concatenate([d, -d, d, -d])[:-3]))


# (n, d) outside cl_div's domain: recorded by the GPU test, not asserted
DIV_OUT_OF_RANGE = (
    (1.0, 5e-324), (1.0, 2.0 ** -1030), (1.0, 2.0 ** -1023), (1.0, 0.0), (1.0, -0.0), (0.0, 0.0), (0.0, 2.0 ** -1030),
    (1.0, 2.0 ** 1022), (1.0, 1.5 * 2.0 ** 1022), (1.0, 2.0 ** 1023), (1.0, 1.7976931348623157e308),
    (0.0, 2.0 ** 1023), (1e300, 1e-300), (1e-300, 1e300), (2.0 ** -1000, 2.0 ** 60), (3.0 * 2.0 ** -1000, 7.0),
    (3.0 * 2.0 ** -1060, 7.0 * 2.0 ** -50), (np.inf, 3.0), (3.0, np.inf), (np.nan, 3.0), (3.0, np.nan), (np.inf, np.inf),
)


# ---------------------------------------------------------------------- sqrt
@functools.lru_cache(maxsize=None)
def sqrt_args():
    rng = np.random.default_rng(20250306)
    k = rng.integers(1, 1 << 26, 4096).astype(np.float64)
    m = rng.integers(1 << 25, 1 << 26, 2048).astype(np.float64) * 2.0 ** rng.integers(-500, 480, 2048)
    x = np.concatenate([
        2.0 ** rng.uniform(-1022.0, 1023.9, 1 << 15) * (rng.uniform(1.0, 2.0, 1 << 15) / 2.0),
        rng.integers(1, 1 << 52, 4096, dtype=np.uint64).view(np.float64),            # subnormal
        k * k, m * m,                                                                # exact squares
        neighbours(1.0), neighbours(4.0), neighbours(2.0 ** -1022), neighbours(1.7976931348623157e308)[:1],
        [0.0, -0.0, np.inf, 5e-324, np.nan, -np.inf, -5e-324, -1.0],
        -10.0 ** rng.uniform(-300.0, 300.0, 1024),                                   # negative: NaN
        np.abs(random_bits(rng, 1 << 14)),
    ])
    return _finish(x)


# -------------------------------------------------------- fp32 exact forms
@functools.lru_cache(maxsize=None)
def expf_args():
    rng = np.random.default_rng(20250307)
    u = rng.uniform
    f = np.float32
    x = _f32([
        u(-40.0, 20.0, 1 << 16), u(-87.0, 87.0, (1 << 16) + 37),                 # the ranges of test_fp32_fast_libm_ulp
        u(88.0, 110.0, 4096), u(-110.0, -88.0, 4096),                            # |x| >= 88: the complete function
        u(-103.98, -87.33, 4096),                                                # subnormal results
        np.copysign(2.0 ** u(-149.0, -20.0, 2048), u(-1, 1, 2048)),
        neighbours(f(88.0)), neighbours(f(-88.0)), neighbours(f(88.72284)), neighbours(f(-87.33655)),
        neighbours(f(-103.972084)), neighbours(f(-103.2789)),
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754944e-38, 3.4028235e38, -3.4028235e38], f),
        random_bits(rng, 1 << 16, np.float32),
    ])
    return _finish(x)


@functools.lru_cache(maxsize=None)
def powf_args():
    rng = np.random.default_rng(20250308)
    u = rng.uniform
    f = np.float32
    phys = np.array(POW_PHYSICS_EXPONENTS)
    sx = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, 1.1754942e-38, 1.1754944e-38, 3.4028235e38,
                   -2.0, -2.5, -3.0], f)
    sy = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 0.5, 2.0, 3.0, -3.0, 1e-20, 1e20, 2.0 ** 24,
                   2.0 ** 24 + 2.0, 2.0 ** 62], f)
    gx, gy = np.meshgrid(sx, sy, indexing="ij")
    subn = rng.integers(1, 1 << 23, 1024, dtype=np.uint32).view(np.float32)
    x = _f32([
        10.0 ** u(-12.0, 8.0, (1 << 17) + 37),
        gx.ravel(),
        np.full(2048, 2.0), np.full(2048, 2.0),
        subn,
        -10.0 ** u(-6.0, 6.0, 1024),
        random_bits(rng, 1 << 16, np.float32),
    ])
    y = _f32([
        rng.choice(phys, 1 << 16), u(-3.0, 3.0, (1 << 16) + 37),
        gy.ravel(),
        u(124.0, 130.0, 2048), u(-152.0, -124.0, 2048),                          # overflow; subnormal results, 0
        u(-3.0, 3.0, 1024),
        rng.integers(-9, 10, 1024).astype(float),
        random_bits(rng, 1 << 16, np.float32),
    ])
    return _finish(x), _finish(y)


@functools.lru_cache(maxsize=None)
def divf_args():
    """fp32 cl_div over its domain: normal divisors 2^-126 <= |d| < 2^126 and
    numerators 2^-100 <= |n| <= 2^100 (every residual is exact); the quotients
    reach from the subnormal range to overflow, and the test asserts the finite
    normal ones, down to 2^-126."""
    rng = np.random.default_rng(20250309)
    n = N_RANDOM
    d = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-125.9, 125.9, n)).astype(np.float32)
    num = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-100.0, 100.0, n)).astype(np.float32)
    d[:1 << 15] = (10.0 ** rng.uniform(-12.0, 5.0, 1 << 15)).astype(np.float32)      # CLOUDSC-like
    num[:1 << 14] = (10.0 ** rng.uniform(-12.0, 5.0, 1 << 14)).astype(np.float32)
    # small quotients on purpose: 2^-126 <= |q| < 2^-100
    k = 1 << 14
    d[-k:] = (2.0 ** rng.uniform(30.0, 125.9, k)).astype(np.float32)
    num[-k:] = (d[-k:].astype(np.float64) * 2.0 ** rng.uniform(-125.5, -100.0, k)).astype(np.float32)
    return _finish(num), _finish(d)
