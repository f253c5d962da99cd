"""Field set conversion (cloudsc_fields_convert / cloudsc_cpu_fields_convert), the part that needs no GPU:
the argument rules of both entry points, and the host form against a NumPy restatement written here
(tests/fields_convert_cases.py), on raw bits."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_convert_cases as fc


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def call(lib, gpu, ngptot, klev, sp, snp, sf, dp, dnp, df):
    """Either entry point on raw arguments (sf / df: a Fields or None)."""
    a = (ngptot, klev, sp, snp, C.byref(sf) if sf is not None else None, dp, dnp, C.byref(df) if df is not None else None)
    return lib.cloudsc_fields_convert(0, None, *a) if gpu else lib.cloudsc_cpu_fields_convert(1, *a)


def cpu_convert(lib, src, dst, names=None, nthreads=3):
    ca.check(lib.cloudsc_cpu_fields_convert(nthreads, src.ngptot, src.klev, src.precision, src.nproma,
                                            C.byref(src.fields(names)), dst.precision, dst.nproma,
                                            C.byref(dst.fields(names))))


# ---------------------------------------------------------------------------
# argument rules: CLOUDSC_EINVAL from both entry points, before any device is looked for
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gpu", [False, True], ids=["cpu", "gpu"])
def test_argument_rules(lib, gpu):
    n, klev = 20, 3
    src = fc.HostSet(n, 8, klev, ca.FP64).fill_encoded()
    dst = fc.HostSet(n, 16, klev, ca.MIXED)
    sf, df = src.fields(), dst.fields()
    bad = lambda *a: call(lib, gpu, *a) == ca.EINVAL
    if not gpu:
        assert call(lib, gpu, n, klev, ca.FP64, 8, sf, ca.MIXED, 16, df) == 0       # the well-formed call
    # a member that is NULL in exactly one of the two sets
    one = dst.fields()
    one.pq = None
    assert bad(n, klev, ca.FP64, 8, sf, ca.MIXED, 16, one)
    assert bad(n, klev, ca.FP64, 8, one, ca.MIXED, 16, sf)
    # no member to convert
    assert bad(n, klev, ca.FP64, 8, ca.Fields(), ca.MIXED, 16, ca.Fields())
    # the same pointer for a member in src and dst
    same = dst.fields()
    same.pclv = sf.pclv
    assert bad(n, klev, ca.FP64, 8, sf, ca.MIXED, 16, same)
    assert bad(n, klev, ca.FP64, 8, sf, ca.FP64, 8, sf)
    # an unknown precision code
    for code in (0, 2, 16, -8):
        assert bad(n, klev, code, 8, sf, ca.MIXED, 16, df)
        assert bad(n, klev, ca.FP64, 8, sf, code, 16, df)
    # ngptot, klev or either NPROMA < 1, NPROMA > 2^24
    for v in (0, -1):
        assert bad(v, klev, ca.FP64, 8, sf, ca.MIXED, 16, df)
        assert bad(n, v, ca.FP64, 8, sf, ca.MIXED, 16, df)
        assert bad(n, klev, ca.FP64, v, sf, ca.MIXED, 16, df)
        assert bad(n, klev, ca.FP64, 8, sf, ca.MIXED, v, df)
    assert bad(n, klev, ca.FP64, (1 << 24) + 1, sf, ca.MIXED, 16, df)
    assert bad(n, klev, ca.FP64, 8, sf, ca.MIXED, (1 << 24) + 1, df)
    # a NULL struct
    assert bad(n, klev, ca.FP64, 8, None, ca.MIXED, 16, df)
    assert bad(n, klev, ca.FP64, 8, sf, ca.MIXED, 16, None)
    if gpu:
        # no refused call wrote anything
        for name in dst.names:
            assert np.all(dst.full[name].view(np.uint8) == fc.SENTINEL_BYTE), name


def test_nproma_limit_is_inclusive(lib):
    """NPROMA = 2^24 itself is accepted (one block of a 10-column problem)."""
    src = fc.HostSet(10, 1 << 24, 1, ca.FP64, names=["plsm"])
    src.arrays["plsm"][0, 0, :10] = np.arange(10)
    dst = fc.HostSet(10, 4, 1, ca.FP64, names=["plsm"])
    cpu_convert(lib, src, dst)
    assert np.array_equal(fc.to_columns(dst.arrays["plsm"], 10)[0], np.arange(10.0))


# ---------------------------------------------------------------------------
# the host form against the NumPy restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sp,dp", fc.STORAGE, ids=["d2d", "d2f", "f2d", "f2f"])
@pytest.mark.parametrize("ngptot,snp,dnp", fc.SHAPES)
def test_cpu_form_matches_numpy(lib, ngptot, snp, dnp, sp, dp):
    src = fc.HostSet(ngptot, snp, fc.KLEV, sp).fill_encoded()
    dst = fc.HostSet(ngptot, dnp, fc.KLEV, dp)
    cpu_convert(lib, src, dst)
    fc.check_against_numpy(src, dst)       # ktype included; padding lanes and guard margins keep the sentinel
    # the values still name their (member, row, column): nothing was moved to the wrong place
    for n in dst.names:
        assert np.array_equal(fc.to_columns(dst.arrays[n], ngptot), fc.encoded(n, fc.rows_of(n, fc.KLEV), ngptot)), n


@pytest.mark.parametrize("sp,dp", [(ca.FP64, ca.MIXED), (ca.MIXED, ca.FP64)], ids=["d2f", "f2d"])
def test_cpu_form_klev_137(lib, sp, dp):
    src = fc.HostSet(150, 24, 137, sp).fill_encoded()
    dst = fc.HostSet(150, 64, 137, dp)
    cpu_convert(lib, src, dst, nthreads=0)
    fc.check_against_numpy(src, dst)


def test_thread_count_does_not_matter(lib):
    src = fc.HostSet(150, 24, fc.KLEV, ca.FP64).fill_encoded()
    for nthreads in (1, 2, 64):
        dst = fc.HostSet(150, 8, fc.KLEV, ca.MIXED)
        cpu_convert(lib, src, dst, nthreads=nthreads)
        fc.check_against_numpy(src, dst)


# ---------------------------------------------------------------------------
# narrowing
# ---------------------------------------------------------------------------
def test_narrowing_edges(lib):
    """One fp64 field holding the edge values: ties to even both ways, the two half-way cases at the
    subnormal floor, the subnormal boundary, overflow, signed zeros and infinities, a NaN."""
    v = fc.narrowing_edges()
    n = v.size
    src = fc.HostSet(n, n, 1, ca.FP64, names=["pt"])
    src.arrays["pt"][0, 0, :] = v
    dst = fc.HostSet(n, 4, 1, ca.MIXED, names=["pt"])
    cpu_convert(lib, src, dst)
    got = fc.to_columns(dst.arrays["pt"], n)[0]
    with np.errstate(over="ignore", under="ignore"):
        exp = v.astype(np.float32)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(fc.bits(got)[~nan], fc.bits(exp)[~nan]), (got, exp)
    # what the restatement says, spelled out: the rules of the contract
    f32 = lambda x: np.float32(x)
    assert got[0] == f32(1.0) and got[1] == f32(1.0 + 2.0 ** -22)
    assert got[2] == 0.0 and not np.signbit(got[2]) and got[3] == f32(2.0 ** -149)
    assert got[4] == f32(2.0 ** -126) and np.isposinf(got[5])
    assert dst.guard_intact("pt")


# ---------------------------------------------------------------------------
# subsets and round trips
# ---------------------------------------------------------------------------
def test_subset_writes_only_its_members(lib):
    src = fc.HostSet(150, 24, fc.KLEV, ca.FP64).fill_encoded()
    dst = fc.HostSet(150, 64, fc.KLEV, ca.MIXED)
    cpu_convert(lib, src, dst, names=["pt", "pclv"])
    fc.check_against_numpy(src, dst, names=["pt", "pclv"])
    for n in dst.names:
        if n not in ("pt", "pclv"):
            assert np.all(dst.full[n].view(np.uint8) == fc.SENTINEL_BYTE), n


def test_round_trips(lib, ds):
    """fp64 -> float -> fp64 is astype(float32).astype(float64); fp64 8 -> 64 -> 8 is the identity.
    On the dataset's own values (not float-representable)."""
    n = 150
    a = ca.make_host_state(ds, n, 8, ca.FP64)
    names = [k for k in a.arrays if k not in ca.OUTPUT_FIELDS]
    b = ca.make_host_state(ds, n, 64, ca.MIXED)
    c = ca.make_host_state(ds, n, 8, ca.FP64)
    d = ca.make_host_state(ds, n, 64, ca.FP64)
    e = ca.make_host_state(ds, n, 8, ca.FP64)
    for st in (b, c, d, e):
        for k in names:
            st.arrays[k][...] = 0
    ca.cpu_convert_fields(a, b, names=names)
    ca.cpu_convert_fields(b, c, names=names)
    ca.cpu_convert_fields(a, d, names=names, nthreads=2)
    ca.cpu_convert_fields(d, e, names=names, nthreads=2)
    cols = lambda st, k: ca.blocks_to_columns(st.arrays[k], n)     # (padding lanes are not converted)
    for k in names:
        with np.errstate(over="ignore", under="ignore"):
            exp = cols(a, k) if k == "ktype" else cols(a, k).astype(np.float32).astype(np.float64)
        assert np.array_equal(fc.bits(cols(c, k)), fc.bits(exp)), k
        assert np.array_equal(fc.bits(cols(e, k)), fc.bits(cols(a, k))), k
    assert any(not np.array_equal(cols(c, k), cols(a, k)) for k in names)       # the rounding did something


def test_python_mirror_on_plain_fields(lib):
    src = fc.HostSet(100, 100, fc.KLEV, ca.FP64, names=["paph", "ktype"]).fill_encoded()
    dst = fc.HostSet(100, 64, fc.KLEV, ca.FP32, names=["paph", "ktype"])
    ca.cpu_convert_fields(src.fields(), dst.fields(), 100, fc.KLEV, ca.FP64, 100, ca.FP32, 64, nthreads=1)
    fc.check_against_numpy(src, dst)
    with pytest.raises(ca.CloudscError) as err:
        ca.cpu_convert_fields(src.fields(), dst.fields(["paph"]), 100, fc.KLEV, ca.FP64, 100, ca.FP32, 64)
    assert err.value.code == ca.EINVAL
