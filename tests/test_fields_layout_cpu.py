"""Layout conversion (cloudsc_fields_convert_layout / cloudsc_cpu_fields_convert_layout), the part that needs
no GPU: the argument rules of both entry points, and the host form against the NumPy restatement
L[g, r] = B[g // np, r, g % np] (tests/fields_layout_cases.py) on raw bits, in both directions."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_convert_cases as fc
import fields_layout_cases as lc

B, L = lc.B, lc.L


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def call(lib, gpu, ngptot, klev, outputs, sp, sl, snp, sf, dp, dl, dnp, df):
    """Either entry point on raw arguments (sf / df: a Fields or None)."""
    a = (ngptot, klev, outputs, sp, sl, snp, C.byref(sf) if sf is not None else None,
         dp, dl, dnp, C.byref(df) if df is not None else None)
    return lib.cloudsc_fields_convert_layout(0, None, *a) if gpu else lib.cloudsc_cpu_fields_convert_layout(1, *a)


def cpu_convert(lib, src, dst, names=None, nthreads=3, outputs=None):
    ca.check(lib.cloudsc_cpu_fields_convert_layout(
        nthreads, src.ngptot, src.klev, src.outputs if outputs is None else outputs, src.precision, src.layout,
        src.nproma, C.byref(src.fields(names)), dst.precision, dst.layout, dst.nproma, C.byref(dst.fields(names))))


# ---------------------------------------------------------------------------
# argument rules: CLOUDSC_EINVAL from both entry points, before any device is looked for
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sl,dl", [(B, L), (L, B), (L, L), (B, B)], ids=["b2l", "l2b", "l2l", "b2b"])
@pytest.mark.parametrize("gpu", [False, True], ids=["cpu", "gpu"])
def test_argument_rules(lib, gpu, sl, dl):
    n, klev, ALL = 20, 3, ca.OUTPUTS_ALL
    snp, dnp = (0 if sl == L else 8), (0 if dl == L else 16)
    src = lc.HostSet(sl, n, snp, klev, ca.FP64).fill_random()
    dst = lc.HostSet(dl, n, dnp, klev, ca.MIXED)
    sf, df = src.fields(), dst.fields()
    bad = lambda *a: call(lib, gpu, *a) == ca.EINVAL
    if not gpu:
        assert call(lib, gpu, n, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, dnp, df) == 0   # the well-formed call
        dst = lc.HostSet(dl, n, dnp, klev, ca.MIXED)
        df = dst.fields()
    # an unknown layout
    for code in (2, -1, 64):
        assert bad(n, klev, ALL, ca.FP64, code, snp, sf, ca.MIXED, dl, dnp, df)
        assert bad(n, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, code, dnp, df)
    # a non-zero NPROMA on a LEVELS side; no NPROMA on a BLOCKED side
    for v in (1, n, 64, -1):
        if sl == L:
            assert bad(n, klev, ALL, ca.FP64, sl, v, sf, ca.MIXED, dl, dnp, df)
        if dl == L:
            assert bad(n, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, v, df)
    if sl == B:
        for v in (0, -1, (1 << 24) + 1):
            assert bad(n, klev, ALL, ca.FP64, sl, v, sf, ca.MIXED, dl, dnp, df)
    if dl == B:
        for v in (0, -1, (1 << 24) + 1):
            assert bad(n, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, v, df)
    # an unknown output selection
    for code in (2, 3, 4, 6, -1):
        assert bad(n, klev, code, ca.FP64, sl, snp, sf, ca.MIXED, dl, dnp, df)
    # what the table rules refuse: a member that is NULL in exactly one of the two sets
    one = dst.fields()
    one.pq = None
    assert bad(n, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, dnp, one)
    one = src.fields()
    one.ktype = None
    assert bad(n, klev, ALL, ca.FP64, sl, snp, one, ca.MIXED, dl, dnp, df)
    # no member to convert
    assert bad(n, klev, ALL, ca.FP64, sl, snp, ca.Fields(), ca.MIXED, dl, dnp, ca.Fields())
    # the same pointer for a member in src and dst (a transposed member, and a member of one row)
    for name in ("pclv", "plsm"):
        same = dst.fields()
        setattr(same, name, getattr(sf, name))
        assert bad(n, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, dnp, same)
    # an unknown precision code
    for code in (0, 2, 16, -8):
        assert bad(n, klev, ALL, code, sl, snp, sf, ca.MIXED, dl, dnp, df)
        assert bad(n, klev, ALL, ca.FP64, sl, snp, sf, code, dl, dnp, df)
    # ngptot or klev < 1
    for v in (0, -1):
        assert bad(v, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, dnp, df)
        assert bad(n, v, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, dnp, df)
    # a NULL struct
    assert bad(n, klev, ALL, ca.FP64, sl, snp, None, ca.MIXED, dl, dnp, df)
    assert bad(n, klev, ALL, ca.FP64, sl, snp, sf, ca.MIXED, dl, dnp, None)
    # no refused call wrote anything
    for name in dst.names:
        assert dst.untouched(name), name


# ---------------------------------------------------------------------------
# the host form against the NumPy restatement, both directions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,storage", lc.CASES, ids=lc.CASE_IDS)
def test_cpu_form_matches_numpy(lib, shape, storage):
    (ngptot, nproma, klev), (sp, dp) = shape, storage
    blocked = lc.HostSet(B, ngptot, nproma, klev, sp).fill_random(1)
    levels = lc.HostSet(L, ngptot, 0, klev, dp)
    cpu_convert(lib, blocked, levels)
    lc.check_against_numpy(blocked, levels)       # ktype and the surface members included
    levels = lc.HostSet(L, ngptot, 0, klev, sp).fill_random(2)
    blocked = lc.HostSet(B, ngptot, nproma, klev, dp)
    cpu_convert(lib, levels, blocked)
    lc.check_against_numpy(levels, blocked)       # padding lanes and guard margins keep the sentinel


def test_restatement_is_the_issue_formula():
    """The helpers of fields_layout_cases.py say L[g, r] = B[g // np, r, g % np], spelled out once."""
    src = lc.HostSet(B, 70, 16, 3, ca.FP64, names=["paph"]).fill_random()
    dst = lc.HostSet(L, 70, 0, 3, ca.FP64, names=["paph"])
    exp = lc.expected(src, dst, "paph")
    for g in (0, 15, 16, 69):
        for r in range(4):
            assert fc.bits(exp[g, r]) == fc.bits(src.arrays["paph"][g // 16, r, g % 16])


def test_thread_count_does_not_matter(lib):
    src = lc.HostSet(B, 700, 24, 17, ca.FP64).fill_random()
    back = lc.HostSet(L, 700, 0, 17, ca.MIXED).fill_random()
    for nthreads in (1, 2, 64, 0):
        dst = src.like(L, precision=ca.MIXED)
        cpu_convert(lib, src, dst, nthreads=nthreads)
        lc.check_against_numpy(src, dst)
        dst = back.like(B, nproma=24, precision=ca.FP64)
        cpu_convert(lib, back, dst, nthreads=nthreads)
        lc.check_against_numpy(back, dst)


# ---------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [ca.FP64, ca.FP32], ids=["double", "float"])
@pytest.mark.parametrize("sl,dl", [(B, L), (L, B)], ids=["b2l", "l2b"])
def test_equal_sizes_move_bits(lib, precision, sl, dl):
    """Signalling and quiet NaNs with payloads, -0.0, subnormals and infinities survive a copy between
    equal storage sizes bit for bit."""
    ut = np.uint64 if precision == ca.FP64 else np.uint32
    special = {np.uint64: [0x7FF0000000000001, 0x7FF8DEADBEEF0001, 0xFFF4000000000123, 0x8000000000000000,
                           0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000],
               np.uint32: [0x7F800001, 0x7FC0BEEF, 0xFFA00123, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000,
                           0xFF800000]}[ut]
    n, klev = 70, 4
    src = lc.HostSet(sl, n, 0 if sl == L else 16, klev, precision, names=["pt", "pclv"]).fill_random()
    for name in src.names:
        cols = np.array(src.columns(name))
        flat = cols.view(ut).reshape(-1)
        flat[::3] = np.resize(np.array(special, dtype=ut), flat[::3].size)
        src.set_columns(name, cols)
        assert np.array_equal(fc.bits(np.array(src.columns(name))), cols.view(ut))
    dst = src.like(dl, nproma=16)
    cpu_convert(lib, src, dst)
    for name in src.names:
        assert np.array_equal(fc.bits(np.array(dst.columns(name))), fc.bits(np.array(src.columns(name)))), name
    lc.check_against_numpy(src, dst)


@pytest.mark.parametrize("sl,dl", [(B, L), (L, B)], ids=["b2l", "l2b"])
def test_narrowing_edges(lib, sl, dl):
    """The narrowing edges of fields_convert_cases.py through a transposed member: one conversion, round
    to nearest even, gradual underflow, overflow to infinity."""
    v = fc.narrowing_edges()
    n, klev = v.size, 2
    src = lc.HostSet(sl, n, 0 if sl == L else 4, klev, ca.FP64, names=["pt"])
    src.set_columns("pt", np.stack([v, v[::-1]]))
    dst = src.like(dl, nproma=8, precision=ca.MIXED)
    cpu_convert(lib, src, dst)
    got = np.array(dst.columns("pt"))
    with np.errstate(over="ignore", under="ignore"):
        exp = np.stack([v, v[::-1]]).astype(np.float32)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(fc.bits(got)[~nan], fc.bits(exp)[~nan])
    f32 = np.float32
    assert got[0, 0] == f32(1.0) and got[0, 1] == f32(1.0 + 2.0 ** -22)
    assert got[0, 2] == 0.0 and not np.signbit(got[0, 2]) and got[0, 3] == f32(2.0 ** -149)
    assert got[0, 4] == f32(2.0 ** -126) and np.isposinf(got[0, 5])
    assert dst.guard_intact("pt")


# ---------------------------------------------------------------------------
# subsets, the surface selection, round trips
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("names", [lc.INPUTS, lc.OUTPUTS], ids=["inputs", "outputs"])
@pytest.mark.parametrize("sl,dl", [(B, L), (L, B)], ids=["b2l", "l2b"])
def test_subset_writes_only_its_members(lib, sl, dl, names):
    src = lc.HostSet(sl, 150, 0 if sl == L else 24, 17, ca.FP64).fill_random()
    dst = src.like(dl, nproma=64, precision=ca.MIXED)
    cpu_convert(lib, src, dst, names=names)
    lc.check_against_numpy(src, dst, names=names)
    for n in dst.names:
        if n not in names:
            assert dst.untouched(n), n


@pytest.mark.parametrize("sl,dl", [(B, L), (L, B), (L, L), (B, B)], ids=["b2l", "l2b", "l2l", "b2b"])
def test_outputs_surface_members_are_one_row(lib, sl, dl):
    """With OUTPUTS_SURFACE the four flux members are [ngptot] on a LEVELS side and [nblocks][nproma] on a
    BLOCKED one; the guard margin right after them shows that one row and no more is written."""
    names = list(ca.SURFACE_FLUX_FIELDS) + ["pcovptot", "tendency_loc_cld", "plude"]
    src = lc.HostSet(sl, 150, 0 if sl == L else 24, 17, ca.FP64, names, ca.OUTPUTS_SURFACE).fill_random()
    dst = lc.HostSet(dl, 150, 0 if dl == L else 64, 17, ca.MIXED, names, ca.OUTPUTS_SURFACE)
    assert dst.arrays["pfplsl"].size == (150 if dl == L else 192)
    cpu_convert(lib, src, dst)
    lc.check_against_numpy(src, dst)
    # and under OUTPUTS_ALL and OUTPUTS_PROGNOSTIC the same members are half-level profiles
    for outputs in (ca.OUTPUTS_ALL, ca.OUTPUTS_PROGNOSTIC):
        src = lc.HostSet(sl, 150, 0 if sl == L else 24, 17, ca.FP64, names).fill_random()
        dst = lc.HostSet(dl, 150, 0 if dl == L else 64, 17, ca.MIXED, names)
        cpu_convert(lib, src, dst, outputs=outputs)
        lc.check_against_numpy(src, dst)


def test_round_trip_is_the_plain_convert(lib):
    """B(24) -> L -> B(64) is cloudsc_cpu_fields_convert 24 -> 64 on raw bits, guard margins included."""
    for sp, dp in lc.STORAGE:
        b24 = lc.HostSet(B, 300, 24, 17, sp).fill_random()
        lev = b24.like(L)
        b64, ref = b24.like(B, nproma=64, precision=dp), b24.like(B, nproma=64, precision=dp)
        cpu_convert(lib, b24, lev)
        cpu_convert(lib, lev, b64)
        ca.check(lib.cloudsc_cpu_fields_convert(2, 300, 17, sp, 24, C.byref(b24.fields()), dp, 64,
                                                C.byref(ref.fields())))
        lc.same_sets(b64, ref)


def test_levels_to_levels_forwards(lib):
    """L -> L is the plain convert over one block of ngptot columns: the same element positions."""
    for sp, dp in lc.STORAGE:
        a = lc.HostSet(L, 300, 0, 17, sp).fill_random()
        b, ref = a.like(precision=dp), a.like(precision=dp)
        cpu_convert(lib, a, b)
        lc.check_against_numpy(a, b)
        ca.check(lib.cloudsc_cpu_fields_convert(2, 300, 17, sp, 300, C.byref(a.fields()), dp, 300,
                                                C.byref(ref.fields())))
        lc.same_sets(b, ref)


def test_blocked_to_blocked_forwards(lib):
    a = lc.HostSet(B, 300, 24, 17, ca.FP64).fill_random()
    b, ref = a.like(nproma=64, precision=ca.MIXED), a.like(nproma=64, precision=ca.MIXED)
    cpu_convert(lib, a, b)
    ca.check(lib.cloudsc_cpu_fields_convert(2, 300, 17, ca.FP64, 24, C.byref(a.fields()), ca.MIXED, 64,
                                            C.byref(ref.fields())))
    lc.same_sets(b, ref)


# ---------------------------------------------------------------------------
# Python
# ---------------------------------------------------------------------------
def test_python_mirror(lib):
    src = lc.HostSet(L, 100, 0, 5, ca.FP64, names=["paph", "pclv", "ktype"]).fill_random()
    dst = src.like(B, nproma=64, precision=ca.FP32)
    ca.cpu_convert_fields_layout(src.fields(), dst.fields(), 100, 5, ca.FP64, L, 0, ca.FP32, B, 64, nthreads=1)
    lc.check_against_numpy(src, dst)
    with pytest.raises(ca.CloudscError) as err:
        ca.cpu_convert_fields_layout(src.fields(), dst.fields(), 100, 5, ca.FP64, L, 100, ca.FP32, B, 64)
    assert err.value.code == ca.EINVAL


def test_step_wrappers_refuse_a_levels_set():
    f = ca.LevelsFields()
    p = ca.Params()
    for fn, args in [(ca.gpu_run_outputs, (f, ca.FP64, ca.VARIANT_KCACHE, ca.OUTPUTS_ALL, 10, 10, 3)),
                     (ca.cpu_run_outputs, (p, f, ca.FP64, ca.OUTPUTS_ALL, 10, 10, 3)),
                     (ca.gpu_run_tendbuf, (f, ca.FP64, ca.VARIANT_KCACHE, 10, 10, 3, 8)),
                     (ca.cpu_run_tendbuf, (p, f, ca.FP64, 10, 10, 3, 8))]:
        with pytest.raises(ValueError, match="LAYOUT_LEVELS"):
            fn(*args)
