"""Field set comparison, validation and expansion without a GPU: the argument rules of the four entry
points (CLOUDSC_EINVAL before any HIP call, so also on a machine without a device) and the host twin
cloudsc_cpu_fields_compare against the restatement of tests/fields_compare_cases.py."""
import ctypes as C

import numpy as np
import pytest

import cloudsc_amd as ca
import fields_compare_cases as cc
import fields_convert_cases as fc


@pytest.fixture(scope="module")
def lib():
    return ca.gpu_lib()


def cpu_compare(lib, a, b, names=None, nthreads=2):
    d = cc.new_diffs()
    ca.check(lib.cloudsc_cpu_fields_compare(nthreads, a.ngptot, a.klev, a.precision, a.nproma,
                                            C.byref(a.fields(names)), b.precision, b.nproma, C.byref(b.fields(names)),
                                            d))
    return d


# ---------------------------------------------------------------------------
# ABI and argument rules
# ---------------------------------------------------------------------------
def test_members_and_diff_size(lib):
    assert lib.cloudsc_fields_members() == len(ca.ALL_FIELDS)
    assert lib.cloudsc_fields_diff_sizeof() == C.sizeof(ca.FieldDiff) == 7 * 8 + 4 * 8


def compare_calls(lib):
    """(name, call(ngptot, klev, ap, anp, fa, bp, bnp, fb, diff)) of the device form and the host twin"""
    return [("device", lambda *x: lib.cloudsc_fields_compare(0, None, *x)),
            ("host", lambda *x: lib.cloudsc_cpu_fields_compare(1, *x))]


@pytest.mark.parametrize("which", [0, 1], ids=["device", "host"])
def test_compare_einval(lib, which):
    call = compare_calls(lib)[which][1]
    a, b, _ = cc.make_pair(10, 4, 8, 2, ca.FP64, ca.MIXED, names=["pt", "ktype"])
    fa, fb, d = a.fields(), b.fields(), cc.new_diffs()
    ok = (10, 2, ca.FP64, 4, C.byref(fa), ca.MIXED, 8, C.byref(fb), d)

    def with_(i, v):
        x = list(ok)
        x[i] = v
        return call(*x)
    assert with_(0, 0) == ca.EINVAL and with_(1, 0) == ca.EINVAL            # sizes
    assert with_(3, 0) == ca.EINVAL and with_(6, -1) == ca.EINVAL           # an NPROMA < 1
    assert with_(3, (1 << 24) + 1) == ca.EINVAL and with_(6, (1 << 24) + 1) == ca.EINVAL
    assert with_(2, 7) == ca.EINVAL and with_(5, 0) == ca.EINVAL            # precision codes
    assert with_(4, None) == ca.EINVAL and with_(7, None) == ca.EINVAL and with_(8, None) == ca.EINVAL
    only_pt = a.fields(["pt"])                                              # ktype in exactly one set
    assert with_(4, C.byref(only_pt)) == ca.EINVAL and with_(7, C.byref(only_pt)) == ca.EINVAL
    empty = ca.Fields()
    x = list(ok)
    x[4] = x[7] = C.byref(empty)
    assert call(*x) == ca.EINVAL                                            # no member in both


def test_validate_einval(lib, ds):
    st = ca.make_host_state(ds, 10, 4)
    f = st.fields()
    keep = []
    ref = ca.make_reference(ds, keep)
    stats = (ca.Stats * 21)()
    ok = [0, None, ca.FP64, 10, 4, ds.klev, 0, C.byref(f), C.byref(ref), stats]

    def with_(i, v):
        x = list(ok)
        x[i] = v
        return lib.cloudsc_fields_validate(*x)
    assert with_(2, 5) == ca.EINVAL
    assert with_(3, 0) == ca.EINVAL and with_(4, 0) == ca.EINVAL and with_(4, (1 << 24) + 1) == ca.EINVAL
    assert with_(5, ds.klev - 1) == ca.EINVAL and with_(5, 0) == ca.EINVAL      # not the reference's klev
    assert with_(6, -1) == ca.EINVAL
    assert with_(7, None) == ca.EINVAL and with_(8, None) == ca.EINVAL and with_(9, None) == ca.EINVAL
    g = ca.fields_subset(f)
    g.pfplsl = None                                                            # a validated member missing
    assert with_(7, C.byref(g)) == ca.EINVAL
    r2 = ca.make_reference(ds, keep)
    r2.field[3] = None
    assert with_(8, C.byref(r2)) == ca.EINVAL
    r3 = ca.make_reference(ds, keep)
    r3.klon = 0
    assert with_(8, C.byref(r3)) == ca.EINVAL


def test_expand_einval(lib, ds):
    st = ca.make_host_state(ds, 10, 4)
    f = st.fields()
    keep = []
    t = ca.make_template(ds, keep)
    ok = [0, None, ca.FP64, 10, 4, 0, C.byref(t), C.byref(f)]

    def with_(i, v):
        x = list(ok)
        x[i] = v
        return lib.cloudsc_fields_expand(*x)
    assert with_(2, 16) == ca.EINVAL
    assert with_(3, 0) == ca.EINVAL and with_(4, 0) == ca.EINVAL and with_(4, (1 << 24) + 1) == ca.EINVAL
    assert with_(5, -1) == ca.EINVAL
    assert with_(6, None) == ca.EINVAL and with_(7, None) == ca.EINVAL
    outs = ca.fields_subset(f, list(ca.OUTPUT_FIELDS))                         # no input member to fill
    assert with_(7, C.byref(outs)) == ca.EINVAL
    t2 = ca.make_template(ds, keep)
    t2.pq = None                                                               # a member to fill without its template
    assert with_(6, C.byref(t2)) == ca.EINVAL
    t3 = ca.make_template(ds, keep)
    t3.klon = 0
    assert with_(6, C.byref(t3)) == ca.EINVAL


def test_compare_grid_knob_range(lib):
    assert lib.cloudsc_debug_set_compare_grid(-1) == ca.EINVAL
    assert lib.cloudsc_debug_set_compare_grid((1 << 16) + 1) == ca.EINVAL
    assert lib.cloudsc_debug_set_compare_grid(3) == 0 and lib.cloudsc_debug_set_compare_grid(0) == 0


# ---------------------------------------------------------------------------
# the host twin against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ap,bp", cc.STORAGE, ids=cc.STORAGE_IDS)
@pytest.mark.parametrize("ngptot,anp,bnp", cc.SHAPES)
def test_host_twin_matches_restatement(lib, ngptot, anp, bnp, ap, bp):
    a, b, pos = cc.make_pair(ngptot, anp, bnp, cc.KLEV, ap, bp)
    exp = cc.restate(a, b)
    assert sum(e["mismatches"] for e in exp.values()) == len(set(pos))     # every planted position differs
    zero = exp["pt"]
    assert zero["first"] == (0, 0) and zero["min"] == 0.0                  # the +0 / -0 pair: a mismatch with d = 0
    cc.check_against_restatement(cpu_compare(lib, a, b), exp)


@pytest.mark.parametrize("ap,bp", cc.STORAGE, ids=cc.STORAGE_IDS)
@pytest.mark.parametrize("ngptot,anp,bnp", cc.TALL_SHAPES)
def test_host_twin_klev_137(lib, ngptot, anp, bnp, ap, bp):
    a, b, pos = cc.make_pair(ngptot, anp, bnp, cc.TALL_KLEV, ap, bp, names=cc.OUTPUTS)
    exp = cc.restate(a, b)
    assert sum(e["mismatches"] for e in exp.values()) == len(set(pos))
    cc.check_against_restatement(cpu_compare(lib, a, b), exp)


def test_subset_and_same_pointer(lib):
    a, b, _ = cc.make_pair(150, 24, 64, cc.KLEV, ca.FP64, ca.MIXED)
    exp = cc.restate(a, b, names=["pq", "pclv"])
    cc.check_against_restatement(cpu_compare(lib, a, b, names=["pq", "pclv"]), exp)
    same = cpu_compare(lib, a, a)                                           # the same pointers: nothing is written
    assert all(same[m].mismatches == 0 and same[m].stats.maxerr == 0.0 and same[m].compared > 0
               for m in range(len(fc.MEMBERS)))


@pytest.mark.parametrize("ap,bp", cc.STORAGE, ids=cc.STORAGE_IDS)
@pytest.mark.parametrize("ngptot,anp,bnp", [(150, 24, 64), (150, 64, 150), (130, 1, 64)])
def test_identical_sets(lib, ngptot, anp, bnp, ap, bp):
    """The same float-exact values in two blockings and storage types: no mismatch, max |d| = 0."""
    a, b, _ = cc.make_pair(ngptot, anp, bnp, cc.KLEV, ap, bp, plant=False)
    d = cpu_compare(lib, a, b)
    for m, n in enumerate(fc.MEMBERS):
        assert d[m].compared == fc.rows_of(n, cc.KLEV) * ngptot, n
        assert (d[m].mismatches, d[m].first_column, d[m].first_row) == (0, -1, -1), n
        assert d[m].stats.maxerr == 0.0 and d[m].stats.errsum == 0.0 and d[m].stats.errsum_lo == 0.0, n


def test_nan_contract(lib):
    """A NaN in an active lane: NaN sums; min, max and max |d| skip it; it is a mismatch unless the other
    set holds the same word."""
    a, b, _ = cc.make_pair(150, 24, 64, cc.KLEV, ca.FP64, ca.FP64, names=["pt", "pq"], plant=False)
    a.arrays["pt"][1, 2, 5] = np.nan                  # global column 29, row 2
    a.arrays["pq"][0, 1, 3] = np.nan                  # global column 3, row 1 ...
    b.arrays["pq"][0, 1, 3] = np.nan                  # ... the same word in b
    d = cpu_compare(lib, a, b)
    pt, pq = d[fc.MEMBERS.index("pt")], d[fc.MEMBERS.index("pq")]
    assert (pt.mismatches, pt.first_column, pt.first_row) == (1, 29, 2)
    assert (pq.mismatches, pq.first_column, pq.first_row) == (0, -1, -1)
    for x in (pt, pq):
        assert np.isnan(x.stats.errsum) and x.stats.maxerr == 0.0
        assert not np.isnan(x.stats.minval) and not np.isnan(x.stats.maxval)
    assert np.isnan(pq.stats.refsum) and not np.isnan(pt.stats.refsum)


def test_thread_independence(lib):
    a, b, _ = cc.make_pair(1000, 64, 24, cc.TALL_KLEV, ca.FP64, ca.MIXED, names=cc.OUTPUTS)
    runs = [cpu_compare(lib, a, b, nthreads=t) for t in (1, 3, 16)]
    for m in range(len(fc.MEMBERS)):
        assert len({cc.exact_fields(r[m]) for r in runs}) == 1, fc.MEMBERS[m]
        assert len({(r[m].stats.errsum, r[m].stats.refsum) for r in runs}) == 1, fc.MEMBERS[m]


def test_python_host_form(lib):
    """cpu_compare_fields on HostStates: the dict form, skipped members left out."""
    a, b, _ = cc.make_pair(150, 24, 64, cc.KLEV, ca.FP64, ca.MIXED, names=["pt", "pclv"])
    sa = ca.HostState(150, 24, cc.KLEV, ca.FP64, a.arrays)
    sb = ca.HostState(150, 64, cc.KLEV, ca.MIXED, b.arrays)
    got = ca.cpu_compare_fields(sa, sb)
    exp = cc.restate(a, b)
    assert sorted(got) == ["pclv", "pt"]
    for n in got:
        assert got[n]["mismatches"] == exp[n]["mismatches"] and got[n]["compared"] == exp[n]["compared"]
        assert got[n]["first"] == exp[n]["first"] and got[n]["stats"][2] == exp[n]["maxerr"]
